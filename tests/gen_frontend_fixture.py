"""Writes tests/golden/frontend_*.npz: small synthetic GREATER clips (RGB-D + flat render) and CARLA clips (lidar sweeps)
pushed through the REFERENCE's own functions, stage by stage, on the CPU.  Container-only, like tests/gen_optim_fixture.py:
it imports the real reference through oracle.ref_import.load() (unchanged), the reference's utils/utils.py the same way, and
reads the hue-cluster list out of data/data_greater.py as data.

    python tests/gen_frontend_fixture.py [OUT_DIR]

The steps between the reference's functions (the loops of data/data_greater.py:386-516 and data/data_carla.py:443-623, which
live inside dataset classes that read files) are driven from here in the reference's order with the reference's arguments.

Margin condition, asserted at generation time: no reference point lies within 1e-4 of a filter bound or of the floor-cut
surface, no h * 360 within 1e-3 of a .5 rounding boundary, no rounded hue at (or within 1e-3 of) the midpoint between two
clusters; inputs that violate it are re-drawn until it holds, so that membership and ids never hang on the last bit.

The seeded inputs are rebuilt by the tests from the small integers stored in the files (8-bit colours, 16-bit depth).
"""
import ast
import os
import re
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MARGIN, HUE_MARGIN, MAX_DEPTH = 1e-4, 1e-3, 32.0

GREATER = dict(V=2, T=3, H=48, W=64, other_bounds=5.0, min_z=-1.0, seed=2301)
# (name, keyword arguments of greater_clip, numpy / torch seed); 'a' also stores every stage
GREATER_CASES = [
    ('a', dict(n_points_rnd=1200, n_fps_input=1024, n_fps_target=768, pcl_input_frames=2, pcl_target_frames=2, src_view=0,
               track_id=-1), 77),
    ('b', dict(n_points_rnd=0, n_fps_input=1536, n_fps_target=-900, pcl_input_frames=3, pcl_target_frames=1, src_view=1,
               track_id=4), 78),
    ('c', dict(n_points_rnd=400, n_fps_input=2048, n_fps_target=0, pcl_input_frames=1, pcl_target_frames=3, src_view=1,
               track_id=0), 79),           # (input shorter than n_fps_input: zero padding; targets not subsampled)
]
GREATER_CASES_BY_NAME = {name: kw for name, kw, _ in GREATER_CASES}
CARLA = dict(V=2, T=3, N=1500, min_z=-1.0, other_bounds=20.0, target_bounds=16.0, seed=2302)
CARLA_STAGE_CASES = [(mode, ref) for mode in (1, 2, 3, 4) for ref in (None, -1)]
CARLA_CASES = [
    ('m1', dict(cube_mode=1, reference_frame=None, n_points_rnd=0, n_fps_input=384, n_fps_target=384, pcl_input_frames=2,
                pcl_target_frames=2, correct_origin_ground=True, oversample_vehped_target=False), 81),
    ('m2', dict(cube_mode=2, reference_frame=-1, n_points_rnd=300, n_fps_input=384, n_fps_target=-300, pcl_input_frames=3,
                pcl_target_frames=1, correct_origin_ground=True, oversample_vehped_target=True), 82),
    ('m3', dict(cube_mode=3, reference_frame=None, n_points_rnd=0, n_fps_input=384, n_fps_target=0, pcl_input_frames=1,
                pcl_target_frames=1, correct_origin_ground=False, oversample_vehped_target=False), 83),
    ('m4', dict(cube_mode=4, reference_frame=-1, n_points_rnd=350, n_fps_input=384, n_fps_target=384, pcl_input_frames=3,
                pcl_target_frames=2, correct_origin_ground=True, oversample_vehped_target=False), 84),
]
CARLA_CASES_BY_NAME = {name: kw for name, kw, _ in CARLA_CASES}


# --------------------------------------------------------------------------------------------------------------- inputs
def _look_at(eye, target):
    """(3, 4) world -> camera extrinsics of a camera at `eye` looking at `target` (z forward, y down)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, down, fwd, eye
    return np.linalg.inv(pose)[:3].astype(np.float32)


def greater_cameras(cfg=GREATER):
    V, T, H, W = cfg['V'], cfg['T'], cfg['H'], cfg['W']
    cam_RT = np.stack([np.stack([_look_at([7.0 * np.cos(2.2 * v + 0.15 * t), 7.0 * np.sin(2.2 * v + 0.15 * t), 3.5 + 0.2 * t],
                                          [0.3, -0.2, 0.4]) for t in range(T)]) for v in range(V)])
    cam_K = np.zeros((V, T, 3, 3), dtype=np.float32)
    cam_K[..., 0, 0] = cam_K[..., 1, 1] = 55.5 + np.arange(V)[:, None]
    cam_K[..., 0, 2], cam_K[..., 1, 2], cam_K[..., 2, 2] = W / 2.0, H / 2.0, 1.0
    return cam_RT, cam_K


def images_from_integers(rgb_u8, flat_u8, depth_u16):
    """The float32 frames an 8-bit colour PNG and a 16-bit depth PNG decode to (value / 255, value / 65535 * 32 m)."""
    to_f = lambda a, top: (a.astype(np.float32) / np.float32(top))
    return to_f(rgb_u8, 255), to_f(flat_u8, 255), to_f(depth_u16, 65535) * np.float32(MAX_DEPTH)


def _draw_greater(rng, clusters, cfg=GREATER):
    import matplotlib.colors
    shape = (cfg['V'], cfg['T'], cfg['H'], cfg['W'])
    rgb = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    which = rng.integers(0, len(clusters), size=shape)
    hue = (np.asarray(clusters, np.float64)[which] + rng.uniform(-2.5, 2.5, size=shape)) % 360.0
    hsv = np.stack([hue / 360.0, np.ones(shape), rng.uniform(0.5, 1.0, size=shape)], axis=-1)
    background = rng.uniform(size=shape) < 0.4                                   # low saturation: instance id -1
    hsv[background, 1] = rng.uniform(0.0, 0.6, size=int(background.sum()))
    flat = np.clip(np.round(matplotlib.colors.hsv_to_rgb(hsv) * 255.0), 0, 255).astype(np.uint8)
    depth = rng.integers(int(2.5 / MAX_DEPTH * 65535), int(13.0 / MAX_DEPTH * 65535), size=shape).astype(np.uint16)
    depth[rng.uniform(size=shape) < 0.12] = 0                                    # holes
    return rgb, flat, depth


def _bound_margin(xyz, bounds, floor_fix):
    """Smallest distance of each point (float64 arithmetic on the float32 coordinates) to a decision surface."""
    x, y, z = (xyz[:, i].astype(np.float64) for i in range(3))
    d = np.full(xyz.shape[0], np.inf)
    for c, (lo, hi) in zip((x, y, z), bounds):
        d = np.minimum(d, np.minimum(np.abs(c - np.float32(lo)), np.abs(c - np.float32(hi))))
    if floor_fix:
        d = np.minimum(d, np.abs(z - (np.maximum(np.abs(x), np.abs(y)) - 4.5) / 3.5))
    return d


def _hue_ok(flat, clusters):
    """Margin condition of the instance ids of float32 flat frames (..., 3): a boolean per pixel."""
    import matplotlib.colors
    hsv = matplotlib.colors.rgb_to_hsv(flat)
    deg = hsv[..., 0].astype(np.float64) * 360.0
    frac = deg - np.floor(deg)
    ok = np.abs(frac - 0.5) > HUE_MARGIN
    c = np.sort(np.asarray(clusters, np.float64))
    mids = (c[1:] + c[:-1]) / 2.0
    ok &= np.abs(np.round(deg)[..., None] - mids).min(axis=-1) > HUE_MARGIN
    ok &= np.abs(deg[..., None] - mids).min(axis=-1) > HUE_MARGIN
    ok &= np.abs(hsv[..., 1].astype(np.float64) - 0.9) > HUE_MARGIN
    return ok


# --------------------------------------------------------------------------------------------------------------- reference
def load_reference():
    """(namespace of oracle.ref_import.load(), the reference's utils/utils.py module, its hue-cluster list)."""
    from oracle import ref_import
    ref = ref_import.load()
    root = ref_import.REFERENCE_ROOT
    added = [root] + [os.path.join(root, d) for d in ('data', 'eval', 'model', 'utils')]
    saved = {k: sys.modules.pop(k) for k in ('__init__', 'utils') if k in sys.modules}
    cwd = os.getcwd()
    os.chdir(root)
    sys.path[:0] = added
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            import utils as r_utils
    finally:
        os.chdir(cwd)
        for p in added:
            sys.path.remove(p)
        for k in ('__init__', 'utils'):
            sys.modules.pop(k, None)
        sys.modules.update(saved)
    with open(os.path.join(root, 'data', 'data_greater.py')) as f:
        m = re.search(r'^_PREFLAT_HUE_CLUSTERS\s*=\s*(\[[^\]]*\])', f.read(), flags=re.M)
    return ref, r_utils, ast.literal_eval(m.group(1))


def _greater_frame(ref, clusters, rgb, flat, depth, cam_RT, cam_K):
    """One frame up to the cuboid filter: the reference's functions with the reference's arguments."""
    import matplotlib.colors
    flat_hsv = matplotlib.colors.rgb_to_hsv(flat)
    ids = np.abs(np.round(flat_hsv[..., 0:1] * 360.0)[..., None] - clusters).argmin(axis=-1)
    ids[flat_hsv[..., 1] < 0.9] = -1.0
    return ref.geometry.point_cloud_from_rgbd(np.concatenate([ids, rgb], axis=-1), depth, cam_RT, cam_K).astype(np.float32)


def _tail(ref, r_utils, all_pcl, kw, src_view, target_filter=None, retain=None):
    """From the per-view, per-frame clouds to the final tensors: the reference's functions in the reference's order."""
    g = ref.geometry
    out = {}
    V, T = len(all_pcl), len(all_pcl[0])
    out['pcl_sizes'] = np.array([[all_pcl[v][t].shape[0] for t in range(T)] for v in range(V)])
    video_views = r_utils.accumulate_pcl_time_numpy(all_pcl)
    merged = r_utils.merge_pcl_views_numpy(all_pcl, insert_view_idx=True)
    out['accumulated'] = video_views[src_view].astype(np.float32).copy()
    n_in = sum(all_pcl[src_view][t].shape[0] for t in range(kw['pcl_input_frames']))
    pcl_input = video_views[src_view][:n_in]
    np.random.shuffle(pcl_input)
    pcl_input = torch.from_numpy(np.ascontiguousarray(pcl_input, dtype=np.float32))
    pre = pcl_input.shape[0]
    pcl_input = g.subsample_pad_pcl_torch(pcl_input, kw['n_fps_input'], sample_mode='farthest_point', subsample_only=False)
    out['sample_input_ratios'] = np.array([pcl_input.shape[0] / max(pre, 1)])
    out['pcl_input_size'] = np.int64(min(pre, pcl_input.shape[0]))
    targets, sizes, ratios = [], [], []
    for t in range(kw['pcl_target_frames']):
        frame = merged[-kw['pcl_target_frames'] + t]
        out['merged_%d' % t] = frame.astype(np.float32).copy()
        np.random.shuffle(frame)
        frame = torch.from_numpy(np.ascontiguousarray(frame, dtype=np.float32))
        if target_filter is not None:
            frame = target_filter(frame)
        targets.append(frame)
        sizes.append(frame.shape[0])
    if kw['n_fps_target'] != 0:
        mode = 'farthest_point' if kw['n_fps_target'] > 0 else 'random'
        for i in range(len(targets)):
            pre = targets[i].shape[0]
            extra = {} if retain is None else dict(retain_vehped=retain, segm_idx=5)
            targets[i] = g.subsample_pad_pcl_torch(targets[i], abs(kw['n_fps_target']), sample_mode=mode, subsample_only=False,
                                                   **extra)
            ratios.append(targets[i].shape[0] / max(pre, 1))
            sizes[i] = min(pre, targets[i].shape[0])
    sem = pcl_input[..., 3:-4]
    pcl_input = torch.cat([pcl_input[..., :3], pcl_input[..., -4:]], dim=-1)
    track_in = torch.zeros_like(pcl_input[..., 0:1])
    track_tg = [torch.zeros_like(f[..., 0:1]) for f in targets]
    track_id, inst_col = kw.get('track_id', -1), 3 if retain is None else 4
    if track_id >= 0:                                     # data/data_greater.py:554-560 with the caller's track_id
        track_in[torch.logical_and(sem[..., 0] == track_id, pcl_input[..., -1] == 0)] = 1.0
        for f, m in zip(targets, track_tg):
            m[f[..., inst_col] == track_id] = 1.0
    out['pcl_input'] = torch.cat([pcl_input, track_in], dim=-1).numpy()
    out['pcl_input_sem'] = sem.numpy().copy()
    for i, (f, m) in enumerate(zip(targets, track_tg)):
        out['pcl_target_%d' % i] = torch.cat([f, m], dim=-1).numpy()
    out['pcl_target_size'] = np.array(sizes, dtype=np.int64)
    out['sample_target_ratios'] = np.array(ratios, dtype=np.float64)
    out['np_state'] = np.random.get_state()[1].copy()
    out['np_pos'] = np.int64(np.random.get_state()[2])
    out['torch_state'] = torch.get_rng_state().numpy().copy()
    return out


def _with_index(pcl):
    return np.concatenate([pcl, np.arange(pcl.shape[0], dtype=pcl.dtype)[:, None]], axis=1)


def generate_greater(ref, r_utils, clusters, cfg=GREATER):
    g = ref.geometry
    rng = np.random.default_rng(cfg['seed'])
    cam_RT, cam_K = greater_cameras(cfg)
    rgb_u8, flat_u8, depth_u16 = _draw_greater(rng, clusters, cfg)
    ob, V, T = cfg['other_bounds'], cfg['V'], cfg['T']
    box = dict(x_min=-ob, x_max=ob, y_min=-ob, y_max=ob, z_min=cfg['min_z'], z_max=ob)
    bounds = ((-ob, ob), (-ob, ob), (cfg['min_z'], ob))
    for attempt in range(100):                                                  # re-draw what violates the margin condition
        rgb, flat, depth = images_from_integers(rgb_u8, flat_u8, depth_u16)
        bad_hue = ~_hue_ok(flat, clusters)
        bad_depth = np.zeros(depth.shape, dtype=bool)
        for v in range(V):
            for t in range(T):
                full = _greater_frame(ref, clusters, rgb[v, t], flat[v, t], depth[v, t], cam_RT[v, t], cam_K[v, t])
                ys, xs = np.where(depth[v, t] > 0.0)
                close = _bound_margin(full[:, :3], bounds, True) <= MARGIN
                bad_depth[v, t, ys[close], xs[close]] = True
        if not bad_hue.any() and not bad_depth.any():
            break
        fresh = _draw_greater(rng, clusters, cfg)
        flat_u8[bad_hue], depth_u16[bad_depth] = fresh[1][bad_hue], fresh[2][bad_depth]
    else:
        raise RuntimeError('the margin condition could not be met')
    inputs = dict(rgb_u8=rgb_u8, flat_u8=flat_u8, depth_u16=depth_u16, cam_RT=cam_RT, cam_K=cam_K,
                  hue_clusters=np.asarray(clusters, dtype=np.float32), other_bounds=np.float64(ob), min_z=np.float64(cfg['min_z']))
    files = {'frontend_greater_inputs': inputs}
    for name, kw, seed in GREATER_CASES:
        np.random.seed(seed)
        torch.manual_seed(seed)
        out = dict(seed=np.int64(seed))
        all_pcl, ratios = [], []
        for v in range(V):
            view = []
            for t in range(T):
                full = _greater_frame(ref, clusters, rgb[v, t], flat[v, t], depth[v, t], cam_RT[v, t], cam_K[v, t])
                kept = g.filter_pcl_bounds_numpy(_with_index(full), greater_floor_fix=True, **box)
                assert (_bound_margin(full[:, :3], bounds, True) > MARGIN).all()
                ratios.append(kept.shape[0] / max(full.shape[0], 1))
                sub = kept
                if kw['n_points_rnd'] > 0:
                    sub = g.subsample_pad_pcl_numpy(kept, kw['n_points_rnd'], subsample_only=False)
                if name == 'a':
                    out['unprojected_v%d_t%d' % (v, t)] = full
                    out['kept_v%d_t%d' % (v, t)] = kept[:, -1].astype(np.int32)
                    out['subsampled_v%d_t%d' % (v, t)] = sub[:, -1].astype(np.int32)
                view.append(np.ascontiguousarray(sub[:, :-1]))
            all_pcl.append(view)
        out['cuboid_filter_ratios'] = np.array(ratios)
        tail = _tail(ref, r_utils, all_pcl, kw, kw['src_view'])
        stages = {k: tail.pop(k) for k in list(tail) if k == 'accumulated' or k.startswith('merged_')}
        out.update(tail)
        files['frontend_greater_' + name] = out
        if name == 'a':
            files['frontend_greater_a_merge'] = stages
    return files


def _rigid(rng, yaw, xyz):
    c, s = np.cos(yaw), np.sin(yaw)
    tilt = rng.normal(scale=0.02, size=2)
    rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    rx = np.array([[1, 0, 0], [0, np.cos(tilt[0]), -np.sin(tilt[0])], [0, np.sin(tilt[0]), np.cos(tilt[0])]])
    ry = np.array([[np.cos(tilt[1]), 0, np.sin(tilt[1])], [0, 1, 0], [-np.sin(tilt[1]), 0, np.cos(tilt[1])]])
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = rz @ ry @ rx, xyz
    return m.astype(np.float32)


def _draw_lidar(rng, n):
    xyz = rng.uniform([-25.0, -32.0, -3.5], [62.0, 32.0, 13.0], size=(n, 3))
    cols = [xyz, rng.uniform(-1, 1, size=(n, 1)), rng.integers(0, 30, size=(n, 1)), rng.integers(0, 13, size=(n, 1)),
            rng.integers(0, 256, size=(n, 3)) / 255.0]
    return np.concatenate(cols, axis=1).astype(np.float32)


def _carla_frame(ref, lidar, sensor_RT, v, t, ref_t, ground):
    """One sweep up to the cuboid filter (data/data_carla.py:443-463)."""
    out = lidar
    if t != ref_t or v != 0:
        out = ref.geometry.transform_lidar_frame(out, sensor_RT[t, v], sensor_RT[ref_t, 0].astype(np.float32))
    if ground:
        out = out.copy()
        out[..., 2] += 1.0
    return out


def generate_carla(ref, r_utils, cfg=CARLA):
    g = ref.geometry
    rng = np.random.default_rng(cfg['seed'])
    V, T, N = cfg['V'], cfg['T'], cfg['N']
    sensor_RT = np.stack([np.stack([_rigid(rng, 0.3 + 0.04 * t + 1.1 * v, [40.0 + 3.0 * t + 2.0 * v, -12.0 + 0.5 * t - 6.0 * v,
                                                                           1.0 + 0.1 * v]) for v in range(V)]) for t in range(T)])
    sizes = [[N - 37 * t - 11 * v for t in range(T)] for v in range(V)]
    lidar = [[_draw_lidar(rng, sizes[v][t]) for t in range(T)] for v in range(V)]
    ob, mz = cfg['other_bounds'], cfg['min_z']
    scale = {1: (0.5, 2.0, 1.0, 0.5), 2: (0.6, 2.4, 0.8, 0.6), 3: (0.7, 2.2, 1.0, 0.5), 4: (0.7, 2.5, 1.0, 0.5)}
    out_scale = {1: (2.0, 1.0, 0.5), 2: (2.4, 0.8, 0.4), 3: (2.2, 1.0, 0.4), 4: (2.5, 1.0, 0.4)}
    tb = cfg['target_bounds']

    def all_bounds(mode):
        a, b, c, d = scale[mode]
        sx, sy, sz = out_scale[mode]
        return [((-ob * a, ob * b), (-ob * c, ob * c), (mz, ob * d)),
                ((-2.0, tb * sx + 2.0), (-tb * sy - 2.0, tb * sy + 2.0), (mz, tb * sz))]
    for attempt in range(100):
        bad = [[np.zeros(sizes[v][t], dtype=bool) for t in range(T)] for v in range(V)]
        for ref_frame in (None, -1):
            for ground in (True, False):
                for v in range(V):
                    for t in range(T):
                        ref_t = t if ref_frame is None else range(T)[ref_frame]
                        moved = _carla_frame(ref, lidar[v][t], sensor_RT, v, t, ref_t, ground)
                        for mode in (1, 2, 3, 4):
                            for b in all_bounds(mode):
                                bad[v][t] |= _bound_margin(moved[:, :3], b, False) <= MARGIN
        if not any(b.any() for view in bad for b in view):
            break
        for v in range(V):
            for t in range(T):
                lidar[v][t][bad[v][t]] = _draw_lidar(rng, int(bad[v][t].sum()))
    else:
        raise RuntimeError('the margin condition could not be met')
    inputs = dict(sensor_RT=sensor_RT, min_z=np.float64(mz), other_bounds=np.float64(ob), target_bounds=np.float64(tb))
    for v in range(V):
        for t in range(T):
            inputs['lidar_v%d_t%d' % (v, t)] = lidar[v][t]
    files = {'frontend_carla_inputs': inputs}
    stages = {}
    for mode, ref_frame in CARLA_STAGE_CASES:
        tag = 'm%d_%s' % (mode, 'own' if ref_frame is None else 'last')
        for v in range(V):
            for t in range(T):
                ref_t = t if ref_frame is None else range(T)[ref_frame]
                moved = _carla_frame(ref, lidar[v][t], sensor_RT, v, t, ref_t, True)
                if mode == 1:
                    stages['xyz_%s_v%d_t%d' % (tag[3:], v, t)] = moved[:, :3].copy()
                kept = g.filter_pcl_bounds_carla_input_numpy(_with_index(moved), min_z=mz, other_bounds=ob, cube_mode=mode)
                stages['kept_%s_v%d_t%d' % (tag, v, t)] = kept[:, -1].astype(np.int16)
    files['frontend_carla_stages'] = stages
    for name, kw, seed in CARLA_CASES:
        np.random.seed(seed)
        torch.manual_seed(seed)
        out = dict(seed=np.int64(seed))
        all_lidar, ratios = [], []
        for v in range(V):
            view = []
            for t in range(T):
                ref_t = t if kw['reference_frame'] is None else range(T)[kw['reference_frame']]
                moved = _carla_frame(ref, lidar[v][t], sensor_RT, v, t, ref_t, kw['correct_origin_ground'])
                kept = g.filter_pcl_bounds_carla_input_numpy(moved, min_z=mz, other_bounds=ob, cube_mode=kw['cube_mode'])
                ratios.append(kept.shape[0] / max(moved.shape[0], 1))
                if kw['n_points_rnd'] > 0:
                    kept = g.subsample_pad_pcl_numpy(kept, kw['n_points_rnd'], subsample_only=False)
                view.append(kept.astype(np.float32))
            all_lidar.append(view)
        out['cuboid_filter_ratios'] = np.array(ratios)
        flt = lambda f, m=kw['cube_mode']: g.filter_pcl_bounds_carla_output_torch(f, min_z=mz, other_bounds=tb, padding=2.0, cube_mode=m)
        tail = _tail(ref, r_utils, all_lidar, kw, 0, target_filter=flt, retain=kw['oversample_vehped_target'])
        for k in list(tail):
            if k == 'accumulated' or k.startswith('merged_'):
                tail.pop(k)
        out.update(tail)
        files['frontend_carla_' + name] = out
    return files


def write(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    ref, r_utils, clusters = load_reference()
    files = dict(generate_greater(ref, r_utils, clusters))
    files.update(generate_carla(ref, r_utils))
    paths = []
    for name, arrays in files.items():
        path = os.path.join(out_dir, name + '.npz')
        np.savez_compressed(path, **arrays)
        paths.append((path, os.path.getsize(path)))
    return paths


if __name__ == '__main__':
    for path, size in write(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'golden')):
        print('%8d  %s' % (size, path))
