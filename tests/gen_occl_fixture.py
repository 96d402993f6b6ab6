"""Writes tests/golden/occl_*.npz: the REFERENCE's own data_utils.get_valo_ids (data/data_utils.py:12-100) and a replay of its
track choice (data/data_greater.py:534-552, the reference's lines with the reference's arguments) on the clouds of the synthetic
clips of tests/gen_frontend_fixture.py (frontend_greater_inputs.npz, frontend_carla_inputs.npz).  Container-only, like that
generator, whose way of loading the reference's modules it follows.

    python tests/gen_occl_fixture.py [OUT_DIR]

Every case runs the reference's loader steps under one seed (the loops of gen_frontend_fixture, unchanged), then get_valo_ids,
then the track choice, in the reference's order.  A file holds the small integers the test rebuilds the function's inputs from
(the instance id / semantic tag / time columns of the clouds: get_valo_ids reads nothing else) and the recorded outputs.

PARITY UNPINNED at one call: torchvision is not installed and oracle.ref_import stubs it empty, so get_valo_ids'
torchvision.transforms.ToTensor() is a stand-in here that maps a float32 (N, D) array to a (1, N, D) tensor unscaled -- which
is torchvision's documented behaviour for float input.

The synthetic CARLA sweeps spread 30 instance ids evenly over 13 tags: no vehicle / pedestrian id reaches the minimum count.
The CARLA cases therefore run on a variant of the clip whose instance ids are taken modulo CARLA_ID_MOD (stored in the file);
the generator asserts that a CARLA case has num_valo_ids >= 2, that a case has an id below the minimum count, and that one has
num_valo_ids == 0.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_frontend_fixture as gen  # noqa: E402

CARLA_ID_MOD = 3
MAX_VALO_GREATER, MAX_VALO_CARLA = 32, 256             # _MAX_VALO_IDS of data/data_greater.py:25, data/data_carla.py:22
# (name, keyword arguments of the clip function, live_occl_mode, track_mode, seed)
GREATER_CASES = [
    ('greater_unfilt', dict(n_points_rnd=400, n_fps_input=1024, n_fps_target=512, pcl_input_frames=3, pcl_target_frames=2, src_view=0),
     'unfilt', 'random', 91),
    ('greater_normal', dict(n_points_rnd=1200, n_fps_input=768, n_fps_target=-400, pcl_input_frames=2, pcl_target_frames=1, src_view=1),
     'normal', 'snitch', 92),
    ('greater_few', dict(n_points_rnd=500, n_fps_input=170, n_fps_target=0, pcl_input_frames=2, pcl_target_frames=1, src_view=0),
     'normal', 'random', 93),                       # (about 8 input points per id: some ids reach the minimum, some do not)
    ('greater_none', dict(n_points_rnd=300, n_fps_input=48, n_fps_target=256, pcl_input_frames=1, pcl_target_frames=1, src_view=1),
     'normal', 'random', 94),                       # (no id reaches 8 points: num_valo_ids = 0, and 'random' draws nothing)
]
CARLA_CASES = [
    ('carla_unfilt', dict(cube_mode=4, reference_frame=-1, n_points_rnd=300, n_fps_input=384, n_fps_target=384, pcl_input_frames=3,
                          pcl_target_frames=2, correct_origin_ground=True, oversample_vehped_target=False), 'unfilt', 95),
    ('carla_normal', dict(cube_mode=1, reference_frame=None, n_points_rnd=0, n_fps_input=384, n_fps_target=-300, pcl_input_frames=2,
                          pcl_target_frames=1, correct_origin_ground=True, oversample_vehped_target=True), 'normal', 96),
]
GREATER_BY_NAME = {c[0]: c for c in GREATER_CASES}
CARLA_BY_NAME = {c[0]: c for c in CARLA_CASES}


def carla_variant(lidar):
    """The CARLA clip the cases run on: instance ids modulo CARLA_ID_MOD (copies)."""
    out = [[sweep.copy() for sweep in view] for view in lidar]
    for view in out:
        for sweep in view:
            sweep[:, 4] = np.mod(sweep[:, 4], np.float32(CARLA_ID_MOD))
    return out


def load_data_utils():
    """(reference namespace, its utils module, the hue clusters, its data/data_utils.py module with the ToTensor stand-in)."""
    ref, r_utils, clusters = gen.load_reference()
    from oracle import ref_import
    tv, tr = sys.modules['torchvision'], sys.modules['torchvision.transforms']
    tv.transforms = tr

    class ToTensor:                                    # the stand-in: float32 (N, D) -> (1, N, D), unscaled
        def __call__(self, a):
            assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 2
            return torch.from_numpy(a)[None]
    tr.ToTensor = ToTensor
    root = ref_import.REFERENCE_ROOT
    added = [root] + [os.path.join(root, d) for d in ('data', 'eval', 'model', 'utils')]
    names = ('__init__', 'utils', 'data_utils')
    saved = {k: sys.modules.pop(k) for k in names if k in sys.modules}
    cwd = os.getcwd()
    os.chdir(root)
    sys.path[:0] = added
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            import data_utils as r_data_utils
    finally:
        os.chdir(cwd)
        for p in added:
            sys.path.remove(p)
        for k in names:
            sys.modules.pop(k, None)
        sys.modules.update(saved)
    return ref, r_utils, clusters, r_data_utils


def _columns(frame, cols):
    """The integer-valued columns `cols` of a cloud as int16 (asserted exact)."""
    a = np.asarray(frame)[:, cols]
    out = a.astype(np.int16)
    assert np.array_equal(out.astype(np.float32), a.astype(np.float32))
    return out


def _record(out, mode, all_pcl_used, sem, pcl_input, merged, cols, sem_cols, result):
    live_occl, valo_ids_pad, num_valo_ids, mask = result
    out['live_occl_mode'] = np.array(mode)
    for v, view in enumerate(all_pcl_used):
        for t, frame in enumerate(view):
            out['cloud_v%d_t%d' % (v, t)] = _columns(frame, cols)                 # (instance id[, semantic tag]) of all_pcl[v][t]
    out['input_sem'] = _columns(sem.numpy(), sem_cols)                            # the same columns of pcl_input_sem
    out['input_t'] = _columns(pcl_input.numpy(), [6])[:, 0].astype(np.int8)       # (x, y, z, R, G, B, t)
    for t, frame in enumerate(merged):
        out['merged_%d' % t] = _columns(frame, cols[:1])[:, 0]
    out['live_occl'], out['valo_ids'], out['num_valo_ids'] = live_occl, valo_ids_pad, np.int64(num_valo_ids)
    assert live_occl.dtype == np.float64 and valo_ids_pad.dtype == np.int32
    if mask is not None:
        out['vehped_mask'] = mask.numpy()


def _track_choice(track_mode, pcl_input, sem, targets):
    """The track choice of data/data_greater.py:534-560 replayed with the reference's arguments: candidates are the unique
    int32 ids of the first input frame with at least 16 equal rows, 'snitch' takes 0, 'random' one np.random.choice of the
    candidate list -> (track_id, input mark (n, 1), target marks)."""
    first = sem[pcl_input[:, -1] == 0][:, 0]
    ids = [i for i in first.to(torch.int32).unique().numpy() if i >= 0 and int((first == i).sum()) >= 16]
    track_id = -1
    mark_in = torch.zeros_like(pcl_input[:, :1])
    mark_tg = [torch.zeros_like(f[:, :1]) for f in targets]
    if track_mode != 'none' and ids:
        track_id = {'snitch': lambda: 0, 'random': lambda: np.random.choice(ids)}[track_mode]()
        mark_in[(sem[:, 0] == track_id) & (pcl_input[:, -1] == 0)] = 1.0
        for f, m in zip(targets, mark_tg):
            m[f[:, 3] == track_id] = 1.0
    return int(track_id), mark_in, mark_tg


def generate_greater(ref, r_utils, clusters, r_data_utils):
    g = ref.geometry
    inp = np.load(os.path.join(HERE, 'golden', 'frontend_greater_inputs.npz'))
    rgb, flat, depth = gen.images_from_integers(inp['rgb_u8'], inp['flat_u8'], inp['depth_u16'])
    cam_RT, cam_K = inp['cam_RT'], inp['cam_K']
    ob, mz = float(inp['other_bounds']), float(inp['min_z'])
    V, T = depth.shape[:2]
    files = {}
    for name, kw, mode, track_mode, seed in GREATER_CASES:
        np.random.seed(seed)
        torch.manual_seed(seed)
        all_pcl, all_pcl_nss = [], []
        for v in range(V):
            view, view_nss = [], []
            for t in range(T):
                full = gen._greater_frame(ref, clusters, rgb[v, t], flat[v, t], depth[v, t], cam_RT[v, t], cam_K[v, t])
                kept = g.filter_pcl_bounds_numpy(full, x_min=-ob, x_max=ob, y_min=-ob, y_max=ob, z_min=mz, z_max=ob,
                                                 greater_floor_fix=True)
                view_nss.append(kept)
                sub = kept
                if kw['n_points_rnd'] > 0:
                    sub = g.subsample_pad_pcl_numpy(kept, kw['n_points_rnd'], subsample_only=False)
                view.append(np.ascontiguousarray(sub))
            all_pcl.append(view)
            all_pcl_nss.append(view_nss)
        merged = r_utils.merge_pcl_views_numpy(all_pcl, insert_view_idx=True)
        tail = gen._tail(ref, r_utils, all_pcl, kw, kw['src_view'])
        sem = torch.from_numpy(tail['pcl_input_sem'])
        pcl_input = torch.from_numpy(tail['pcl_input'][:, :7])
        targets = [torch.from_numpy(tail['pcl_target_%d' % i][:, :8]) for i in range(kw['pcl_target_frames'])]
        used = all_pcl_nss if 'unfilt' in mode else all_pcl                        # data/data_greater.py:520
        result = r_data_utils.get_valo_ids(mode, 0, None, False, 0, None, 3, kw['pcl_input_frames'], T, 0, 0, 1, 0, kw['src_view'], V,
                                           MAX_VALO_GREATER, None, used, sem, merged)
        out = dict(seed=np.int64(seed), track_mode=np.array(track_mode))
        _record(out, mode, used, sem, pcl_input, merged, [3], [0], result)
        state = np.random.get_state()
        out['np_state_before'], out['np_pos_before'] = state[1].copy(), np.int64(state[2])
        track_id, mark_in, mark_tg = _track_choice(track_mode, pcl_input, sem, targets)
        state = np.random.get_state()
        out['np_state'], out['np_pos'] = state[1].copy(), np.int64(state[2])
        out['torch_state'] = torch.get_rng_state().numpy().copy()
        out['track_id'] = np.int64(track_id)
        out['input_mark'] = mark_in.numpy()[:, 0].astype(np.uint8)
        for i, m in enumerate(mark_tg):
            out['target_mark_%d' % i] = m.numpy()[:, 0].astype(np.uint8)
        files['occl_' + name] = out
    return files


def generate_carla(ref, r_utils, r_data_utils):
    g = ref.geometry
    inp = np.load(os.path.join(HERE, 'golden', 'frontend_carla_inputs.npz'))
    sensor_RT = inp['sensor_RT']
    T, V = sensor_RT.shape[:2]
    lidar = carla_variant([[inp['lidar_v%d_t%d' % (v, t)] for t in range(T)] for v in range(V)])
    mz, ob, tb = float(inp['min_z']), float(inp['other_bounds']), float(inp['target_bounds'])
    files = {}
    for name, kw, mode, seed in CARLA_CASES:
        np.random.seed(seed)
        torch.manual_seed(seed)
        all_lidar, all_lidar_nss = [], []
        for v in range(V):
            view, view_nss = [], []
            for t in range(T):
                ref_t = t if kw['reference_frame'] is None else range(T)[kw['reference_frame']]
                moved = gen._carla_frame(ref, lidar[v][t], sensor_RT, v, t, ref_t, kw['correct_origin_ground'])
                kept = g.filter_pcl_bounds_carla_input_numpy(moved, min_z=mz, other_bounds=ob, cube_mode=kw['cube_mode'])
                view_nss.append(kept)
                if kw['n_points_rnd'] > 0:
                    kept = g.subsample_pad_pcl_numpy(kept, kw['n_points_rnd'], subsample_only=False)
                view.append(kept.astype(np.float32))
            all_lidar.append(view)
            all_lidar_nss.append(view_nss)
        merged = r_utils.merge_pcl_views_numpy(all_lidar, insert_view_idx=True)
        flt = lambda f, m=kw['cube_mode']: g.filter_pcl_bounds_carla_output_torch(f, min_z=mz, other_bounds=tb, padding=2.0, cube_mode=m)
        tail = gen._tail(ref, r_utils, all_lidar, kw, 0, target_filter=flt, retain=kw['oversample_vehped_target'])
        sem = torch.from_numpy(tail['pcl_input_sem'])
        pcl_input = torch.from_numpy(tail['pcl_input'][:, :7])
        used = all_lidar_nss if 'unfilt' in mode else all_lidar                    # data/data_carla.py:607
        result = r_data_utils.get_valo_ids(mode, 0, None, True, 1, 2, 4, kw['pcl_input_frames'], T, 0, 0, 1, 0, 0, V, MAX_VALO_CARLA,
                                           None, used, sem, merged)
        out = dict(seed=np.int64(seed), id_mod=np.int64(CARLA_ID_MOD))
        _record(out, mode, used, sem, pcl_input, merged, [4, 5], [1, 2], result)
        state = np.random.get_state()
        out['np_state'], out['np_pos'] = state[1].copy(), np.int64(state[2])
        out['torch_state'] = torch.get_rng_state().numpy().copy()
        files['occl_' + name] = out
    return files


def write(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    ref, r_utils, clusters, r_data_utils = load_data_utils()
    files = dict(generate_greater(ref, r_utils, clusters, r_data_utils))
    files.update(generate_carla(ref, r_utils, r_data_utils))
    mins = {'unfilt': 16, 'normal': 8}
    assert any(f['num_valo_ids'] >= 2 for k, f in files.items() if k.startswith('occl_carla')), 'no CARLA case with two valo ids'
    assert any(f['num_valo_ids'] == 0 for f in files.values()), 'no case without valo ids'
    assert files['occl_greater_unfilt']['track_id'] >= 0 and files['occl_greater_unfilt']['np_pos'] != files['occl_greater_unfilt']['np_pos_before']
    below = False
    for f in files.values():                          # an id that is present among the input rows but below the minimum count
        sem = f['input_sem'] if 'normal' in str(f['live_occl_mode']) else None
        if sem is None:
            continue
        ids = sem[:, 0] if sem.shape[1] == 1 else sem[:, 0][(sem[:, 1] == 4) | (sem[:, 1] == 10)]
        n = np.bincount(ids[ids >= 0])
        below |= bool(((n > 0) & (n < mins['normal'])).any()) and f['num_valo_ids'] > 0
    assert below, 'no case with an id below the minimum count beside ids above it'
    paths = []
    for name, arrays in files.items():
        path = os.path.join(out_dir, name + '.npz')
        np.savez_compressed(path, **arrays)
        paths.append((path, os.path.getsize(path), int(arrays['num_valo_ids'])))
    return paths


if __name__ == '__main__':
    for path, size, num in write(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'golden')):
        print('%8d  %s  num_valo_ids = %d' % (size, path, num))
