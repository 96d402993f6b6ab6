"""Shared by tests/test_frontend_host.py (g++ twin) and tests/test_gpu_frontend.py (HIP): the fixtures of
tests/gen_frontend_fixture.py (the reference's own results, stage by stage) against occlusions4d_amd.frontend on one device.
Everything is compared BIT FOR BIT: values, row order, sizes, ratios and the state of both global generators afterwards."""
import numpy as np
import pytest
import torch

import gen_frontend_fixture as gen
import occlusions4d_amd as pk
from conftest import load_golden


def same(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, '%s: shape %s, the reference has %s' % (what, got.shape, want.shape)
    assert got.dtype == want.dtype, '%s: dtype %s, the reference has %s' % (what, got.dtype, want.dtype)
    assert np.array_equal(got.view(np.uint32) if got.dtype == np.float32 else got,
                          want.view(np.uint32) if want.dtype == np.float32 else want), \
        '%s differs from the reference in %d elements' % (what, int((got != want).sum()))


def seed(n):
    np.random.seed(int(n))
    torch.manual_seed(int(n))


def check_tail(got, g, what):
    """(pcl_input, pcl_input_sem, pcl_target, meta) of a clip function against a fixture's final arrays and generator states."""
    pcl_input, sem, targets, meta = got
    same(pcl_input, g['pcl_input'], what + ' pcl_input')
    same(sem, g['pcl_input_sem'], what + ' pcl_input_sem')
    n_target = len([k for k in g if k.startswith('pcl_target_') and k != 'pcl_target_size'])
    assert len(targets) == n_target
    for i, frame in enumerate(targets):
        same(frame, g['pcl_target_%d' % i], what + ' pcl_target[%d]' % i)
    assert np.array_equal(meta['pcl_sizes'], g['pcl_sizes'])
    assert meta['cuboid_filter_ratios'] == g['cuboid_filter_ratios'].tolist()
    assert meta['sample_input_ratios'] == g['sample_input_ratios'].tolist()
    assert meta['sample_target_ratios'] == g['sample_target_ratios'].tolist()
    assert meta['pcl_input_size'] == int(g['pcl_input_size']) and meta['pcl_target_size'] == g['pcl_target_size'].tolist()
    state = np.random.get_state()
    assert np.array_equal(state[1], g['np_state']) and state[2] == int(g['np_pos']), what + ': numpy generator state'
    assert np.array_equal(torch.get_rng_state().numpy(), g['torch_state']), what + ': torch generator state'


# --------------------------------------------------------------------------------------------------------------- GREATER
def greater_inputs():
    g = load_golden('frontend_greater_inputs')
    rgb, flat, depth = gen.images_from_integers(g['rgb_u8'], g['flat_u8'], g['depth_u16'])
    return dict(rgb=rgb, flat=flat, depth=depth, cam_RT=g['cam_RT'], cam_K=g['cam_K'], hue_clusters=g['hue_clusters'],
                other_bounds=float(g['other_bounds']), min_z=float(g['min_z']))


def run_greater(name, device, stages=None):
    kw = dict(gen.GREATER_CASES_BY_NAME[name])
    g = load_golden('frontend_greater_' + name)
    seed(g['seed'])
    if stages is None:
        got = pk.frontend.greater_clip(device=device, **greater_inputs(), **kw)
    else:                                           # (the private entry that also hands out its intermediate clouds)
        got = pk.frontend._greater_clip(device=device, stages=stages, **greater_inputs(), **kw)
    return got, g, kw


def check_greater_stages(device):
    """Case 'a': rows after unprojection, after the filter, after the per-frame subsampling, after time accumulation and
    after the view merge."""
    stages = {}
    got, g, kw = run_greater('a', device, stages)
    inp = greater_inputs()
    V, T, H, W = inp['depth'].shape
    merge = load_golden('frontend_greater_a_merge')
    for v in range(V):
        rows = stages[('rows', v)].cpu().numpy().reshape(T, H * W, 8)
        key = stages[('key', v)].cpu().numpy().reshape(T, H * W)
        for t in range(T):
            valid = np.flatnonzero(inp['depth'][v, t].reshape(-1) > 0)          # (np.where's order: row-major)
            ref = g['unprojected_v%d_t%d' % (v, t)]
            same(rows[t][valid][:, :7], ref, 'unprojected rows v%d t%d' % (v, t))
            assert (rows[t][:, 7] == t).all()
            assert np.array_equal(np.flatnonzero(key[t][valid] > 0.5), g['kept_v%d_t%d' % (v, t)]), 'filter v%d t%d' % (v, t)
            assert not key[t][np.setdiff1d(np.arange(H * W), valid)].any()
            sub = g['subsampled_v%d_t%d' % (v, t)]
            frame = np.concatenate([ref[sub], np.full((len(sub), 1), t, dtype=np.float32)], axis=1)
            if v == kw['src_view'] and t < kw['pcl_input_frames']:
                same(stages[('frame', v, t)], frame, 'subsampled frame v%d t%d' % (v, t))
    same(torch.cat([stages[('frame', kw['src_view'], t)] for t in range(kw['pcl_input_frames'])]),
         merge['accumulated'][:sum(g['pcl_sizes'][kw['src_view']][:kw['pcl_input_frames']])], 'accumulated input')
    for i in range(kw['pcl_target_frames']):
        t = T - kw['pcl_target_frames'] + i
        same(torch.cat([stages[('frame_target', v, t)] for v in range(V)]), merge['merged_%d' % i], 'merged frame %d' % t)
    check_tail(got, g, 'greater a')


# --------------------------------------------------------------------------------------------------------------- CARLA
def carla_inputs():
    g = load_golden('frontend_carla_inputs')
    T, V = g['sensor_RT'].shape[:2]
    lidar = [[g['lidar_v%d_t%d' % (v, t)] for t in range(T)] for v in range(V)]
    return lidar, g


def run_carla(name, device):
    kw = dict(gen.CARLA_CASES_BY_NAME[name])
    g = load_golden('frontend_carla_' + name)
    lidar, inp = carla_inputs()
    seed(g['seed'])
    got = pk.frontend.carla_clip(lidar, inp['sensor_RT'], min_z=float(inp['min_z']), other_bounds=float(inp['other_bounds']),
                                 target_bounds=float(inp['target_bounds']), device=device, **kw)
    return got, g


def check_carla_stages(device, mode, ref_frame):
    """Transformed coordinates and filter membership of every sweep for one cube mode / reference frame setting."""
    lidar, inp = carla_inputs()
    st = load_golden('frontend_carla_stages')
    T, V = inp['sensor_RT'].shape[:2]
    which = 'own' if ref_frame is None else 'last'
    for v in range(V):
        for t in range(T):
            ref_t = t if ref_frame is None else range(T)[ref_frame]
            src = inv = None
            if t != ref_t or v != 0:
                src, inv = inp['sensor_RT'][t, v], np.linalg.inv(inp['sensor_RT'][ref_t, 0])
            rows, key = pk.frontend.lidar_rows(torch.from_numpy(lidar[v][t]).to(device), src, inv, 1.0, mode, float(inp['min_z']),
                                               float(inp['other_bounds']))
            rows, key = rows.cpu().numpy(), key.cpu().numpy()
            same(rows[:, :3], st['xyz_%s_v%d_t%d' % (which, v, t)], 'lidar xyz %s v%d t%d' % (which, v, t))
            same(rows[:, 3:], lidar[v][t][:, 3:], 'lidar attributes')
            assert np.array_equal(np.flatnonzero(key > 0.5), st['kept_m%d_%s_v%d_t%d' % (mode, which, v, t)].astype(np.int64))


def check_argument_errors(device):
    """Shape violations raise AssertionError, as elsewhere in the package; the library's own checks (EINVAL) are those of
    csrc/frontend_math.hpp, one source for both libraries."""
    inp = greater_inputs()
    kw = dict(gen.GREATER_CASES_BY_NAME['a'], device=device)
    with pytest.raises(AssertionError, match='cam_K'):
        pk.frontend.greater_clip(**dict(inp, cam_K=inp['cam_K'][:, :2]), **kw)
    with pytest.raises(AssertionError, match='rgb'):
        pk.frontend.greater_clip(**dict(inp, rgb=inp['rgb'][..., :2]), **kw)
    with pytest.raises(AssertionError, match='depth'):
        pk.frontend.greater_clip(**dict(inp, depth=inp['depth'][0]), **kw)
    with pytest.raises(AssertionError):
        pk.frontend.greater_clip(**inp, **dict(kw, src_view=5))
    with pytest.raises(AssertionError, match='n_clusters'):                    # the library's own check (EINVAL)
        pk.frontend.greater_clip(**dict(inp, hue_clusters=np.arange(65, dtype=np.float32)), **kw)
    lidar, cin = carla_inputs()
    with pytest.raises(AssertionError, match='sensor_RT'):
        pk.frontend.carla_clip(lidar, cin['sensor_RT'][:2], device=device)
    with pytest.raises(AssertionError, match='x, y, z'):
        pk.frontend.lidar_rows(torch.zeros(5, 2, device=device))
    with pytest.raises(AssertionError, match='cube_mode'):
        pk.frontend.lidar_rows(torch.zeros(5, 4, device=device), cube_mode=9)
    lib = pk._lib.lib()
    rows, out, key = (torch.zeros(shape, device=device) for shape in ((4, 4), (4, 4), (4,)))
    source = torch.eye(4)                                                      # (a HOST matrix in both libraries)
    rc = lib.occ4d_lidar_rows_f32(rows.data_ptr(), 4, 4, 4, source.data_ptr(), None, 0.0, 0, 0.0, 1.0, out.data_ptr(), 4, key.data_ptr(),
                                  None)
    assert rc == pk._lib.EINVAL and b'go together' in lib.occ4d_last_error()
