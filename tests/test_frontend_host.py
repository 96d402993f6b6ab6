"""The clip front end (occlusions4d_amd.frontend, include/occ4d_frontend.h) through the g++ twin, without a GPU: every stage
and the final clouds equal the reference's own results (tests/golden/frontend_*.npz, written by tests/gen_frontend_fixture.py)
bit for bit -- values, row order, sizes, ratios and the state of numpy's and torch's global generators afterwards.  The twin
and the HIP kernels share the per-element source (csrc/frontend_math.hpp); tests/test_gpu_frontend.py runs the same
comparisons on the device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import frontend_cases as fc
import gen_frontend_fixture as gen
import occlusions4d_amd as pk

CPU = torch.device('cpu')


@pytest.fixture
def twin():
    pk.cpu_twin.enable()
    try:
        yield pk
    finally:
        pk.cpu_twin.disable()


def test_signature_tables_match_their_headers():
    """occ4d.h keeps its symbol set and version; the front end is bound from the second header through the same parser."""
    lib = pk._lib
    with open(lib.HEADER_PATH) as f:
        text = f.read()
    structs = {'occ4d_linear_args': lib.LinearArgs, 'occ4d_pt_layer_weights': lib.PtLayerWeights,
               'occ4d_launch_events': lib.LaunchEvents, 'occ4d_decoder_weights': lib.DecoderWeights}
    assert lib.SIGNATURES == lib.parse_prototypes(text, structs)
    assert 'frontend' not in text and not any(n in lib.SIGNATURES for n in lib.FRONTEND_SIGNATURES)
    assert lib.parse_constants(text)['ABI_VERSION'] == lib.ABI_VERSION
    with open(lib.FRONTEND_HEADER_PATH) as f:
        front = f.read()
    assert lib.FRONTEND_SIGNATURES == lib.parse_prototypes(front, {})
    assert sorted(lib.FRONTEND_SIGNATURES) == ['occ4d_lidar_rows_f32', 'occ4d_rgbd_rows_f32']
    assert lib.parse_constants(front) == {}                      # (no version of its own: it travels with libocc4d.so)
    res, args = lib.FRONTEND_SIGNATURES['occ4d_lidar_rows_f32']
    assert res is ctypes.c_int and args[8] is ctypes.c_double and args[1] is ctypes.c_int64
    assert len(lib.FRONTEND_SIGNATURES['occ4d_rgbd_rows_f32'][1]) == 22


def test_hip_library_exports_the_frontend_symbols():
    if not os.path.exists(pk._lib.LIB_PATH):
        pytest.skip('libocc4d.so not built')
    handle = ctypes.CDLL(pk._lib.LIB_PATH)
    for name in pk._lib.FRONTEND_SIGNATURES:
        assert hasattr(handle, name), name


def test_twin_binds_the_frontend_prototypes(twin):
    lib = pk._lib.lib()
    for name, (res, args) in pk._lib.FRONTEND_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


@pytest.mark.parametrize('n', [1, 2, 7, 1000, 5003])
def test_shuffling_arange_consumes_the_generator_as_shuffling_the_rows_does(n):
    np.random.seed(5 + n)
    rows = np.arange(n * 8, dtype=np.float32).reshape(n, 8)
    want = rows.copy()
    np.random.shuffle(want)
    after_rows = np.random.get_state()
    np.random.seed(5 + n)
    perm = np.arange(n)
    np.random.shuffle(perm)
    after_perm = np.random.get_state()
    assert np.array_equal(rows[perm], want)
    assert np.array_equal(after_rows[1], after_perm[1]) and after_rows[2:] == after_perm[2:]


def test_greater_every_stage_bit_for_bit(twin):
    fc.check_greater_stages(CPU)


@pytest.mark.parametrize('name', [c[0] for c in gen.GREATER_CASES])
def test_greater_clip_bit_for_bit(twin, name):
    got, g, _ = fc.run_greater(name, CPU)
    fc.check_tail(got, g, 'greater ' + name)
    assert got[0].shape[1] == 8 and got[1].shape[1] == 1 and all(f.shape[1] == 9 for f in got[2])


@pytest.mark.parametrize('mode,ref_frame', gen.CARLA_STAGE_CASES)
def test_carla_transform_and_filter_bit_for_bit(twin, mode, ref_frame):
    fc.check_carla_stages(CPU, mode, ref_frame)


@pytest.mark.parametrize('name', [c[0] for c in gen.CARLA_CASES])
def test_carla_clip_bit_for_bit(twin, name):
    got, g = fc.run_carla(name, CPU)
    fc.check_tail(got, g, 'carla ' + name)
    assert got[0].shape[1] == 8 and got[1].shape[1] == 3 and all(f.shape[1] == 11 for f in got[2])


def test_fixtures_hold_the_margin_condition():
    """What the generator asserted, re-checked on the committed files: memberships and ids do not hang on the last bit."""
    inp = fc.greater_inputs()
    assert gen._hue_ok(inp['flat'], inp['hue_clusters']).all()
    g = fc.load_golden('frontend_greater_a')
    ob, mz = inp['other_bounds'], inp['min_z']
    for k in g:
        if k.startswith('unprojected_'):
            assert (gen._bound_margin(g[k][:, :3], ((-ob, ob), (-ob, ob), (mz, ob)), True) > gen.MARGIN).all(), k


def test_geometry_mirrors(twin):
    """point_cloud_from_rgbd / transform_lidar_frame / filter_pcl_bounds_carla_input_torch / greater_floor_fix: the reference's
    names and arguments on single frames."""
    inp, g = fc.greater_inputs(), fc.load_golden('frontend_greater_a')
    geo = pk.geometry
    pcl = geo.point_cloud_from_rgbd(torch.from_numpy(inp['rgb'][1, 2]), torch.from_numpy(inp['depth'][1, 2]), inp['cam_RT'][1, 2],
                                    inp['cam_K'][1, 2])
    ref = g['unprojected_v1_t2']
    fc.same(pcl, np.ascontiguousarray(ref[:, [0, 1, 2, 4, 5, 6]]), 'point_cloud_from_rgbd')
    ob = inp['other_bounds']
    kept = geo.filter_pcl_bounds_torch(torch.from_numpy(ref), x_min=-ob, x_max=ob, y_min=-ob, y_max=ob, z_min=inp['min_z'], z_max=ob,
                                       greater_floor_fix=True)
    fc.same(kept, ref[g['kept_v1_t2']], 'filter_pcl_bounds_torch(greater_floor_fix=True)')
    lidar, cin = fc.carla_inputs()
    st = fc.load_golden('frontend_carla_stages')
    moved = geo.transform_lidar_frame(torch.from_numpy(lidar[1][0]), cin['sensor_RT'][0, 1], cin['sensor_RT'][2, 0])
    want = st['xyz_last_v1_t0']                   # (the fixture's z carries the +1 m ground offset)
    assert np.array_equal(moved.numpy()[:, :2], want[:, :2]) and np.array_equal(moved.numpy()[:, 2] + np.float32(1.0), want[:, 2])
    shifted = moved.clone()
    shifted[:, 2] += 1.0
    kept = geo.filter_pcl_bounds_carla_input_torch(shifted, min_z=float(cin['min_z']), other_bounds=float(cin['other_bounds']),
                                                   cube_mode=3)
    fc.same(kept, shifted.numpy()[st['kept_m3_last_v1_t0'].astype(np.int64)], 'filter_pcl_bounds_carla_input_torch')
    assert geo.filter_pcl_bounds_carla_input_torch(shifted, cube_mode=7) is shifted


def test_error_conventions(twin):
    fc.check_argument_errors(CPU)


def test_cpu_tensors_are_rejected_without_the_twin():
    assert not pk.cpu_twin.enabled()
    if not os.path.exists(pk._lib.LIB_PATH):
        pytest.skip('libocc4d.so not built')
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        pk.frontend.lidar_rows(torch.zeros(5, 4))
