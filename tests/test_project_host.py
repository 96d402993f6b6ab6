"""Clouds into camera views (include/occ4d_project.h, occlusions4d_amd.projection) through the g++ twin, without a GPU: the four
entry points against the reference's own pixel_coords_from_point_cloud (tests/golden/project_*.npz, written by
tests/gen_project_fixture.py), against the numpy restatement of the z-buffer and visibility decisions over the case matrix of
tests/project_cases.py, the round trip with the front end's unprojection, and evaluate_clip(stats_occlusion=...) against
evaluate_clip(stats_group_fn=...) -- everything EQUAL, no tolerance.  The twin and the HIP kernels share the per-element source
(csrc/project_math.hpp); tests/test_gpu_project.py runs the same comparisons on the device."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import gen_project_fixture as gen
import project_cases as pc
import occlusions4d_amd as pk

CPU = torch.device('cpu')
NAMES = ['occ4d_project_points_f32', 'occ4d_visibility_f32', 'occ4d_zbuffer_resolve_f32', 'occ4d_zbuffer_splat_f32']


@pytest.fixture
def twin():
    pk.cpu_twin.enable()
    try:
        yield pk
    finally:
        pk.cpu_twin.disable()


def test_signature_table_matches_the_header():
    lib = pk._lib
    with open(lib.PROJECT_HEADER_PATH) as f:
        text = f.read()
    assert lib.PROJECT_SIGNATURES == lib.parse_prototypes(text, {})
    assert sorted(lib.PROJECT_SIGNATURES) == NAMES
    for table in (lib.SIGNATURES, lib.FRONTEND_SIGNATURES, lib.EVAL_SIGNATURES, lib.OCCL_SIGNATURES, lib.TRACK_SIGNATURES):
        assert not any(n in table for n in lib.PROJECT_SIGNATURES)
    assert lib.parse_constants(text) == {}
    want = {NAMES[0]: 9, NAMES[1]: 13, NAMES[2]: 16, NAMES[3]: 11}
    for name, count in want.items():
        res, args = lib.PROJECT_SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == count and args[-1] is ctypes.c_void_p, name
    assert lib.PROJECT_SIGNATURES[NAMES[3]][1][9] is ctypes.c_void_p and lib.PROJECT_SIGNATURES[NAMES[1]][1][10] is ctypes.c_float


def test_hip_library_exports_the_symbols():
    if not os.path.exists(pk._lib.LIB_PATH):
        pytest.skip('libocc4d.so not built')
    handle = ctypes.CDLL(pk._lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(handle, name), name


def test_twin_binds_the_prototypes(twin):
    lib = pk._lib.lib()
    for name, (res, args) in pk._lib.PROJECT_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_module_interface():
    pj = pk.projection
    assert (pj.VISIBLE, pj.OCCLUDED, pj.OUTSIDE) == (0, 1, 2) and 'projection' in pk.__all__
    assert list(inspect.signature(pj.pixel_coords_from_point_cloud).parameters) == ['pcl', 'cam_RT', 'cam_K', 'flip_xy']
    assert list(inspect.signature(pj.render_views).parameters) == ['pcl', 'cam_RT', 'cam_K', 'height', 'width', 'channels', 'radius',
                                                                   'background']
    assert inspect.signature(pk.evaluation.evaluate_clip).parameters['stats_occlusion'].default is None


def test_fixture_generator_lists_the_committed_files():
    assert [c[2] for c in gen.CASES] == [2, 7, 1000, 2000, 257, 1025] and all(2 <= c[2] <= 2000 for c in gen.CASES)
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    for name, cam, N, D, H, W, margin, seed in gen.CASES:
        assert os.path.getsize(os.path.join(golden, name + '.npz')) < 480 * 1024
        z = pc.load_golden(name)
        assert z['pcl'].shape == (N, D) and z['out'].shape == (N, D) and z['out_flip'].shape == (N, D) and z['out'].dtype == np.float32
        assert (int(z['height']), int(z['width'])) == (H, W) and z['depth_image'].shape == (H, W) and float(z['margin']) == margin
        assert N < 7 or ((z['out'][:, 2] < 0).any() and (z['out'][:, 2] > 0).any())               # points behind the camera too
        assert not gen.pixel_violations(z['out'], H, W).any()                                     # the margin condition holds ...
        assert not gen.visibility_violations(z['out'], z['depth_image'], margin).any()            # ... for EVERY row
        assert np.array_equal(z['out'][:, 3:], z['pcl'][:, 3:]) and np.array_equal(z['out_flip'][:, [1, 0, 2]], z['out'][:, :3])
    assert abs(pc.load_golden('project_skew_n257')['cam_K'][0, 1]) > 0.1                          # (a skewed K)
    assert os.path.getsize(os.path.join(golden, gen.ROUNDTRIP + '.npz')) < 480 * 1024


@pytest.mark.parametrize('name', gen.NAMES)
def test_projection_equals_the_reference(twin, name):
    codes = pc.check_golden(name, CPU)
    if codes.shape[1] >= 257:
        assert set(np.unique(codes)) == {0, 1, 2}, name


@pytest.mark.parametrize('n', pc.ROW_COUNTS)
def test_case_matrix(twin, n):
    assert pc.check_matrix(n, CPU) == pc.cells_of(n)
    assert pc.cells_of(1025) == 2 * 4 * 2 * 3 * 4 * 2 and pc.cells_of(262401) == 2 * 2 * 2 and pc.cells_of(0) == 192


def test_all_rows_on_one_pixel(twin):
    assert pc.check_one_pixel(CPU)


def test_key_image_with_foreign_indices(twin):
    pc.check_foreign_keys(CPU)


def test_adversarial_rows_are_classified(twin):
    """What the pool is there for, spelled out under the identity camera: which rows take part, and who wins the ties."""
    rows = np.concatenate([pc.adversarial_rows(), np.zeros((15, pc.D - 3), np.float32)], axis=1)
    rt_np, k_np = pc.cameras(1, 37, 53)
    rt, k = torch.from_numpy(rt_np), torch.from_numpy(k_np)
    t = torch.from_numpy(rows)
    code = pk.ops.visibility(t, rt, k, torch.zeros(1, 37, 53), 0.0)[0].tolist()
    #       ties 2.0      0  -0  subn inf nan  +-3e30  nan inf x  -inf  ties 5.0
    assert code == [0, 0, 0, 2, 2, 0, 2, 2, 2, 2, 2, 2, 2, 0, 0]                                  # (a subnormal depth is a depth)
    index = pk.ops.zbuffer_resolve(pk.ops.zbuffer_splat(t, rt, k, 37, 53), t)[1]
    assert sorted(set(index.reshape(-1).tolist())) == [-1, 0, 5, 13]                                  # the lowest row of each tie
    uvz = pk.ops.project_points(t, rt, k)[0].numpy()
    assert np.isnan(uvz[7, 2]) and np.isinf(uvz[6, 2]) and abs(uvz[8, 0]) > 1e30 and uvz[5, 2] == np.float32(1e-40)


def test_round_trip_with_the_front_end(twin):
    pc.check_roundtrip(CPU)


def test_argument_errors(twin):
    pc.check_argument_errors(CPU)


def test_evaluate_clip_groups_by_visibility(twin):
    pc.check_evaluate_clip(CPU)
