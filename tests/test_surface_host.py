"""The occupancy surface as a quad mesh (include/occ4d_surface.h, surface.py, inference.perform_inference(surface=...)) through the
g++ twin, without a GPU: the header and its binding, the two entry points against the numpy restatement of the rules over the case
matrix of tests/surface_cases.py, the guard of the data-dependent positions, the mesh properties that need no restatement, and
perform_inference / evaluate_clip with a Surface on the tracking fixture -- everything but the properties EQUAL, no tolerance.
The twin and the HIP kernels share the per-element source (csrc/surface_math.hpp); tests/test_gpu_surface.py runs the same
comparisons on the device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import refine_cases as rc
import surface_cases as sc
import occlusions4d_amd as pk

CPU = torch.device('cpu')
NAMES = ['occ4d_surface_count_f32', 'occ4d_surface_write_f32']


@pytest.fixture
def twin():
    pk.cpu_twin.enable()
    try:
        yield pk
    finally:
        pk.cpu_twin.disable()


@pytest.fixture(scope='module')
def shared():
    pk.cpu_twin.enable()
    try:
        return rc.Shared(CPU)
    finally:
        pk.cpu_twin.disable()


def test_signature_table_matches_the_header():
    lib = pk._lib
    assert lib.FEATURE_HEADERS['SURFACE'] == 'occ4d_surface.h' and len(lib.FEATURE_HEADERS) == 8
    with open(lib.SURFACE_HEADER_PATH) as f:
        text = f.read()
    assert lib.SURFACE_SIGNATURES == lib.parse_prototypes(text, {})
    assert sorted(lib.SURFACE_SIGNATURES) == NAMES
    for prefix in lib.FEATURE_HEADERS:
        if prefix != 'SURFACE':
            assert not set(getattr(lib, prefix + '_SIGNATURES')) & set(NAMES), prefix
    assert not set(lib.SIGNATURES) & set(NAMES)
    assert lib.parse_constants(text) == {} and lib.ABI_VERSION == 5
    I, L, F, P = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    assert lib.SURFACE_SIGNATURES['occ4d_surface_count_f32'] == (I, [P, L, I, I, I, F, P, P, P, P])
    assert lib.SURFACE_SIGNATURES['occ4d_surface_write_f32'] == (I, [P, L, P, L, I, I, I, I, F, F, F, F, F, F, F, P, P, P, P, L, I, P, I, P])


def test_twin_exports_and_binds_the_prototypes(twin):
    lib = pk._lib.lib()
    handle = ctypes.CDLL(pk.cpu_twin.LIB)
    for name, (res, args) in pk._lib.SURFACE_SIGNATURES.items():
        assert hasattr(handle, name), name
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_restatement_on_grids_worked_by_hand():
    """One inside point in a 3 x 3 x 3 grid: eight cells, each with three crossed edges at t = 0.5; six quads."""
    dens = np.zeros((3, 3, 3), np.float32)
    dens[1, 1, 1] = 1.0
    want = sc.restate(dens.reshape(-1), (3, 3, 3), 0.5, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert want['totals'].tolist() == [8, 6] and want['work'].reshape(3, 3, 3)[:2, :2, :2].reshape(-1).tolist() == list(range(8))
    assert (want['work'].reshape(3, 3, 3)[2] == -1).all()
    # cell (0, 0, 0): its crossed edges end in corner (1, 1, 1): the mean of (0.5, 1, 1), (1, 0.5, 1), (1, 1, 0.5), plus 0.5
    third = np.float32(2.5) / np.float32(3.0)
    assert sc.same_bits(want['vertices'][0], np.full(3, np.float32(0.5) + third, np.float32))
    # faces in the order p * 3 + a: p = (0, 1, 1) on x, (1, 0, 1) on y, (1, 1, 0) on z (outside: reversed), p = (1, 1, 1) on x, y, z
    assert want['faces'].tolist() == [[1, 3, 2, 0], [4, 5, 1, 0], [2, 6, 4, 0], [4, 6, 7, 5], [2, 3, 7, 6], [1, 5, 7, 3]]
    # the tile numbering: 300 items in two tiles
    flags = np.arange(300) % 3 == 0
    assert sc.true_offsets(flags).tolist() == [0, 86]
    assert sc.tile_numbers(flags, flags, [0, 86])[[0, 3, 255, 256, 258]].tolist() == [0, 1, 85, 86, 86]
    assert sc.tile_numbers(flags, flags, [10, -5])[[3, 258]].tolist() == [11, -5]


@pytest.mark.parametrize('counts', sc.GRIDS, ids=lambda c: '%dx%dx%d' % c)
def test_entry_point_matrix(twin, counts):
    assert sc.check_matrix(counts, CPU) == sc.cells_of() == 10


def test_entry_points_on_more_than_1024_tiles(twin):
    sc.check_large(CPU)


def test_one_inside_point(twin):
    sc.check_one_inside_point(CPU)


def test_guard(twin):
    sc.check_guard(CPU)


def test_sphere_is_closed_oriented_and_of_genus_0(twin):
    sc.check_sphere(CPU)


def test_plane_at_the_exact_crossing(twin):
    sc.check_plane(CPU)


def test_argument_errors(twin):
    sc.check_argument_errors(CPU)


def test_signatures_default_to_none():
    sig = inspect.signature(pk.inference.perform_inference).parameters
    assert sig['surface'].default is None and inspect.signature(pk.evaluation.evaluate_clip).parameters['surface'].default is None
    assert 'surface' in pk.__all__ and pk.ops.surface_capacity((3, 4, 5)) == (24, 2 * 2 * 3 + 1 * 3 * 3 + 1 * 2 * 4)


def test_grid_frame_is_what_the_sampler_hands_to_grid_points(twin, monkeypatch):
    seen = []
    grid_points = pk.ops.grid_points
    monkeypatch.setattr(pk.ops, 'grid_points', lambda *a: seen.append(a[:3]) or grid_points(*a))
    for num, min_z, cb, kind, mode in ((1500, -1.0, 5.0, 'greater', 4), (4000, -0.5, 16.0, 'carla', 4)):
        pk.geometry.sample_implicit_points_blind_device(num, min_z, cb, 1, kind, mode, 'grid', CPU)
        frame = pk.geometry.grid_frame(num, min_z, cb, kind, mode)
        assert seen[-1] == tuple(frame) and tuple(frame[0]) == pk.geometry.grid_counts(num, min_z, cb, kind, mode)


def test_single_run_equals_the_restatement(twin, shared):
    sc.check_single_run(shared)


def test_under_refine_the_mesh_is_that_of_the_expanded_array(twin, shared):
    sc.check_refine(shared)


def test_track_mode_all_meshes_the_merged_array(twin, shared):
    sc.check_track_all(shared)


def test_evaluate_clip_passes_surface_through(twin, shared):
    sc.check_clip(shared)


def test_surface_none_is_untouched(twin, shared, monkeypatch):
    sc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(twin, shared):
    sc.check_value_errors(shared)


def test_write_ply_reads_back(tmp_path):
    sc.check_write_ply(tmp_path)
