"""The virtual lidar sweep of the decoded field (include/ext/occ4d_sweep.h, ops.sweep_rays, sweep.FieldSweep / cast and the helpers
lidar_directions, directions_to, poses, march_range, rows_of, residual, perform_inference(sweep=...)) through the g++ twin, without a
GPU: the header and its binding, the case matrix of tests/sweep_cases.py against the restatement of the header, which walks every
sample, the placements, the hand-built owner cells, the two independent checks against float64, the option object, and
perform_inference / evaluate_clip on the refine fixture -- everything but the two independent checks EQUAL, no tolerance.  The twin
and the HIP kernel share the item body of a ray and the argument contract (csrc/sweep_math.hpp), but not the mapping of rays to
threads.  tests/test_gpu_sweep.py runs the same comparisons on the device."""
import ctypes

import pytest
import torch

import refine_cases as rc
import sweep_cases as sc
import occlusions4d_amd as pk

CPU = torch.device('cpu')


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


def test_symbol_is_in_the_open_table_and_in_no_other():
    """ADDON_HEADERS is open by design: this header's symbol is IN it -- the table is never compared with it."""
    lib = pk._lib
    assert lib.ADDON_HEADERS['SWEEP'] == 'ext/occ4d_sweep.h' and ('SWEEP', 'ext/occ4d_sweep.h', 'addon', True) in lib.HEADERS
    for table in (lib.FEATURE_HEADERS, lib.EXTENSION_HEADERS, lib.STRUCT_EXTENSION_HEADERS):
        assert 'SWEEP' not in table
    with open(lib.SWEEP_HEADER_PATH) as f:
        text = f.read()
    assert lib.SWEEP_SIGNATURES == lib.parse_prototypes(text, lib._STRUCTS) and sorted(lib.SWEEP_SIGNATURES) == sorted(sc.SYMBOLS)
    for name in sc.SYMBOLS:
        assert lib.ADDON_SIGNATURES[name] == lib.SWEEP_SIGNATURES[name]
        for other in (lib.SIGNATURES, lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
            assert name not in other
    assert lib.SWEEP_CONSTANTS == sc.CONSTANTS and lib.ABI_VERSION == 5
    assert lib.SWEEP_CONSTANTS['MAX_STEPS'] == lib.RAYCAST_CONSTANTS['MAX_STEPS']
    assert lib.SWEEP_CONSTANTS['MAX_CHANNELS'] == lib.RAYCAST_CONSTANTS['MAX_CHANNELS']
    I, L, P, F = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float
    assert lib.SWEEP_SIGNATURES['occ4d_sweep_rays_f32'] == (
        I, [P, L, I, I, I, F, F, F, F, F, F, F, P, P, I, I, I, I, F, F, I, P, L, I, P, I, I, I, P, I, F, F] + [P] * 9)
    for phrase in ('THE RULES', 'RAYS', 'GRADIENT', 'COS', 'OWNER', 'OUTPUTS', 'ACCESS SAFETY', 'occ4d_raycast.h', 'NOT normalised',
                   'fmaf(Rm_a2, d2, fmaf(Rm_a1, d1, Rm_a0 * d0))', 'den > 0.0f ? fminf(fabsf(nd) / den, 1.0f) : 0.0f',
                   'inst == -1 CAN OCCUR AT A HIT', 'A NaN never wins', 'touches no pointer', 'the very floats'):
        assert phrase in text, phrase


def test_twin_exports_and_binds_the_prototype(twin):
    lib = pk._lib.lib()
    handle = ctypes.CDLL(pk.cpu_twin.LIB)
    for name, (res, args) in pk._lib.SWEEP_SIGNATURES.items():
        assert hasattr(handle, name), name
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_package_exports():
    for name in ('FieldSweep', 'cast', 'lidar_directions', 'directions_to', 'poses', 'march_range', 'rows_of', 'residual'):
        assert hasattr(pk.sweep, name), name
    assert hasattr(pk.ops, 'sweep_rays') and pk.ops.SWEEP_ARRAYS == sc.NAMES and 'sweep' in pk.__all__


def test_the_math_header_calls_the_ray_casts_functions():
    """csrc/sweep_math.hpp includes csrc/raycast_math.hpp and calls its march, clamp, cell, lerp and trilinear; it restates none."""
    with open(pk._lib.LIB_PATH.replace('libocc4d.so', 'csrc/sweep_math.hpp')) as f:
        text = f.read()
    assert '#include "raycast_math.hpp"' in text
    for used in ('ry::march(', 'ry::clamped_coord(', 'ry::cell_of(', 'ry::trilinear(', 'ry::lerp('):
        assert used in text, used
    assert 'row4' not in text and '- 0.5f' not in text and 'floorf' not in text


@pytest.mark.parametrize('counts', sc.GRIDS, ids=lambda c: '%dx%dx%d' % c)
def test_matrix_equals_the_restatement(twin, counts):
    assert sc.check_matrix(counts, CPU) == len(sc.matrix_cells(counts))


def test_placements(twin):
    sc.check_placements(CPU)


def test_axis_rays_exactly_through_grid_points(twin):
    sc.check_axis_rays_through_grid_points(CPU)


def test_zero_and_nan_directions(twin):
    sc.check_zero_and_nan_directions(CPU)


def test_owner_of_hand_built_cells(twin):
    sc.check_owner(CPU)


def test_owner_of_a_cell_the_samples_stepped_over(twin):
    sc.check_owner_of_a_skipped_cell(CPU)


def test_owner_of_a_hit_on_a_slab_is_a_slab_point(twin):
    sc.check_slab(CPU)


def test_analytic_range_and_incidence_on_a_linear_field(twin):
    """(a) The twin IS where the tolerances come from: ANALYTIC_RANGE_WORST / ANALYTIC_COS_WORST, 4 x as tolerance."""
    sc.check_analytic_plane(CPU)


def test_replay_of_points_on_the_plane(twin):
    """(b) REPLAY_WORST on the twin, 4 x as tolerance."""
    sc.check_replay_of_plane_points(CPU)


def test_host_helpers():
    sc.check_host_helpers()


def test_argument_errors(twin):
    sc.check_argument_errors(CPU)


def test_option():
    sc.check_option()


def test_signature_positions():
    sc.check_signatures()


def test_perform_inference_with_sweep(shared, twin, monkeypatch):
    sc.check_end_to_end(shared, monkeypatch)


def test_sem_comes_from_the_last_columns_of_a_call_that_predicts_segmentation(twin):
    sc.check_segmentation(CPU)


def test_evaluate_clip_appends_the_sweeps(shared, twin):
    sc.check_clip(shared)


def test_none_is_untouched(shared, twin, monkeypatch):
    sc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared, twin):
    sc.check_value_errors(shared)
