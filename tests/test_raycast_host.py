"""The decoded field ray-cast into camera views (include/ext/occ4d_raycast.h, projection.render_field, inference.perform_inference(
views=...)) through the g++ twin, without a GPU: the header and its binding, the entry point against the numpy restatement of the
rules over the case matrix of tests/raycast_cases.py, the two checks that need no restatement, and perform_inference /
evaluate_clip with a FieldViews on the tracking fixture -- everything but those two checks EQUAL, no tolerance.  The twin and the
HIP kernel share the per-ray source (csrc/raycast_math.hpp); tests/test_gpu_raycast.py runs the same comparisons on the device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import raycast_cases as yc
import refine_cases as rc
import occlusions4d_amd as pk

CPU = torch.device('cpu')
NAMES = ['occ4d_raycast_grid_f32']


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
    assert lib.EXTENSION_HEADERS['RAYCAST'] == 'ext/occ4d_raycast.h' and 'RAYCAST' not in lib.FEATURE_HEADERS
    assert lib.EXTENSION_SIGNATURES == lib.RAYCAST_SIGNATURES and not set(lib.ALL_SIGNATURES) & set(NAMES)
    with open(lib.RAYCAST_HEADER_PATH) as f:
        text = f.read()
    assert lib.RAYCAST_SIGNATURES == lib.parse_prototypes(text, {})
    assert sorted(lib.RAYCAST_SIGNATURES) == NAMES
    for prefix in lib.FEATURE_HEADERS:
        assert not set(getattr(lib, prefix + '_SIGNATURES')) & set(NAMES), prefix
    assert not set(lib.SIGNATURES) & set(NAMES)
    assert lib.RAYCAST_CONSTANTS == {'MAX_STEPS': 65536, 'MAX_CHANNELS': 32} and lib.ABI_VERSION == 5
    I, L, F, P = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    assert lib.RAYCAST_SIGNATURES['occ4d_raycast_grid_f32'] == (
        I, [P, L, I, I, I, F, F, F, F, F, F, F, P, P, I, I, I, F, F, I, P, L, I, P, I, F, F, P, P, P, P])


def test_twin_exports_and_binds_the_prototype(twin):
    lib = pk._lib.lib()
    handle = ctypes.CDLL(pk.cpu_twin.LIB)
    for name, (res, args) in pk._lib.RAYCAST_SIGNATURES.items():
        assert hasattr(handle, name), name
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_restatement_on_a_ray_worked_by_hand():
    """A 2 x 2 x 2 grid in the exact frame (points at 0 and 0.25), the identity camera at z = -0.5, pixel (0, 0): the ray runs along
    the edge (0, 0, .) whose values are 0 and 1; level 0.5 is crossed half way between the samples at depths 0.5 and 0.75."""
    field = np.zeros((2, 2, 2), np.float32)
    field[:, :, 1] = 1.0
    eye = np.eye(4, dtype=np.float32)
    rt_inv = eye.copy()
    rt_inv[2, 3] = -0.5
    want = yc.restate(field.reshape(-1), (2, 2, 2), yc.EXACT_MINS, yc.EXACT_SPACINGS, 0.5, eye[None], rt_inv[None], 1, 1, 0.25, 0.25, 4,
                      attrs=np.arange(16, dtype=np.float32).reshape(8, 2), cols=[1])
    assert want['depth'].tolist() == [[[0.625]]] and want['cell'].tolist() == [[[0]]] and want['hit'].all()
    assert want['position'].tolist() == [[[[0.0, 0.0, 0.125]]]]
    assert want['features'].tolist() == [[[[2.0]]]]                       # between rows 0 (column 1: 1) and 1 (3), half way
    # a level nothing reaches: the background
    want = yc.restate(field.reshape(-1), (2, 2, 2), yc.EXACT_MINS, yc.EXACT_SPACINGS, 1.5, eye[None], rt_inv[None], 1, 1, 0.25, 0.25, 4,
                      background=-3.0)
    assert want['depth'].tolist() == [[[-3.0]]] and want['cell'].tolist() == [[[-1]]]


@pytest.mark.parametrize('counts', yc.GRIDS, ids=lambda c: '%dx%dx%d' % c)
def test_entry_point_matrix(twin, counts):
    assert yc.check_matrix(counts, CPU) == len(yc.matrix_cells(counts)) == 17


def test_matrix_covers_every_value_of_every_factor():
    cells = yc.matrix_cells((3, 2, 5))
    assert {c[0] for c in cells} == set(yc.IMAGES) and {len(c[1]) for c in cells} >= set(yc.VIEW_COUNTS)
    assert {p for c in cells for p in c[1]} == set(yc.PLACEMENTS)
    assert {c[2] for c in cells} == set(yc.STEP_COUNTS) and {c[3] for c in cells} == set(yc.CHANNEL_COUNTS)
    assert {c[4] for c in cells} == {False, True} and {c[5] for c in cells} == {'pool', 'blob', 'all_above', 'all_below'}


def test_camera_placements(twin):
    yc.check_placements(CPU)


def test_null_outputs(twin):
    yc.check_null_outputs(CPU)


def test_rays_exactly_through_grid_points(twin):
    yc.check_exact_grid_points(CPU)


def test_first_point_is_solid(twin):
    yc.check_first_point_is_solid(CPU)


def test_argument_errors(twin):
    yc.check_argument_errors(CPU)


def test_round_trip_through_the_projection(twin):
    """(a) Worst difference from the float64 camera chain on the g++ twin: 2.55e-7; tolerance 4 x = 1.02e-6."""
    yc.check_round_trip(CPU)


def test_analytic_depth_of_a_linear_field(twin):
    """(b) Worst error against the analytic depth on the g++ twin: 2.29e-8; tolerance 4 x = 9.16e-8."""
    yc.check_analytic_depth(CPU)


def test_signatures_default_to_none():
    sig = inspect.signature(pk.inference.perform_inference).parameters
    assert sig['views'].default is None
    sig = inspect.signature(pk.evaluation.evaluate_clip).parameters
    assert sig['views'].default is None and sig['images'].default is None


def test_single_run_equals_the_restatement(twin, shared):
    yc.check_single_run(shared)


def test_select_shows_the_tracked_object_alone(twin, shared):
    yc.check_select(shared)


def test_under_refine_the_views_are_those_of_the_expanded_array(twin, shared):
    yc.check_refine(shared)


def test_track_mode_all_renders_the_merged_array(twin, shared):
    yc.check_track_all(shared)


def test_evaluate_clip_passes_views_through(twin, shared):
    yc.check_clip(shared)


def test_views_none_is_untouched(twin, shared, monkeypatch):
    yc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(twin, shared):
    yc.check_value_errors(shared)
