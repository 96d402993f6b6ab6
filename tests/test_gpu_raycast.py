"""The decoded field ray-cast into camera views on the HIP path (csrc/raycast.hip): the case matrix, the placements, the null
outputs, the exact cases, the two independent checks and the end-to-end comparisons of tests/test_raycast_host.py on the device
(the kernel and the g++ twin share their per-ray source), and results that do not depend on the stream or the run.  Everything
but the two independent checks EQUAL.

If the images ever differ from the restatement end to end, compare result['implicit_output'] with the call without `views` first:
the entry point is pinned by the matrix."""
import ctypes

import numpy as np
import pytest
import torch

import raycast_cases as yc
import refine_cases as rc
import occlusions4d_amd as pk

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def shared():
    return rc.Shared(DEV)


def test_hip_library_exports_the_symbol():
    handle = ctypes.CDLL(pk._lib.LIB_PATH)
    for name in pk._lib.RAYCAST_SIGNATURES:
        assert hasattr(handle, name), name
    assert sorted(pk._lib.RAYCAST_SIGNATURES) == ['occ4d_raycast_grid_f32']
    assert pk._lib.EXTENSION_HEADERS['RAYCAST'] == 'ext/occ4d_raycast.h'


@pytest.mark.parametrize('counts', yc.GRIDS, ids=lambda c: '%dx%dx%d' % c)
def test_entry_point_matrix(counts):
    assert yc.check_matrix(counts, DEV) == len(yc.matrix_cells(counts))


def test_camera_placements():
    yc.check_placements(DEV)


def test_null_outputs():
    yc.check_null_outputs(DEV)


def test_rays_exactly_through_grid_points():
    yc.check_exact_grid_points(DEV)


def test_first_point_is_solid():
    yc.check_first_point_is_solid(DEV)


def test_argument_errors():
    yc.check_argument_errors(DEV)


def test_round_trip_through_the_projection():
    """(a) Worst difference from the float64 camera chain on the g++ twin: 2.55e-7; tolerance 4 x = 1.02e-6."""
    yc.check_round_trip(DEV)


def test_analytic_depth_of_a_linear_field():
    """(b) Worst error against the analytic depth on the g++ twin: 2.29e-8; tolerance 4 x = 9.16e-8."""
    yc.check_analytic_depth(DEV)


def test_does_not_depend_on_the_stream_or_the_run():
    """Two calls on each of three streams: equal bits (no atomics, every element has one owner)."""
    counts, (H, W), cols = (17, 9, 33), (20, 33), [0, 3, 5]
    n = counts[0] * counts[1] * counts[2]
    rng = np.random.default_rng(29)
    field, attrs = yc.blob(counts, rng), yc.attributes(n, rng)
    rt_inv, k_inv = yc.inverses(*yc.cameras(['outside', 'side', 'inside'], counts, H, W))
    near, step = yc.march_of(counts, 64)
    want = yc.restate(field, counts, yc.MINS, yc.SPACINGS, yc.LEVEL, k_inv, rt_inv, H, W, near, step, 64, attrs, cols)
    assert want['hit'].any()
    field_t, attrs_t, rt_t, k_t = (torch.from_numpy(a).to(DEV) for a in (field, attrs, rt_inv, k_inv))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(3)]
    results = []
    for _ in range(2):
        for st in streams:
            with torch.cuda.stream(st):
                results.append(pk.ops.raycast_grid(field_t, counts, yc.MINS, yc.SPACINGS, float(yc.LEVEL), rt_t, k_t, H, W, float(near),
                                                   float(step), 64, attrs=attrs_t, channels=cols))
    torch.cuda.synchronize()
    for got in results:
        assert yc.same_images([g.cpu().numpy() for g in got], want)


def test_single_run_equals_the_restatement(shared):
    yc.check_single_run(shared)


def test_select_shows_the_tracked_object_alone(shared):
    yc.check_select(shared)


def test_under_refine_the_views_are_those_of_the_expanded_array(shared):
    yc.check_refine(shared)


def test_track_mode_all_renders_the_merged_array(shared):
    yc.check_track_all(shared)


def test_evaluate_clip_passes_views_through(shared):
    yc.check_clip(shared)


def test_views_none_is_untouched(shared, monkeypatch):
    yc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared):
    yc.check_value_errors(shared)
