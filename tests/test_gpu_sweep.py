"""The virtual lidar sweep of the decoded field on the HIP path (csrc/sweep.hip): the case matrix, the placements, the owner cells,
the two independent checks and the end-to-end comparisons of tests/test_sweep_host.py on the device (the kernel and the g++ twin
share their per-ray source, csrc/sweep_math.hpp, but not the mapping of rays to threads), and results that do not depend on the
stream or the run.  Everything but the two independent checks EQUAL to the numpy restatement of include/ext/occ4d_sweep.h.

If the sweep ever differs from the restatement end to end, compare result['implicit_output'] with the call without `sweep` first:
the entry point is pinned by the matrix."""
import ctypes

import numpy as np
import pytest
import torch

import refine_cases as rc
import sweep_cases as sc
import occlusions4d_amd as pk

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def shared():
    return rc.Shared(DEV)


def test_hip_library_exports_the_symbol():
    handle = ctypes.CDLL(pk._lib.LIB_PATH)
    for name in pk._lib.SWEEP_SIGNATURES:
        assert hasattr(handle, name), name
    assert sorted(pk._lib.SWEEP_SIGNATURES) == sc.SYMBOLS
    assert pk._lib.ADDON_HEADERS['SWEEP'] == 'ext/occ4d_sweep.h'


@pytest.mark.parametrize('counts', sc.GRIDS, ids=lambda c: '%dx%dx%d' % c)
def test_entry_point_matrix(counts):
    """Grids x ray images (less than a wave, ragged waves and workgroups) x views 0 / 1 / 3 x per_view x steps x fields x each
    output alone and all together x channels x classes x labels: EQUAL to the restatement, cos included (sqrtf and the divisions
    are correctly rounded on both sides)."""
    assert sc.check_matrix(counts, DEV) == len(sc.matrix_cells(counts))


def test_placements():
    sc.check_placements(DEV)


def test_axis_rays_exactly_through_grid_points():
    sc.check_axis_rays_through_grid_points(DEV)


def test_zero_and_nan_directions():
    sc.check_zero_and_nan_directions(DEV)


def test_owner_of_hand_built_cells():
    sc.check_owner(DEV)


def test_owner_of_a_cell_the_samples_stepped_over():
    sc.check_owner_of_a_skipped_cell(DEV)


def test_owner_of_a_hit_on_a_slab_is_a_slab_point():
    sc.check_slab(DEV)


def test_argument_errors():
    sc.check_argument_errors(DEV)


def test_analytic_range_and_incidence_on_a_linear_field():
    """(a) Against the float64 plane intersection, 153 rays at ranges 2.76 .. 3.17.  Worst differences on the g++ twin: range
    5.46e-7, cos 4.16e-7; tolerances 4 x = 2.184e-6 and 1.664e-6."""
    sc.check_analytic_plane(DEV)


def test_replay_of_points_on_the_plane():
    """(b) 200 points on the level plane replayed through directions_to, measured ranges 2.70 .. 3.36.  Worst |residual| on the
    g++ twin: 4.77e-7 (one float32 step of such a range); tolerance 4 x = 1.908e-6."""
    sc.check_replay_of_plane_points(DEV)


def test_does_not_depend_on_the_stream_or_the_run():
    """Two calls on each of three streams: equal bits (no atomics, every element has one owner)."""
    counts, shape, cols = (17, 9, 33), (9, 17), [0, 3, 5]
    n = counts[0] * counts[1] * counts[2]
    rng = np.random.default_rng(29)
    field, attrs = sc.blob(counts, rng), sc.yc.attributes(n, rng)
    labels = sc.labels_of('mixed', n, rng)
    pose = np.stack([sc.placed(p, counts, field, rng) for p in ('outside', 'solid', 'free')])
    dirs = sc.bundle(shape, rng, 3, True)
    near, step = sc.march_of(counts, 64)
    want = sc.restate(field, counts, sc.MINS, sc.SPACINGS, sc.LEVEL, pose, dirs, shape, True, near, step, 64, attrs, cols, (1, 5), labels,
                      sc.K_OBJECTS, sc.BG, sc.FBG)
    assert want['hit'].any() and not want['hit'].all()
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    field_t, attrs_t, pose_t, dirs_t, labels_t = to(field), to(attrs), to(pose), to(dirs), to(labels)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(3)]
    results = []
    for _ in range(2):
        for st in streams:
            with torch.cuda.stream(st):
                results.append(pk.ops.sweep_rays(field_t, counts, sc.MINS, sc.SPACINGS, float(sc.LEVEL), pose_t, dirs_t, shape, float(near),
                                                 float(step), 64, per_view=True, attrs=attrs_t, channels=cols, sem=(1, 5),
                                                 labels=labels_t, k=sc.K_OBJECTS, background=sc.BG, feature_background=sc.FBG))
    torch.cuda.synchronize()
    for got in results:
        sc.same({name: t.cpu().numpy() for name, t in got.items()}, want)


def test_perform_inference_with_sweep(shared, monkeypatch):
    sc.check_end_to_end(shared, monkeypatch)


def test_sem_comes_from_the_last_columns_of_a_call_that_predicts_segmentation():
    sc.check_segmentation(DEV)


def test_evaluate_clip_appends_the_sweeps(shared):
    sc.check_clip(shared)


def test_sweep_none_is_untouched(shared, monkeypatch):
    sc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared):
    sc.check_value_errors(shared)


def test_signature_positions():
    sc.check_signatures()
