"""The coarse-to-fine decode of the query grid on the HIP path (csrc/refine.hip): the case matrix, the expansion's guard and the
end-to-end comparisons of tests/test_refine_host.py on the device (the kernels and the g++ twin share their per-element source),
and results that do not depend on the stream or the run.  Everything EQUAL.

If a refined call ever differs from the restatement end to end, compare its decoded rows with the dense call's first: the mark
and the expansion are pinned by the matrix."""
import ctypes

import numpy as np
import pytest
import torch

import refine_cases as rc
import occlusions4d_amd as pk

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def shared():
    return rc.Shared(DEV)


def test_hip_library_exports_the_symbols():
    handle = ctypes.CDLL(pk._lib.LIB_PATH)
    for name in pk._lib.REFINE_SIGNATURES:
        assert hasattr(handle, name), name
    assert sorted(pk._lib.REFINE_SIGNATURES) == ['occ4d_refine_expand_f32', 'occ4d_refine_mark_f32']


@pytest.mark.parametrize('counts', rc.GRIDS, ids=lambda c: '%dx%dx%d' % c)
def test_entry_point_matrix(counts):
    assert rc.check_matrix(counts, DEV) == rc.cells_of(counts)


def test_entry_points_on_more_than_1024_tiles():
    rc.check_large(DEV)


def test_expand_guard():
    rc.check_expand_guard(DEV)


def test_argument_errors():
    rc.check_argument_errors(DEV)


def test_does_not_depend_on_the_stream_or_the_run():
    """Two calls on each of three streams: equal bits (no atomics, every element has one owner)."""
    counts, b, g = rc.LARGE_GRID, 2, 5
    n, blocks = 65 ** 3, 33 ** 3
    rng = np.random.default_rng(23)
    raw = rc.densities('pool', blocks, rng)
    density = torch.from_numpy(raw).to(DEV)
    want_active, want_key = rc.restate_mark(rc.squashed(raw, 1, DEV), counts, b, 1, rc.LOW)
    n_fine = int(want_key.sum())
    rep_out = rc.rows_on(DEV, blocks, g, False, lambda r: r)[1]
    fine_out = rc.rows_on(DEV, n_fine, g, False, lambda r: -(r + 1))[1]
    want = rc.restate_expand(want_key, counts, b, rep_out.cpu().numpy(), fine_out.cpu().numpy())
    rows = torch.zeros((n, 1), device=DEV)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(3)]
    results = []
    for _ in range(2):
        for st in streams:
            with torch.cuda.stream(st):
                key, active = pk.ops.refine_mark(density, counts, b, 1, float(rc.LOW), op=1)
                _, count, offsets = pk.ops.compact_rows_with_offsets(rows, key, 0.5)
                results.append((key, active, count, pk.ops.refine_expand(key, offsets, rep_out, fine_out, counts, b)))
    torch.cuda.synchronize()
    for key, active, count, out in results:
        assert count == n_fine and np.array_equal(active.cpu().numpy(), want_active)
        assert rc.same_bits(key.cpu().numpy(), want_key) and rc.same_bits(out.cpu().numpy(), want)


@pytest.mark.parametrize('dilate', [0, 1])
def test_single_run_equals_the_restatement_on_the_dense_output(shared, dilate):
    rc.check_single_run(shared, dilate)


def test_low_0_is_the_dense_result_and_low_2_decodes_the_representatives_only(shared):
    rc.check_low_extremes(shared)


def test_track_mode_all_device_merge_equals_host_merge(shared):
    rc.check_track_all(shared)


def test_scorers_see_the_expanded_array(shared):
    rc.check_scorers(shared)


def test_evaluate_clip_passes_refine_through(shared):
    rc.check_clip(shared)


def test_refine_none_is_untouched(shared, monkeypatch):
    rc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared):
    rc.check_value_errors(shared)
