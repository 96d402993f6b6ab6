"""Measured returns carved into the query grid on the HIP path (csrc/evidence.hip): the case matrix, the hand-worked walks, the
contention and drop cases, the pins to sight.look and the end-to-end comparisons of tests/test_evidence_host.py on the device (the
kernels and the g++ twin share csrc/evidence_math.hpp, but not where the marks land: here they are integer atomics), and results that
do not depend on the stream or the run.  Everything EQUAL to the numpy restatement of include/ext/occ4d_evidence.h.

If the product ever differs from the restatement end to end, compare result['implicit_output'] with the call without `evidence`
first: the entry points are pinned by the matrix."""
import ctypes

import numpy as np
import pytest
import torch

import evidence_cases as ec
import refine_cases as rc
import occlusions4d_amd as pk

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def shared():
    return rc.Shared(DEV)


def test_hip_library_exports_the_symbols():
    handle = ctypes.CDLL(pk._lib.LIB_PATH)
    for name in pk._lib.EVIDENCE_SIGNATURES:
        assert hasattr(handle, name), name
    assert sorted(pk._lib.EVIDENCE_SIGNATURES) == ec.SYMBOLS
    assert pk._lib.ADDON_HEADERS['EVIDENCE'] == 'ext/occ4d_evidence.h'


@pytest.mark.parametrize('counts', ec.GRIDS, ids=lambda c: '%dx%dx%d' % c)
def test_entry_point_matrix(counts):
    """Grids (the last above 2^20 cells) x R = 0, 1, 63, 64, 65, 1000 x V = 1, 3, 40 with sensors inside, outside, 2^20 cells away
    and in their returns' own cell: framed outputs EQUAL to the restatement, twice, permuted, with and without counts."""
    assert ec.check_matrix(counts, DEV) == len(ec.matrix_cells(counts))


@pytest.mark.parametrize('counts', [(96, 96, 58), (128, 128, 64)], ids=lambda c: '%dx%dx%d' % c)
def test_bits_staged_beyond_64_kib_of_lds(counts):
    """The near side of the capacity rule: the published grid and the grid of exactly 2^20 cells."""
    ec.check_capacity_near_side(DEV, counts)


def test_walks_worked_by_hand():
    ec.check_hand_worked(DEV)


def test_contention():
    ec.check_contention(DEV)


def test_drops_are_counted_in_their_priority():
    ec.check_drops(DEV)


def test_pinned_to_the_walk_of_sight():
    ec.check_pinned_to_the_walk_of_sight(DEV)


@pytest.mark.parametrize('share,seed', [(0.15, 11), (0.30, 12)])
def test_seen_solids_contradict_nothing(share, seed):
    ec.check_seen_solids_contradict_nothing(DEV, share, seed)


def test_consequences():
    ec.check_consequences(DEV)


def test_argument_errors():
    ec.check_argument_errors(DEV)


def test_does_not_depend_on_the_stream_or_the_run():
    """Two calls on each of three streams: equal bits (integer sums and ORs commute)."""
    counts = (40, 40, 40)
    rng = np.random.default_rng(41)
    returns, sensor, origins = ec.scene(counts, 1000, 3, rng)
    want = ec.restate_carve(returns, sensor, origins, counts)
    ret, sen, org = ec.on(DEV, returns), ec.on(DEV, sensor), ec.on(DEV, origins)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(3)]
    results = []
    for _ in range(2):
        for st in streams:
            with torch.cuda.stream(st):
                results.append(pk.ops.grid_carve(ret, org, counts, ec.MINS, ec.SPACINGS, sen, True))
    torch.cuda.synchronize()
    for passed, hits, passes, status in results:
        got = dict(passed=passed.cpu().numpy(), hits=hits.cpu().numpy(), passes=passes.cpu().numpy(), status=status.cpu().numpy())
        ec.same_carve(got, want, True, 'streams')


def test_perform_inference_with_evidence(shared, monkeypatch):
    ec.check_end_to_end(shared, monkeypatch)


def test_evaluate_clip_appends_the_evidences(shared):
    ec.check_clip(shared)


def test_evidence_none_is_untouched(shared, monkeypatch):
    ec.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared):
    ec.check_value_errors(shared)


def test_signature_positions():
    ec.check_signatures()
