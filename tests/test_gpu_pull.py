"""Straight free legs over the query grid on the HIP path (csrc/pull.hip): the cases of tests/pull_cases.py through libocc4d.so, EQUAL
to the restatement of the header's rules and to the g++ twin bit for bit (the twin loaded as a second plain handle: the kernels and
the twin share the blocked test, HIT and the candidate test; the pull kernel tests 256 candidates of an anchor at a time and reduces
the largest free one over the workgroup, the twin takes them one by one), every call twice with equal bits, and the consequences and
the end-to-end comparisons of tests/test_pull_host.py on the device.  Integers only; the one tolerance is derived in
pull_cases.LENGTH_MARGIN; no grid is larger than 33 x 34 x 35 but for the two either side of the staging limit."""
import ctypes

import pytest
import torch

import pull_cases as pc
import refine_cases as rc
import occlusions4d_amd as pk

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def shared():
    return rc.Shared(DEV)


@pytest.fixture(scope='module')
def twin_handle():
    handle = pk._lib.bind(ctypes.CDLL(pk.cpu_twin.build()), missing=lambda name: None)      # a second handle: enable() is not called
    assert not pk.cpu_twin.enabled() and handle.occ4d_is_cpu_twin() == 1
    return handle


def test_hip_library_exports_the_symbols():
    handle = ctypes.CDLL(pk._lib.LIB_PATH)
    for name in pc.SYMBOLS:
        assert hasattr(handle, name) and name in pk._lib.ADDON_SIGNATURES, name
    assert pk._lib.ADDON_HEADERS['PULL'] == 'ext/occ4d_pull.h'


def test_bits_equal_the_restatement_and_the_twin(twin_handle):
    assert pc.check_bits(DEV, twin_handle) == len(pc.BIT_LENGTHS) * len(pc.MIN_CLEARS) * 2


@pytest.mark.parametrize('counts', pc.PAIR_GRIDS, ids=pc.PAIR_GRID_IDS)
def test_pairs_equal_the_restatement_and_the_twin_twice(twin_handle, counts):
    assert pc.check_pairs(counts, DEV, twin_handle) == len(pc.FIELDS) * 2


def test_pair_counts_round_the_wave(twin_handle):
    pc.check_pair_counts(DEV, twin_handle)


def test_consequences_of_the_rules():
    pc.check_consequences(DEV)


@pytest.mark.parametrize('name', [n for n in pc.PULL_NAMES if n not in pc.RANDOM30])
def test_pulled_paths_equal_the_restatement_and_the_twin_twice(twin_handle, name):
    pc.check_pull_case(name, DEV, twin_handle)


def test_random_fields_take_the_fallback_leg(twin_handle):
    assert sum(pc.check_pull_case(name, DEV, twin_handle) for name in pc.RANDOM30) >= 1


def test_pinned_shapes():
    pc.check_pinned_shapes(DEV)


def test_hand_made_chains_through_the_raw_entry_point(twin_handle):
    pc.check_hand_chains(DEV, pk._lib.lib())
    pc.check_hand_chains('cpu', twin_handle)


@pytest.mark.parametrize('counts', pc.THRESHOLD_GRIDS, ids=['largest-staged', 'first-beyond'])
def test_either_side_of_the_staging_limit(twin_handle, counts):
    pc.check_threshold(counts, DEV, pk._lib.lib())
    pc.check_threshold(counts, 'cpu', twin_handle)


def test_argument_errors():
    pc.check_argument_errors(DEV)


def test_paths_to_world_takes_waypoints():
    pc.check_paths_to_world_takes_waypoints(DEV)


def test_perform_inference_with_pull(shared, monkeypatch):
    pc.check_end_to_end(shared, monkeypatch)


def test_evaluate_clip_passes_the_waypoints_through(shared):
    pc.check_clip(shared)


def test_pull_false_is_untouched(shared, monkeypatch):
    pc.check_pull_false_is_untouched(shared, monkeypatch)
