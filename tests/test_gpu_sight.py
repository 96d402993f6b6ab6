"""Line of sight through the decoded occupancy on the HIP path (csrc/sight.hip): the case matrix of tests/sight_cases.py through
libocc4d.so, EQUAL to the restatement of the header's rules and to the g++ twin bit for bit (the twin loaded as a second plain
handle: the kernels and the twin share the bit test, the choice of T, the SQUEEZE and the walk; the kernels give a wave a 4 x 4 x 4
block of queries, the twin goes over the queries in flat order), every call twice with equal bits, and the by-hand cases, the
consequences and the end-to-end comparisons of tests/test_sight_host.py on the device.  Integers only, no tolerance anywhere; no
case is larger than 33 x 34 x 35."""
import ctypes

import pytest
import torch

import refine_cases as rc
import sight_cases as sc
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
    for name in sc.SYMBOLS:
        assert hasattr(handle, name) and name in pk._lib.ADDON_SIGNATURES, name
    assert pk._lib.ADDON_HEADERS['SIGHT'] == 'ext/occ4d_sight.h'


def test_cases_worked_by_hand():
    sc.check_by_hand(DEV)


@pytest.mark.parametrize('counts', sc.GRIDS, ids=sc.GRID_IDS)
def test_matrix_equals_the_restatement_and_the_twin_twice(twin_handle, counts):
    assert sc.check_grid(counts, DEV, twin_handle) == len(sc.FIELDS) * len(sc.origin_counts(counts)) * 3 * 2 * len(sc.FLAGS) * 2


def test_raw_entry_points_write_nothing_else(twin_handle):
    sc.check_raw_canaries(DEV, pk._lib.lib())
    sc.check_raw_canaries('cpu', twin_handle)


def test_consequences_of_the_rules():
    sc.check_consequences(DEV)


def test_argument_errors():
    sc.check_argument_errors(DEV)


def test_look_against_the_restatement():
    sc.check_look(DEV)


def test_codes_and_by_label_against_numpy():
    sc.check_codes_and_by_label(DEV)


def test_perform_inference_with_sight(shared, monkeypatch):
    sc.check_end_to_end(shared, monkeypatch)


def test_evaluate_clip_passes_sight_through(shared):
    sc.check_clip(shared)


def test_sight_none_is_untouched(shared, monkeypatch):
    sc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared):
    sc.check_value_errors(shared)
