"""The next best view on the HIP path (csrc/viewplan.hip): the cases of tests/viewplan_cases.py through libocc4d.so, EQUAL to the
restatement of the header's rules and to the g++ twin bit for bit (the twin loaded as a second plain handle: the kernels and the twin
share DEAD, RANGE, the pair test and the keys; the VIS kernel votes 64 points of a candidate at a time and skips waves without a
target, the counts are reduced over waves, LDS and atomic adds, the twin takes everything in order), every call twice with equal
bits, and the consequences and the end-to-end comparisons of tests/test_viewplan_host.py on the device.  Integers only, no tolerance;
no grid is larger than 20 x 17 x 13, the largest GREEDY input is 1500 x 4100 words."""
import ctypes

import pytest
import torch

import viewplan_cases as vc
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
    for name in vc.SYMBOLS:
        assert hasattr(handle, name) and name in pk._lib.ADDON_SIGNATURES, name
    assert pk._lib.ADDON_HEADERS['VIEWPLAN'] == 'ext/occ4d_viewplan.h'


@pytest.mark.parametrize('counts', vc.GRIDS, ids=vc.GRID_IDS)
def test_matrix_equals_the_restatement_and_the_twin_twice(twin_handle, counts):
    calls, live_inside, dead_solid = vc.check_grid(counts, DEV, twin_handle)
    assert calls == len(vc.FIELDS) * 12 * 2
    if counts == (3, 2, 5):
        assert live_inside >= 6 and dead_solid >= 6


def test_greedy_by_hand(twin_handle):
    vc.check_greedy_by_hand(DEV, pk._lib.lib())
    vc.check_greedy_by_hand('cpu', twin_handle)


def test_wall_by_hand():
    vc.check_wall_by_hand(DEV)


def test_consequences_of_the_rules():
    vc.check_consequences(DEV)


def test_raw_calls_write_nothing_else(twin_handle):
    vc.check_raw_canaries(DEV, pk._lib.lib())
    vc.check_raw_canaries('cpu', twin_handle)


def test_argument_errors():
    vc.check_argument_errors(DEV)


def test_plan_equals_the_restatement():
    vc.check_plan(DEV)


def test_perform_inference_with_next_view(shared, monkeypatch):
    vc.check_end_to_end(shared, monkeypatch)


def test_evaluate_clip_appends_the_plans(shared):
    vc.check_clip(shared)


def test_none_is_untouched(shared, monkeypatch):
    vc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared):
    vc.check_value_errors(shared)
