"""The distance transform of the grid's solid set on the HIP path (csrc/distance.hip): the case matrix of tests/distance_cases.py
through libocc4d.so, EQUAL to the restatements and to the g++ twin (loaded as a second plain handle: the kernel and the twin share the
order relation and the item bodies, the twin goes line by line and the kernel tile by tile), each case run twice with equal bytes,
and the end-to-end comparisons of tests/test_distance_host.py on the device.  Integers only, no tolerance anywhere."""
import ctypes

import pytest
import torch

import distance_cases as dc
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


def test_hip_library_exports_the_symbol():
    handle = ctypes.CDLL(pk._lib.LIB_PATH)
    for name in dc.SYMBOLS:
        assert hasattr(handle, name) and name in pk._lib.ADDON_SIGNATURES, name
    assert pk._lib.ADDON_HEADERS['DISTANCE'] == 'ext/occ4d_distance.h'


@pytest.mark.parametrize('name', dc.NAMES)
def test_case_equals_the_restatements_and_the_twin(twin_handle, name):
    got = dc.run(dc.BY_NAME[name], DEV)
    assert dc.same(got, name), name
    again = dc.run(dc.BY_NAME[name], DEV)
    on_twin = dc.run_raw(twin_handle, dc.BY_NAME[name])
    for a, b, c in zip(got, again, on_twin):
        assert (a is None and b is None and c is None) or a.tobytes() == b.tobytes() == c.tobytes(), name


def test_argument_errors():
    dc.check_argument_errors(DEV)


def test_perform_inference_with_clearance(shared):
    dc.check_end_to_end(shared)


def test_evaluate_clip_passes_clearance_through(shared):
    dc.check_clip(shared)


def test_clearance_none_is_untouched(shared, monkeypatch):
    dc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared):
    dc.check_value_errors(shared)
