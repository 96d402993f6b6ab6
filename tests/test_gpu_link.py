"""The components linked across output frames on the HIP path (csrc/link.hip): the case matrix of tests/link_cases.py through
libocc4d.so, EQUAL to the numpy / Python-integer restatement and to the g++ twin (loaded as a second plain handle: the kernels and
the twin share the insert, the order relation and the item bodies), every case run twice with equal bits, the Tracker over
sequences, and the end-to-end comparisons of tests/test_link_host.py on the device.  Integers only, no tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import link_cases as lc
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
    for name in lc.SYMBOLS:
        assert hasattr(handle, name) and name in pk._lib.ADDON_SIGNATURES, name
    assert pk._lib.ADDON_HEADERS['LINK'] == 'ext/occ4d_link.h'


@pytest.mark.parametrize('name', lc.NAMES)
def test_case_equals_the_restatement_and_the_twin_twice(twin_handle, name):
    got = lc.run(lc.BY_NAME[name], DEV)
    assert lc.same(got, name), name
    again = lc.run(lc.BY_NAME[name], DEV)
    raw = lc.run_raw(twin_handle, lc.BY_NAME[name])
    assert lc.same(raw, name), name
    if lc.expected(name)[1][2]:                       # the table overflowed: the pair rows and two totals are unspecified
        strip = lambda r: (r[0][lc.cap_of(lc.BY_NAME[name]):], r[1][2:], r[2])
        got, again, raw = strip(got), strip(again), strip(raw)
    assert lc.bits(got) == lc.bits(again) == lc.bits(raw), name


def test_argument_errors():
    lc.check_argument_errors(DEV)


def test_tracker_over_sequences():
    lc.check_tracker(DEV)


def test_perform_inference_with_a_tracker(shared):
    lc.check_end_to_end(shared)


def test_evaluate_clip_passes_the_tracker_through(shared):
    lc.check_clip(shared)


def test_tracker_none_is_untouched(shared, monkeypatch):
    lc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared):
    lc.check_value_errors(shared)
