"""The connected components of the grid's solid set on the HIP path (csrc/components.hip): the case matrix of
tests/components_cases.py through libocc4d.so, EQUAL to the breadth-first-search restatement and to the g++ twin (loaded as a second
plain handle: the kernels and the twin share find, unite and the item bodies), results that do not depend on the run, and the
end-to-end comparisons of tests/test_components_host.py on the device.  Integers only, no tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import components_cases as cc
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
    for name in cc.SYMBOLS:
        assert hasattr(handle, name) and name in pk._lib.ADDON_SIGNATURES, name
    assert pk._lib.ADDON_HEADERS['COMPONENTS'] == 'ext/occ4d_components.h'


@pytest.mark.parametrize('name', cc.NAMES)
def test_case_equals_the_restatement_and_the_twin(twin_handle, name):
    got = cc.run(cc.BY_NAME[name], DEV)
    assert cc.same(got, name), name
    labels, totals, table = cc.run_raw(twin_handle, cc.BY_NAME[name])
    rows = len(table) if cc.BY_NAME[name]['cap'] is None else min(cc.BY_NAME[name]['cap'], len(table))
    assert np.array_equal(got[0], labels) and np.array_equal(got[1], totals) and np.array_equal(got[2][:rows], table[:rows]), name


def test_does_not_depend_on_the_run():
    """Three runs of every random case of the (40, 24, 20) grid: labels, totals and table equal bit for bit (the links only ever go
    to a lower index of the same component, the table adds integers)."""
    assert len(cc.RANDOM_BIG) == 9 + 3
    for name in cc.RANDOM_BIG:
        runs = [cc.run(cc.BY_NAME[name], DEV) for _ in range(3)]
        for got in runs:
            assert cc.same(got, name), name
            for a, b in zip(got[:3], runs[0][:3]):
                assert a.tobytes() == b.tobytes(), name


def test_argument_errors():
    cc.check_argument_errors(DEV)


def test_perform_inference_with_components(shared):
    cc.check_end_to_end(shared)


def test_evaluate_clip_passes_components_through(shared):
    cc.check_clip(shared)


def test_components_none_is_untouched(shared, monkeypatch):
    cc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared):
    cc.check_value_errors(shared)


def test_by_class_on_the_case_that_predicts_segmentation():
    cc.check_by_class(DEV)
