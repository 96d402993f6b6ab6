"""Shortest free-space paths over the grid on the HIP path (csrc/geodesic.hip): the case matrix of tests/geodesic_cases.py through
libocc4d.so, EQUAL to the restatements and to the g++ twin (loaded as a second plain handle: the kernels and the twin share the relax
step and the parent rule, the twin relaxes the whole grid as one tile and the kernel tiles of the header's shape), the larger random
cases run twice with equal bytes, the serpentine that one round cannot finish, the traced paths, and the end-to-end comparisons of
tests/test_geodesic_host.py on the device.  Integers only, no tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import geodesic_cases as gc
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
    for name in gc.SYMBOLS:
        assert hasattr(handle, name) and name in pk._lib.ADDON_SIGNATURES, name
    assert pk._lib.ADDON_HEADERS['GEODESIC'] == 'ext/occ4d_geodesic.h'


@pytest.mark.parametrize('name', gc.CONVERGED)
def test_case_equals_the_restatements_and_the_twin(twin_handle, name):
    """Converged at the default rounds -- asserted --: equal to the restatements, to the twin bit for bit, and to itself run again."""
    c = gc.BY_NAME[name]
    got = gc.run(c, DEV)
    assert gc.same(got, name), name
    on_twin = gc.run_raw(twin_handle, c)
    assert on_twin['status'][0] == 1
    again = gc.run(c, DEV)
    assert again['status'][0] == 1
    for other in (on_twin, again):
        assert other['cost'].tobytes() == got['cost'].tobytes(), name
        assert (got['parent'] is None and other['parent'] is None) or other['parent'].tobytes() == got['parent'].tobytes(), name


def test_serpentine_with_one_round_and_solved():
    gc.check_serpentine(DEV)


@pytest.mark.parametrize('name', gc.TRACED)
def test_traced_paths(name):
    gc.check_trace(name, DEV)


def test_trace_of_the_serpentine():
    gc.check_trace_of_serpentine(DEV)


def test_resume_goes_on_from_the_cost_it_is_given():
    c = gc.BY_NAME['%dx%dx%d-random40-corners-c26' % gc.BIG]
    clear, seeds = torch.from_numpy(c['clear']).to(DEV), torch.from_numpy(c['seeds']).to(DEV)
    cost, status, _ = pk.ops.grid_geodesic(clear, c['counts'], seeds, rounds=1)
    assert status.cpu().tolist() == [0, 1]
    again, status, parent = pk.ops.grid_geodesic(clear, c['counts'], None, parent=True, resume=cost)
    assert again.data_ptr() == cost.data_ptr() and status.cpu()[0] == 1
    assert np.array_equal(again.cpu().numpy(), gc.expected(c['name'])[0]) and np.array_equal(parent.cpu().numpy(), gc.expected(c['name'])[1])


def test_argument_errors():
    gc.check_argument_errors(DEV)


def test_perform_inference_with_route(shared):
    gc.check_end_to_end(shared)


def test_evaluate_clip_passes_route_through(shared):
    gc.check_clip(shared)


def test_route_none_is_untouched(shared, monkeypatch):
    gc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared):
    gc.check_value_errors(shared)
