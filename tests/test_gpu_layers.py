"""The object layers on the HIP path (csrc/layers.hip): the cases of tests/layers_cases.py through libocc4d.so, EQUAL to the
restatement of the header's rules, which walks every sample, and to the g++ twin bit for bit (the twin loaded as a second plain
handle: the kernel and the twin share the owner of a sample, the find-or-open step and the march; the kernel keeps a lane's layers in
registers, matches labels across the lanes of a wave, gathers per workgroup in LDS and finishes with integer atomics, the twin takes
the pixels in order), every call twice with equal bits, and the consequences and the end-to-end comparisons of
tests/test_layers_host.py on the device.  Integers only, no tolerance; the largest case is 3 views of 20 x 33 pixels over 64
samples."""
import ctypes

import pytest
import torch

import layers_cases as lc
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
    for name in lc.SYMBOLS:
        assert hasattr(handle, name) and name in pk._lib.ADDON_SIGNATURES, name
    assert pk._lib.ADDON_HEADERS['LAYERS'] == 'ext/occ4d_layers.h'


@pytest.mark.parametrize('counts', lc.GRIDS, ids=lc.GRID_IDS)
def test_matrix_equals_the_restatement_and_the_twin_twice(twin_handle, counts):
    assert lc.check_matrix(counts, DEV, twin_handle) == len(lc.matrix_cells(counts))


def test_more_objects_than_gather_slots(twin_handle):
    lc.check_more_objects_than_slots(DEV, twin_handle)


def test_slabs_on_the_central_ray():
    lc.check_slabs_on_the_central_ray(DEV)


def test_table_from_the_pixel_arrays():
    lc.check_table_from_pixels(DEV)


def test_prefix():
    lc.check_prefix(DEV)


def test_permutation():
    lc.check_permutation(DEV)


def test_five_slabs_by_hand():
    lc.check_by_hand(DEV)


def test_cameras_that_see_nothing():
    lc.check_nothing_seen(DEV)


def test_argument_errors():
    lc.check_argument_errors(DEV)


def test_perform_inference_with_layers(shared, monkeypatch):
    lc.check_end_to_end(shared, monkeypatch)


def test_evaluate_clip_appends_the_layers(shared):
    lc.check_clip(shared)


def test_none_is_untouched(shared, monkeypatch):
    lc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared):
    lc.check_value_errors(shared)
