"""The oriented boxes on the HIP path (csrc/boxes.hip): the cases of tests/boxes_cases.py through libocc4d.so, EQUAL to the
restatement of the header's rules and to the g++ twin bit for bit (the twin loaded as a second plain handle: the kernels and the twin
share the DEAD test, the projections and the keys; the reduce kernel walks runs of labels with the directions across its lanes,
gathers per workgroup in LDS and finishes with integer atomics, the twin takes the points in order), every call twice with equal
bits, and the consequences and the end-to-end comparisons of tests/test_boxes_host.py on the device.  Integers only, no tolerance;
the largest grids are 96 x 96 x 2 and 2048 x 2 x 1."""
import ctypes

import pytest
import torch

import boxes_cases as bc
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
    for name in bc.SYMBOLS:
        assert hasattr(handle, name) and name in pk._lib.ADDON_SIGNATURES, name
    assert pk._lib.ADDON_HEADERS['BOXES'] == 'ext/occ4d_boxes.h'


@pytest.mark.parametrize('counts', bc.GRIDS, ids=bc.GRID_IDS)
def test_matrix_equals_the_restatement_and_the_twin_twice(twin_handle, counts):
    assert bc.check_grid(counts, DEV, twin_handle) == len(bc.LABEL_KINDS) * len(bc.A_VALUES)


def test_more_objects_than_gather_slots(twin_handle):
    bc.check_columns(DEV, twin_handle)


def test_coefficients_at_the_int32_edge(twin_handle):
    bc.check_int32_edge(DEV, twin_handle)


def test_columns_longer_than_one_load(twin_handle):
    bc.check_tall(DEV, twin_handle)


def test_choice_by_hand():
    bc.check_choice_by_hand(DEV)


def test_rotated_rectangles(twin_handle):
    bc.check_rectangles(DEV, twin_handle)


def test_consequences_of_the_rules():
    bc.check_consequences(DEV)


def test_argument_errors():
    bc.check_argument_errors(DEV)


def test_perform_inference_with_boxes(shared, monkeypatch):
    bc.check_end_to_end(shared, monkeypatch)


def test_evaluate_clip_joins_the_boxes(shared):
    bc.check_clip(shared)


def test_none_is_untouched(shared, monkeypatch):
    bc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared):
    bc.check_value_errors(shared)
