"""The oriented boxes of the labelled objects (include/ext/occ4d_boxes.h, ops.grid_box_extents / boxes_choose, components.Boxes /
yaw_directions / oriented_boxes / tracks, perform_inference(boxes=...)) through the g++ twin, without a GPU: the header and its
binding, the case matrix of tests/boxes_cases.py against the restatement of the header, the choice worked by hand, rotated
rectangles, the consequences of the rules on what the library returns, the raw entry points inside canaries, the option object, and
perform_inference / evaluate_clip on the refine fixture -- everything EQUAL, no tolerance.  The twin and the HIP kernels share the
DEAD test, the projections, the keys and the argument contracts (csrc/boxes_math.hpp), but neither the order of the work nor the
reductions.  tests/test_gpu_boxes.py runs the same comparisons on the device."""
import ctypes

import pytest
import torch

import boxes_cases as bc
import refine_cases as rc
import occlusions4d_amd as pk

CPU = torch.device('cpu')


@pytest.fixture
def twin():
    pk.cpu_twin.enable()
    try:
        yield pk
    finally:
        pk.cpu_twin.disable()


@pytest.fixture(scope='module')
def shared():
    pk.cpu_twin.enable()
    try:
        return rc.Shared(CPU)
    finally:
        pk.cpu_twin.disable()


def test_symbols_are_in_the_open_table_and_in_no_other():
    """ADDON_HEADERS is open by design: this header's symbols are IN it -- the table is never compared with them."""
    lib = pk._lib
    assert lib.ADDON_HEADERS['BOXES'] == 'ext/occ4d_boxes.h'
    for table in (lib.FEATURE_HEADERS, lib.EXTENSION_HEADERS, lib.STRUCT_EXTENSION_HEADERS):
        assert 'BOXES' not in table
    with open(lib.BOXES_HEADER_PATH) as f:
        text = f.read()
    assert lib.BOXES_SIGNATURES == lib.parse_prototypes(text, lib._STRUCTS) and sorted(lib.BOXES_SIGNATURES) == sorted(bc.SYMBOLS)
    for name in bc.SYMBOLS:
        assert lib.ADDON_SIGNATURES[name] == lib.BOXES_SIGNATURES[name]
        for other in (lib.SIGNATURES, lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
            assert name not in other
    assert lib.BOXES_CONSTANTS == bc.CONSTANTS and lib.ABI_VERSION == 5
    I, P = ctypes.c_int, ctypes.c_void_p
    assert lib.BOXES_SIGNATURES['occ4d_boxes_extents_i32'] == (I, [P, I, I, I, I, P, I, P, P, P])
    assert lib.BOXES_SIGNATURES['occ4d_boxes_choose_i32'] == (I, [P, P, P, I, I, P, P])
    for phrase in ('THE RULES', 'DEAD', 'EMPTY', 'THE LOWEST a', 'LAUNCHES', 'ACCESS SAFETY', 'GRID', 'OBJECTS', 'DIRECTIONS', 'EXTENTS',
                   'RANGE', 'CHOICE', 'before a coefficient is used', 'Nothing read from them becomes an index'):
        assert phrase in text, phrase


def test_twin_exports_and_binds_the_prototypes(twin):
    lib = pk._lib.lib()
    handle = ctypes.CDLL(pk.cpu_twin.LIB)
    for name, (res, args) in pk._lib.BOXES_SIGNATURES.items():
        assert hasattr(handle, name), name
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_package_exports():
    for name in ('Boxes', 'yaw_directions', 'oriented_boxes', 'tracks', 'boxes_and_centroids'):
        assert hasattr(pk.components, name), name
    for name in bc.OPS:
        assert hasattr(pk.ops, name), name


@pytest.mark.parametrize('counts', bc.GRIDS, ids=bc.GRID_IDS)
def test_matrix_equals_the_restatement_twice(twin, counts):
    assert bc.check_grid(counts, CPU) == len(bc.LABEL_KINDS) * len(bc.A_VALUES)


def test_more_objects_than_gather_slots(twin):
    bc.check_columns(CPU)


def test_coefficients_at_the_int32_edge(twin):
    bc.check_int32_edge(CPU)


def test_columns_longer_than_one_load(twin):
    bc.check_tall(CPU)


def test_choice_by_hand(twin):
    bc.check_choice_by_hand(CPU)


def test_rotated_rectangles(twin):
    bc.check_rectangles(CPU)


def test_consequences_of_the_rules(twin):
    bc.check_consequences(CPU)


def test_argument_errors(twin):
    bc.check_argument_errors(CPU)


def test_yaw_directions():
    bc.check_yaw_directions()


def test_oriented_boxes_by_hand():
    bc.check_oriented_boxes()


def test_tracks_by_hand():
    bc.check_tracks_by_hand()


def test_option():
    bc.check_option()


def test_signature_positions():
    bc.check_signatures()


def test_perform_inference_with_boxes(shared, twin, monkeypatch):
    bc.check_end_to_end(shared, monkeypatch)


def test_evaluate_clip_joins_the_boxes(shared, twin):
    bc.check_clip(shared)


def test_none_is_untouched(shared, twin, monkeypatch):
    bc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared, twin):
    bc.check_value_errors(shared)
