"""The object layers in camera views (include/ext/occ4d_layers.h, ops.grid_layers, projection.ObjectLayers / object_layers and the
helpers layer_depth, amodal_mask, visible_mask, occlusion_rate, occlusion_pairs, perform_inference(layers=...)) through the g++ twin,
without a GPU: the header and its binding, the case matrix of tests/layers_cases.py against the restatement of the header, which
walks every sample, the consequences of the rules on what the library returns, five slabs worked by hand, the raw entry point inside
canaries, the option object, and perform_inference / evaluate_clip on the refine fixture -- everything EQUAL, no tolerance.  The twin
and the HIP kernel share the owner of a sample, the find-or-open step, the march and the argument contract (csrc/layers_math.hpp),
but neither the order of the pixels nor the reduction into the table.  tests/test_gpu_layers.py runs the same comparisons on the
device."""
import ctypes

import pytest
import torch

import layers_cases as lc
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


def test_symbol_is_in_the_open_table_and_in_no_other():
    """ADDON_HEADERS is open by design: this header's symbol is IN it -- the table is never compared with it."""
    lib = pk._lib
    assert lib.ADDON_HEADERS['LAYERS'] == 'ext/occ4d_layers.h'
    for table in (lib.FEATURE_HEADERS, lib.EXTENSION_HEADERS, lib.STRUCT_EXTENSION_HEADERS):
        assert 'LAYERS' not in table
    with open(lib.LAYERS_HEADER_PATH) as f:
        text = f.read()
    assert lib.LAYERS_SIGNATURES == lib.parse_prototypes(text, lib._STRUCTS) and sorted(lib.LAYERS_SIGNATURES) == sorted(lc.SYMBOLS)
    for name in lc.SYMBOLS:
        assert lib.ADDON_SIGNATURES[name] == lib.LAYERS_SIGNATURES[name]
        for other in (lib.SIGNATURES, lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
            assert name not in other
    assert lib.LAYERS_CONSTANTS == lc.CONSTANTS and lib.ABI_VERSION == 5
    I, P, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    assert lib.LAYERS_SIGNATURES['occ4d_layers_march_i32'] == (I, [P, I, I, I, I, F, F, F, F, F, F, P, P, I, I, I, F, F, I, I] + [P] * 8)
    for phrase in ('THE RULES', 'OWNER', 'LAYERS', 'PER-PIXEL OUTPUTS', 'TABLE', 'STATUS', 'CONTRACT', 'SHORTCUT', 'LAUNCHES', 'ACCESS SAFETY',
                   'occ4d_raycast.h', 'floorf(g_a + 0.5f)', 'never ends early on overflow', 'lower bounds', 'touches no pointer'):
        assert phrase in text, phrase


def test_twin_exports_and_binds_the_prototype(twin):
    lib = pk._lib.lib()
    handle = ctypes.CDLL(pk.cpu_twin.LIB)
    for name, (res, args) in pk._lib.LAYERS_SIGNATURES.items():
        assert hasattr(handle, name), name
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_package_exports():
    for name in ('ObjectLayers', 'object_layers', 'layer_depth', 'amodal_mask', 'visible_mask', 'occlusion_rate', 'occlusion_pairs'):
        assert hasattr(pk.projection, name), name
    assert hasattr(pk.ops, 'grid_layers')


def test_the_math_header_calls_the_ray_casts_functions():
    """csrc/layers_math.hpp includes csrc/raycast_math.hpp and calls its ray, depth, coordinate and IN test; it restates none."""
    with open(pk._lib.LIB_PATH.replace('libocc4d.so', 'csrc/layers_math.hpp')) as f:
        text = f.read()
    assert '#include "raycast_math.hpp"' in text
    for call in ('ry::ray_point(', 'ry::grid_coord(', 'ry::in_axis(', 'ry::depth_of('):
        assert call in text, call
    assert 'row4' not in text and '- 0.5f' not in text


@pytest.mark.parametrize('counts', lc.GRIDS, ids=lc.GRID_IDS)
def test_matrix_equals_the_restatement_twice(twin, counts):
    assert lc.check_matrix(counts, CPU) == len(lc.matrix_cells(counts))


def test_the_matrix_covers_every_value():
    cells = lc.matrix_cells((12, 7, 9))
    assert {c[0] for c in cells} == set(lc.IMAGES) and {len(c[1]) for c in cells} >= set(lc.VIEW_COUNTS)
    assert {p for c in cells for p in c[1]} == set(lc.PLACEMENTS) and {c[2] for c in cells} == set(lc.STEP_COUNTS)
    assert {c[3] for c in cells} == set(lc.LAYER_COUNTS) and {c[4] for c in cells} == set(lc.LABEL_KINDS)
    assert {c[5] for c in cells} == set(lc.OUTPUT_SETS)


def test_more_objects_than_gather_slots(twin):
    lc.check_more_objects_than_slots(CPU)


def test_slabs_on_the_central_ray(twin):
    lc.check_slabs_on_the_central_ray(CPU)


def test_table_from_the_pixel_arrays(twin):
    lc.check_table_from_pixels(CPU)


def test_prefix(twin):
    lc.check_prefix(CPU)


def test_permutation(twin):
    lc.check_permutation(CPU)


def test_five_slabs_by_hand(twin):
    lc.check_by_hand(CPU)


def test_cameras_that_see_nothing(twin):
    lc.check_nothing_seen(CPU)


def test_argument_errors(twin):
    lc.check_argument_errors(CPU)


def test_option():
    lc.check_option()


def test_signature_positions():
    lc.check_signatures()


def test_perform_inference_with_layers(shared, twin, monkeypatch):
    lc.check_end_to_end(shared, monkeypatch)


def test_evaluate_clip_appends_the_layers(shared, twin):
    lc.check_clip(shared)


def test_none_is_untouched(shared, twin, monkeypatch):
    lc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared, twin):
    lc.check_value_errors(shared)
