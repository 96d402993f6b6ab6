"""The connected components of the grid's solid set (include/ext/occ4d_components.h, components.py, inference.perform_inference(
components=...)) through the g++ twin, without a GPU: the header and its binding, the entry points against the breadth-first-search
restatement over the case matrix of tests/components_cases.py (and scipy.ndimage.label where scipy is there), the rejected calls,
and perform_inference / evaluate_clip with a Components on the tracking fixture -- everything EQUAL, no tolerance.  The twin and the
HIP kernels share find, unite and the item bodies (csrc/components_math.hpp); tests/test_gpu_components.py runs the same comparisons
on the device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import components_cases as cc
import refine_cases as rc
import occlusions4d_amd as pk

CPU = torch.device('cpu')
SYMBOLS = ['occ4d_components_label_f32', 'occ4d_components_table_i64']


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
    assert lib.ADDON_HEADERS['COMPONENTS'] == 'ext/occ4d_components.h'
    for table in (lib.FEATURE_HEADERS, lib.EXTENSION_HEADERS, lib.STRUCT_EXTENSION_HEADERS):
        assert 'COMPONENTS' not in table
    with open(lib.COMPONENTS_HEADER_PATH) as f:
        text = f.read()
    assert lib.COMPONENTS_SIGNATURES == lib.parse_prototypes(text, lib._STRUCTS) and sorted(lib.COMPONENTS_SIGNATURES) == SYMBOLS
    for name in SYMBOLS:
        assert lib.ADDON_SIGNATURES[name] == lib.COMPONENTS_SIGNATURES[name]
        for other in (lib.SIGNATURES, lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
            assert name not in other
    assert lib.COMPONENTS_CONSTANTS == {'COLS': 12, 'TILE': 256, 'TILE_X': 6, 'TILE_Y': 7, 'TILE_Z': 6} and lib.ABI_VERSION == 5
    assert tuple(lib.COMPONENTS_CONSTANTS['TILE_' + a] for a in 'XYZ') == cc.TILE and cc.COLS == 12
    I, L, F, P = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    assert lib.COMPONENTS_SIGNATURES['occ4d_components_label_f32'] == (I, [P, L, F, P, L, F, P, I, I, I, I, I, P, P, P, P])
    assert lib.COMPONENTS_SIGNATURES['occ4d_components_table_i64'] == (I, [P, P, I, I, I, P, P, I, P])
    assert pk.ops.components_work_len(1000) == 3 * 1000 + 3 * 4


def test_twin_exports_and_binds_the_prototypes(twin):
    lib = pk._lib.lib()
    handle = ctypes.CDLL(pk.cpu_twin.LIB)
    for name, (res, args) in pk._lib.COMPONENTS_SIGNATURES.items():
        assert hasattr(handle, name), name
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_restatement_on_cases_worked_by_hand():
    field = np.array([1, 1, 0, 1, 0, 0, 1, 1], np.float32)               # (2, 2, 2): x = 0: [[1, 1], [0, 1]], x = 1: [[0, 0], [1, 1]]
    labels, totals, table = cc.restate(field, (2, 2, 2), 0.5)
    assert labels.tolist() == [0, 0, -1, 0, -1, -1, 0, 0] and totals.tolist() == [1, 5, 1]
    assert table.tolist() == [[5, 0, -1, 2, 3, 3, 0, 0, 0, 1, 1, 1]]
    labels, totals, table = cc.restate(field, (2, 2, 2), 0.5, klass=np.array([0, 1, 0, 1, 0, 0, 1, -1], np.int32))
    assert labels.tolist() == [0, 1, -1, 1, -1, -1, 2, -1] and totals.tolist() == [3, 4, 3]
    assert table[:, :3].tolist() == [[1, 0, 0], [2, 1, 1], [1, 6, 1]]
    labels, totals, table = cc.restate(field, (2, 2, 2), 0.5, klass=np.array([0, 1, 0, 1, 0, 0, 1, -1], np.int32), min_size=2)
    assert labels.tolist() == [-1, 0, -1, 0, -1, -1, -1, -1] and totals.tolist() == [1, 2, 3] and table[:, 1].tolist() == [1]
    cc.check_expectations_by_hand()


@pytest.mark.parametrize('name', cc.NAMES)
def test_case_equals_the_restatement(twin, name):
    cc.check(name, CPU)


def test_restatement_equals_scipy_where_both_apply():
    """No classes, min_size 1: the numbering is scipy.ndimage.label's minus one, at all three connectivities."""
    ndimage = pytest.importorskip('scipy.ndimage')
    assert len(cc.SCIPY_NAMES) > 80
    for name in cc.SCIPY_NAMES:
        labels, count = cc.scipy_labels(name, ndimage)
        assert np.array_equal(cc.expected(name)[0], labels) and cc.expected(name)[1][0] == count, name


def test_argument_errors(twin):
    cc.check_argument_errors(CPU)


def test_option_object_and_host_summary():
    c = pk.components.Components()
    assert (c.level, c.connectivity, c.select, c.by_class, c.min_size) == (None, 6, None, False, 1) and c.resolve(0.25) == 0.25
    assert pk.components.Components(level=0.7).resolve(0.25) == 0.7 and 'connectivity=18' in repr(pk.components.Components(connectivity=18))
    for kw, text in ((dict(level=cc.NAN), 'NaN'), (dict(connectivity=8), 'connectivity = 8 must be 6, 18 or 26'),
                     (dict(min_size=0), 'min_size = 0'), (dict(min_size=1.5), 'min_size = 1.5'), (dict(connectivity=True), 'connectivity')):
        with pytest.raises(ValueError, match=text):
            pk.components.Components(**kw)
    with pytest.raises(ValueError, match='NaN'):
        c.resolve(cc.NAN)
    table = np.array([[4, 0, -1, 2, 6, 10, 0, 1, 2, 1, 2, 3], [1, 9, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3]], np.int64)
    got = pk.components.boxes_and_centroids(table, (1.0, -2.0, 0.0), (0.5, 0.25, 2.0))
    assert got['size'].tolist() == [4, 1] and got['klass'].tolist() == [-1, 2] and got['centroid'].dtype == np.float64
    assert got['centroid'].tolist() == [[1.5, -1.5, 6.0], [2.75, -1.125, 7.0]]
    assert got['box_min'].tolist() == [[1.25, -1.625, 5.0], [2.75, -1.125, 7.0]]
    assert got['box_max'].tolist() == [[1.75, -1.375, 7.0], [2.75, -1.125, 7.0]]
    sig = inspect.signature(pk.inference.perform_inference).parameters
    assert sig['components'].default is None
    sig = inspect.signature(pk.evaluation.evaluate_clip).parameters
    assert sig['components'].default is None and sig['objects'].default is None
    assert 'components' in pk.__all__


def test_semantic_class_is_the_first_maximum():
    out = torch.tensor([[0.9, 0.1, 0.7, 0.7], [0.2, 0.5, 0.1, 0.5], [0.3, 0.0, 0.0, 0.0]])
    assert pk.components.semantic_class(out, 1, 3).tolist() == [1, 0, 0] and pk.components.semantic_class(out, 1, 3).dtype == torch.int32


def test_perform_inference_with_components(twin, shared):
    cc.check_end_to_end(shared)


def test_evaluate_clip_passes_components_through(twin, shared):
    cc.check_clip(shared)


def test_components_none_is_untouched(twin, shared, monkeypatch):
    cc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(twin, shared):
    cc.check_value_errors(shared)


def test_by_class_on_the_case_that_predicts_segmentation(twin):
    cc.check_by_class(CPU)
