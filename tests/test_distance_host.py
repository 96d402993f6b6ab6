"""The distance transform of the grid's solid set (include/ext/occ4d_distance.h, distance.py, inference.perform_inference(
clearance=...)) through the g++ twin, without a GPU: the header and its binding, the entry point against the two restatements over
the case matrix of tests/distance_cases.py (and scipy.ndimage.distance_transform_edt where scipy is there), the rejected calls, the
option object and the host helpers against numpy, and perform_inference / evaluate_clip with a Clearance on the tracking fixture --
everything EQUAL, no tolerance.  The twin and the HIP kernel share the site test, the order relation and the item bodies
(csrc/distance_math.hpp), but not the tiling: the twin goes line by line.  tests/test_gpu_distance.py runs the same comparisons on
the device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import distance_cases as dc
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
    """ADDON_HEADERS is open by design: this header's symbol is IN it -- the table is never compared with it."""
    lib = pk._lib
    assert lib.ADDON_HEADERS['DISTANCE'] == 'ext/occ4d_distance.h'
    for table in (lib.FEATURE_HEADERS, lib.EXTENSION_HEADERS, lib.STRUCT_EXTENSION_HEADERS):
        assert 'DISTANCE' not in table
    with open(lib.DISTANCE_HEADER_PATH) as f:
        text = f.read()
    assert lib.DISTANCE_SIGNATURES == lib.parse_prototypes(text, lib._STRUCTS) and sorted(lib.DISTANCE_SIGNATURES) == dc.SYMBOLS
    for name in dc.SYMBOLS:
        assert lib.ADDON_SIGNATURES[name] == lib.DISTANCE_SIGNATURES[name]
        for other in (lib.SIGNATURES, lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
            assert name not in other
    assert lib.DISTANCE_CONSTANTS['NONE'] == dc.NONE == 2 ** 31 - 1 == pk.distance.NONE and lib.DISTANCE_CONSTANTS['MAX_AXIS'] == dc.MAX_AXIS == 512
    assert lib.ABI_VERSION == 5
    I, L, F, P = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    assert lib.DISTANCE_SIGNATURES['occ4d_distance_grid_f32'] == (I, [P, L, F, P, L, F, I, I, I, I, I, I, I, P, P, P])
    # the project's lines run at the full width, the longest legal line at a narrower one that still fits the tile
    k = lib.DISTANCE_CONSTANTS
    assert pk.ops.distance_tile_width(96) == k['TILE_WIDTH'] and pk.ops.distance_tile_width(512) * 512 <= k['TILE_POINTS']
    assert pk.ops.distance_tile_width(58, stage=0) == k['RUN_POINTS'] // 58 and pk.ops.distance_tile_width(512, stage=0) >= 1


def test_twin_exports_and_binds_the_prototype(twin):
    lib = pk._lib.lib()
    handle = ctypes.CDLL(pk.cpu_twin.LIB)
    for name, (res, args) in pk._lib.DISTANCE_SIGNATURES.items():
        assert hasattr(handle, name), name
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_restatements_on_cases_worked_by_hand():
    dc.check_by_hand()


def test_the_two_restatements_agree():
    """(a) the staged rule and (b) the global minimum give the same dist2 wherever (b) applies, at both weights."""
    names = [n for n in dc.NAMES if dc.expected_global(n) is not None]
    assert len(names) > 200 and any('w419' in n for n in names)
    for name in names:
        assert np.array_equal(dc.expected(name)[0], dc.expected_global(name)), name


@pytest.mark.parametrize('name', dc.NAMES)
def test_case_equals_the_restatements(twin, name):
    dc.check(name, CPU)


def test_argument_errors(twin):
    dc.check_argument_errors(CPU)


def test_option_object():
    c = pk.distance.Clearance()
    assert (c.level, c.select, c.weights, c.nearest, c.inside) == (None, None, (1, 1, 1), False, False) and c.resolve(0.25) == 0.25
    c = pk.distance.Clearance(level=0.7, select=(3, 0.5), weights=[4, np.int64(1), 9], nearest=1, inside=True)
    assert c.resolve(0.25) == 0.7 and c.select == (3, 0.5) and c.weights == (4, 1, 9) and c.nearest is True and c.inside is True
    assert 'weights=(4, 1, 9)' in repr(c)
    for kw, text in ((dict(level=dc.NAN), 'NaN'), (dict(weights=(1, 0, 1)), r'weights = \(1, 0, 1\) must be three integers >= 1'),
                     (dict(weights=(1, 1)), 'three integers'), (dict(weights=(1.0, 1, 1)), 'three integers'),
                     (dict(weights=(True, 1, 1)), 'three integers'), (dict(weights=(1, -2, 1)), 'three integers'),
                     (dict(weights=(2 ** 31, 1, 1)), 'three integers'), (dict(weights=3), 'three integers')):
        with pytest.raises(ValueError, match=text):
            pk.distance.Clearance(**kw)
    with pytest.raises(ValueError, match='NaN'):
        pk.distance.Clearance().resolve(dc.NAN)
    sig = inspect.signature(pk.inference.perform_inference).parameters
    assert sig['clearance'].default is None and list(sig)[-2:] == ['tracker', 'clearance']
    sig = inspect.signature(pk.evaluation.evaluate_clip).parameters
    assert sig['clearance'].default is None and sig['clearances'].default is None
    assert 'distance' in pk.__all__


def test_metric_signed_and_expand_labels_against_numpy():
    rng = np.random.default_rng(5)
    dist2 = rng.integers(0, 2 ** 31 - 1, 1000).astype(np.int32)
    dist2[:5] = [0, 1, 2, dc.NONE, dc.NONE - 1]
    got = pk.distance.metric(torch.from_numpy(dist2), 0.125)
    want = np.where(dist2 == dc.NONE, np.inf, np.sqrt(dist2.astype(np.float64)) * 0.125).astype(np.float32)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want) and got[3] == np.inf and got[2] == np.float32(np.sqrt(2.0) * 0.125)
    assert np.array_equal(pk.distance.metric(torch.from_numpy(dist2)).numpy(), np.where(dist2 == dc.NONE, np.inf, np.sqrt(dist2.astype(np.float64))).astype(np.float32))
    outside = np.array([4, 0, 0, dc.NONE, 0], np.int32)
    inside = np.array([0, 9, 1, 0, dc.NONE], np.int32)
    got = pk.distance.signed(torch.from_numpy(outside), torch.from_numpy(inside), 0.5)
    assert got.dtype == torch.float32 and got.tolist() == [1.0, -1.5, -0.5, np.inf, -np.inf]
    labels = np.array([-1, 3, -1, 0, 7], np.int32)
    nearest = np.array([1, 1, 4, 3, -1], np.int32)
    got = pk.distance.expand_labels(torch.from_numpy(labels), torch.from_numpy(nearest))
    assert got.dtype == torch.int32 and got.tolist() == [3, 3, 7, 0, -1]
    assert pk.distance.expand_labels(torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)).shape == (0,)
    with pytest.raises(AssertionError):
        pk.distance.metric(torch.zeros(3))
    with pytest.raises(AssertionError):
        pk.distance.expand_labels(torch.from_numpy(labels), torch.from_numpy(nearest[:3]))


def test_transform_is_the_piece(twin):
    """distance.transform on a dense (N, G) array: the density column and the select column read in place."""
    counts = (5, 7, 6)
    rng = np.random.default_rng(9)
    out = rng.random((210, 4), dtype=np.float32)
    got = pk.distance.transform(torch.from_numpy(out), counts, 0.8, select=(2, 0.3), weights=dc.ANISO, nearest=True, inside=True)
    assert sorted(got) == ['dist2', 'inside2', 'nearest']
    kw = dict(mask=np.ascontiguousarray(out[:, 2]), mask_level=0.3)
    dist2, nearest = dc.restate(np.ascontiguousarray(out[:, 0]), counts, 0.8, dc.ANISO, 0, **kw)
    assert np.array_equal(got['dist2'].numpy(), dist2) and np.array_equal(got['nearest'].numpy(), nearest)
    assert np.array_equal(got['inside2'].numpy(), dc.restate(np.ascontiguousarray(out[:, 0]), counts, 0.8, dc.ANISO, 1, **kw)[0])
    assert sorted(pk.distance.transform(torch.from_numpy(out), counts, 0.8)) == ['dist2']
    with pytest.raises(ValueError, match='NaN'):
        pk.distance.transform(torch.from_numpy(out), counts, dc.NAN)
    with pytest.raises(ValueError, match='three integers'):
        pk.distance.transform(torch.from_numpy(out), counts, 0.5, weights=(1, 2.5, 1))


def test_perform_inference_with_clearance(twin, shared):
    dc.check_end_to_end(shared)


def test_evaluate_clip_passes_clearance_through(twin, shared):
    dc.check_clip(shared)


def test_clearance_none_is_untouched(twin, shared, monkeypatch):
    dc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(twin, shared):
    dc.check_value_errors(shared)
