"""The watershed segments of the decoded occupancy (include/ext/occ4d_watershed.h, watershed.py, inference.perform_inference(
segments=...)) through the g++ twin, without a GPU: the header and its binding, the restatement on cases worked by hand, the entry
points against it over the case matrix of tests/watershed_cases.py, the consequences of the rules against yardsticks of their own
(ops.grid_components, scipy.ndimage.label where it is installed), the option object, and perform_inference / evaluate_clip with
Segments on the tracking fixture -- everything EQUAL, no tolerance.  The twin and the HIP kernels share ORDER, the ascent choice, the
MERGE test and the item bodies (csrc/watershed_math.hpp), but not the tiling: the twin goes over the whole grid as one tile.
tests/test_gpu_watershed.py runs the same comparisons on the device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import refine_cases as rc
import watershed_cases as wc
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
    assert lib.ADDON_HEADERS['WATERSHED'] == 'ext/occ4d_watershed.h'
    for table in (lib.FEATURE_HEADERS, lib.EXTENSION_HEADERS, lib.STRUCT_EXTENSION_HEADERS):
        assert 'WATERSHED' not in table
    with open(lib.WATERSHED_HEADER_PATH) as f:
        text = f.read()
    assert lib.WATERSHED_SIGNATURES == lib.parse_prototypes(text, lib._STRUCTS) and sorted(lib.WATERSHED_SIGNATURES) == wc.SYMBOLS
    for name in wc.SYMBOLS:
        assert lib.ADDON_SIGNATURES[name] == lib.WATERSHED_SIGNATURES[name]
        for other in (lib.SIGNATURES, lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
            assert name not in other
    k = lib.WATERSHED_CONSTANTS
    assert k == dict(TILE=256, TILE_X=8, TILE_Y=8, TILE_Z=8, HOPS=8, ROUND_WORDS=12, TOTALS=4) and k['TILE'] == lib.COMPONENTS_CONSTANTS['TILE']
    assert lib.ABI_VERSION == 5
    I, P = ctypes.c_int, ctypes.c_void_p
    assert lib.WATERSHED_SIGNATURES['occ4d_watershed_label_i32'] == (I, [P, I, I, I, I, I, I, P, P, P, P])
    assert lib.WATERSHED_SIGNATURES['occ4d_watershed_peaks_i32'] == (I, [P, P, I, P, P, I, P])
    # the work array: O(n) int32 and an O(n / 256) tile term
    assert pk.ops.watershed_work_len(0) == 12 and pk.ops.watershed_work_len(1) == 4 + 4 + 12 and pk.ops.watershed_work_len(257) == 4 * 257 + 8 + 12
    assert pk.ops.watershed_work_len(96 * 96 * 58) == 4 * 534528 + 4 * 2088 + 12


def test_twin_exports_and_binds_the_prototypes(twin):
    lib = pk._lib.lib()
    handle = ctypes.CDLL(pk.cpu_twin.LIB)
    for name, (res, args) in pk._lib.WATERSHED_SIGNATURES.items():
        assert hasattr(handle, name), name
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_restatement_on_cases_worked_by_hand():
    wc.check_by_hand()


@pytest.mark.parametrize('name', wc.NAMES)
def test_case_equals_the_restatement_twice(twin, name):
    wc.check(name, CPU)


@pytest.mark.parametrize('name', wc.NAMES)
def test_consequences_of_the_rules(twin, name):
    wc.check_consequences(name, CPU)


def test_two_touching_balls_flip_where_the_restatement_says(twin):
    wc.check_balls(CPU)


def test_caps_and_untouched_rows(twin):
    wc.check_caps(CPU, pk._lib.lib())


def test_argument_errors(twin):
    wc.check_argument_errors(CPU)


def test_option_object_and_signatures():
    s = pk.watershed.Segments(4)
    assert (s.h, s.level, s.select, s.weights, s.connectivity, s.min_size) == (4, None, None, (1, 1, 1), 26, 1)
    assert (s.keyword, s.clip_list[0], s.needs, s.into) == ('segments', 'parts', None, None) and isinstance(s, pk.products.LevelProduct)
    s = pk.watershed.Segments(h=np.int64(0), level=0.25, select=(3, 0.5), weights=[1, np.int32(2), 3], connectivity=6, min_size=np.int32(7))
    assert (s.h, s.level, s.select, s.weights, s.connectivity, s.min_size) == (0, 0.25, (3, 0.5), (1, 2, 3), 6, 7)
    assert repr(s) == 'Segments(h=0, level=0.25, select=(3, 0.5), weights=(1, 2, 3), connectivity=6, min_size=7)'
    assert pk.watershed.Segments(2 ** 31 - 1).h == 2 ** 31 - 1 and s.resolve(0.5) == 0.25 and pk.watershed.Segments(1).resolve(0.5) == 0.5
    with pytest.raises(TypeError):
        pk.watershed.Segments()                                            # h has no default
    for kw, text in ((dict(h=-1), r'h = -1 must be an integer in \[0, 2\^31 - 1\]'), (dict(h=2 ** 31), 'h = 2147483648 must be'),
                     (dict(h=1.0), 'h = 1.0 must be'), (dict(h=True), 'h = True must be'), (dict(h=None), 'h = None must be'),
                     (dict(h=1, level=float('nan')), 'level is NaN'), (dict(h=1, connectivity=8), 'connectivity = 8 must be 6, 18 or 26'),
                     (dict(h=1, connectivity=True), 'connectivity'), (dict(h=1, min_size=0), 'min_size = 0 must be an integer >= 1'),
                     (dict(h=1, min_size=2.0), 'min_size'), (dict(h=1, weights=(1, 0, 1)), 'weights = .* must be three integers >= 1'),
                     (dict(h=1, weights=(1, 1)), 'three integers'), (dict(h=1, select=5), 'select = 5 must be')):
        with pytest.raises(ValueError, match=text):
            pk.watershed.Segments(**kw)
    out = torch.zeros((8, 2))
    for kw, text in ((dict(h=-1), 'h = -1'), (dict(h=0, connectivity=7), 'connectivity = 7'), (dict(h=0, min_size=0), 'min_size = 0'),
                     (dict(h=0, weights=(1, 2)), 'three integers'), (dict(h=0, level=float('nan')), 'level is NaN')):
        with pytest.raises(ValueError, match=text):
            pk.watershed.split(out, (2, 2, 2), **dict(dict(level=0.5), **kw))
    sig = inspect.signature(pk.inference.perform_inference).parameters
    names = list(sig)
    assert sig['segments'].default is None and names[-2:] == ['tracker', 'clearance'] and names.index('segments') == len(names) - 3
    sig = inspect.signature(pk.evaluation.evaluate_clip).parameters
    assert sig['segments'].default is None and sig['parts'].default is None and list(sig)[-4:] == ['segments', 'parts', 'route', 'routes']
    assert 'watershed' in pk.__all__ and 'measured on a trained model' in ' '.join(pk.watershed.Segments.__doc__.split())


def test_split_is_distance_then_watershed(twin):
    """watershed.split on a dense output: the depth of column 0 >= level under the mask column, then the rules."""
    rng = np.random.default_rng(5)
    counts = (9, 10, 11)
    out = torch.from_numpy(rng.random((990, 3)).astype(np.float32))
    labels, table, peaks = pk.watershed.split(out, counts, 0.3, 1, select=(2, 0.2), connectivity=18, min_size=2, channel=1)
    member = (out[:, 1].numpy() >= np.float32(0.3)) & (out[:, 2].numpy() >= np.float32(0.2))
    want = wc.restate(wc.depth2(member, counts), counts, 18, 1, 2)
    assert np.array_equal(labels.numpy(), want['labels']) and np.array_equal(table.numpy(), want['table']) and np.array_equal(peaks.numpy(), want['peaks'])
    # weights: the depth in weighted steps
    labels, table, peaks = pk.watershed.split(out, counts, 0.3, 3, weights=(1, 4, 9))
    inside2 = pk.ops.grid_distance(out[:, 0], counts, 0.3, (1, 4, 9), 1)[0]
    want = wc.restate(inside2.numpy(), counts, 26, 3)
    assert np.array_equal(labels.numpy(), want['labels']) and np.array_equal(peaks.numpy(), want['peaks'])


def test_compositions_with_components_distance_and_tracker(twin):
    wc.check_compositions(CPU)


def test_perform_inference_with_segments(twin, shared):
    wc.check_end_to_end(shared)


def test_evaluate_clip_passes_segments_through(twin, shared):
    wc.check_clip(shared)


def test_segments_none_is_untouched(twin, shared, monkeypatch):
    wc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(twin, shared):
    wc.check_value_errors(shared)
