"""The components linked across output frames (include/ext/occ4d_link.h, components.Tracker, inference.perform_inference(
components=..., tracker=...)) through the g++ twin, without a GPU: the header and its binding, the two entry points against the
numpy / Python-integer restatement over the case matrix of tests/link_cases.py, the rejected calls, the Tracker over sequences, and
perform_inference / evaluate_clip with a tracker on the tracking fixture -- everything EQUAL, no tolerance.  The twin and the HIP
kernels share the insert, the order relation and the item bodies (csrc/link_math.hpp); tests/test_gpu_link.py runs the same
comparisons on the device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import link_cases as lc
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
    lib = pk._lib
    assert lib.ADDON_HEADERS['LINK'] == 'ext/occ4d_link.h'
    for table in (lib.FEATURE_HEADERS, lib.EXTENSION_HEADERS, lib.STRUCT_EXTENSION_HEADERS):
        assert 'LINK' not in table
    with open(lib.LINK_HEADER_PATH) as f:
        text = f.read()
    assert lib.LINK_SIGNATURES == lib.parse_prototypes(text, lib._STRUCTS) and sorted(lib.LINK_SIGNATURES) == lc.SYMBOLS
    for name in lc.SYMBOLS:
        assert lib.ADDON_SIGNATURES[name] == lib.LINK_SIGNATURES[name]
        for other in (lib.SIGNATURES, lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES, lib.COMPONENTS_SIGNATURES):
            assert name not in other
    assert lib.LINK_CONSTANTS == {'PAIR_COLS': 4, 'TILE': lc.TILE, 'MIN_SLOTS': lc.MIN_SLOTS, 'MAX_DEN': 2 ** 20} and lib.ABI_VERSION == 5
    I, L, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert lib.LINK_SIGNATURES['occ4d_link_overlap_i32'] == (I, [P, P, I, I, L, P, P, I, P, P])
    assert lib.LINK_SIGNATURES['occ4d_link_match_i32'] == (I, [P, P, I, P, L, P, L, I, I, P, I, I, P, P, P, P, P])
    for n, cap in ((1000, 100), (19200, 19200), (5, 10 ** 6), (0, 0), (534528, 534528)):
        assert pk.ops.link_work_len(n, cap) == lc.work_len(n, cap)
    assert lc.slots_for(19200, 19200) == 65536 and lc.slots_for(100, 0) == 64


def test_twin_exports_and_binds_the_prototypes(twin):
    lib = pk._lib.lib()
    handle = ctypes.CDLL(pk.cpu_twin.LIB)
    for name, (res, args) in pk._lib.LINK_SIGNATURES.items():
        assert hasattr(handle, name), name
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_restatement_on_cases_worked_by_hand():
    # two a overlap one b with equal IoU (2 / 4 each): the lower a wins, and 1 / 2 is met exactly: count * den == num * union
    la, lb = np.array([0, 0, 1, 1, -1, 2]), np.array([0, 0, 0, 0, 1, -1])
    pairs, members = lc.restate_overlap(la, lb, 3, 2)
    assert pairs.tolist() == [[0, 0, 2, 0], [1, 0, 2, 2]] and members == 4
    size_a, size_b, track_a = [2, 2, 1], [4, 1], [7, 8, 9]
    link, best_a, nxt = lc.restate_match(pairs, size_a, size_b, track_a, 20, 1, 2)
    assert link.tolist() == [[7, 0, 0, 2], [20, -1, -1, 0]] and best_a.tolist() == [[0, 2], [0, 2], [-1, 0]] and nxt == 21
    link, best_a, nxt = lc.restate_match(pairs, size_a, size_b, track_a, 20, 2 ** 19 + 1, 2 ** 20)       # just above 1 / 2: no link
    assert link.tolist() == [[20, -1, 0, 2], [21, -1, -1, 0]] and best_a.tolist() == [[0, 2], [0, 2], [-1, 0]] and nxt == 22
    # the order of the pairs is that of their roots, not of (a, b)
    assert lc.restate_overlap(np.array([1, 0, 1]), np.array([0, 0, 0]), 2, 1)[0].tolist() == [[1, 0, 2, 0], [0, 0, 1, 1]]
    # one a split into two equal b: the lower b continues, the other is new although a is its best
    pairs, members = lc.restate_overlap(np.array([0, 0, 0, 0]), np.array([1, 1, 0, 0]), 1, 2)
    assert pairs.tolist() == [[0, 1, 2, 0], [0, 0, 2, 2]]
    link, best_a, nxt = lc.restate_match(pairs, [4], [2, 2], [3], 10, 0, 1)
    assert link.tolist() == [[3, 0, 0, 2], [10, -1, 0, 2]] and best_a.tolist() == [[0, 2]] and nxt == 11
    # the greater IoU wins, not the greater count: 3 / (30 + 10 - 3) against 2 / (2 + 10 - 2)
    link, best_a, nxt = lc.restate_match(np.array([[0, 0, 3, 0], [1, 0, 2, 5]]), [30, 2], [10], [0, 1], 2, 0, 1)
    assert link.tolist() == [[1, 1, 1, 2]] and best_a.tolist() == [[0, 3], [0, 2]] and nxt == 2
    # labels outside [0, k) are no members; no previous frame: every b is new, in order
    assert lc.restate_overlap(np.array([5, -3, 1]), np.array([0, 0, 2]), 2, 2)[0].shape == (0, 4)
    assert lc.restate_match(np.zeros((0, 4)), [], [5, 6, 7], [], 4, 1, 1)[0].tolist() == [[4, -1, -1, 0], [5, -1, -1, 0], [6, -1, -1, 0]]
    lc.check_expectations_by_hand()
    lc.check_tracker_expectations_by_hand()


@pytest.mark.parametrize('name', lc.NAMES)
def test_case_equals_the_restatement(twin, name):
    lc.check(name, CPU)


def test_argument_errors(twin):
    lc.check_argument_errors(CPU)


def test_tracker_over_sequences(twin):
    lc.check_tracker(CPU)


def test_tracks_summary_and_defaults():
    lc.check_tracks_summary()
    assert inspect.signature(pk.inference.perform_inference).parameters['tracker'].default is None
    assert inspect.signature(pk.evaluation.evaluate_clip).parameters['tracker'].default is None
    assert inspect.signature(pk.components.Tracker.__init__).parameters['min_iou'].default == 0.0
    sig = inspect.signature(pk.ops.components_overlap).parameters
    assert list(sig)[:5] == ['labels_a', 'labels_b', 'k_a', 'k_b', 'cap'] and sig['cap'].default is None and sig['trim'].default is False
    assert list(inspect.signature(pk.ops.components_match).parameters) == ['pairs', 'totals', 'table_a', 'table_b', 'track_a', 'next_id', 'min_iou']
    assert pk.ops._min_iou_fraction(0.3) == (3, 10) and pk.ops._min_iou_fraction(1 / 3) == (1, 3) and pk.ops._min_iou_fraction((7, 9)) == (7, 9)


def test_perform_inference_with_a_tracker(twin, shared):
    lc.check_end_to_end(shared)


def test_evaluate_clip_passes_the_tracker_through(twin, shared):
    lc.check_clip(shared)


def test_tracker_none_is_untouched(twin, shared, monkeypatch):
    lc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(twin, shared):
    lc.check_value_errors(shared)
