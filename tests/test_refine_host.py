"""The coarse-to-fine decode of the query grid (include/occ4d_refine.h, inference.perform_inference(refine=...)) through the g++
twin, without a GPU: the header and its binding, the two entry points against the numpy restatement of the rules over the case
matrix of tests/refine_cases.py, the expansion's guard, and perform_inference / evaluate_clip with a GridRefine against the dense
call on the tracking fixture -- everything EQUAL, no tolerance.  The twin and the HIP kernels share the per-element source
(csrc/refine_math.hpp); tests/test_gpu_refine.py runs the same comparisons on the device."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import refine_cases as rc
import occlusions4d_amd as pk

CPU = torch.device('cpu')
NAMES = ['occ4d_refine_expand_f32', 'occ4d_refine_mark_f32']


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


def test_signature_table_matches_the_header():
    lib = pk._lib
    assert lib.FEATURE_HEADERS['REFINE'] == 'occ4d_refine.h'
    with open(lib.REFINE_HEADER_PATH) as f:
        text = f.read()
    assert lib.REFINE_SIGNATURES == lib.parse_prototypes(text, {})
    assert sorted(lib.REFINE_SIGNATURES) == NAMES
    for prefix in lib.FEATURE_HEADERS:
        if prefix != 'REFINE':
            assert not set(getattr(lib, prefix + '_SIGNATURES')) & set(NAMES), prefix
    assert not set(lib.SIGNATURES) & set(NAMES)
    assert lib.parse_constants(text) == {} and lib.ABI_VERSION == 5
    res, args = lib.REFINE_SIGNATURES['occ4d_refine_mark_f32']
    assert res is ctypes.c_int and len(args) == 12 and args[1] is ctypes.c_int64 and args[8] is ctypes.c_float
    res, args = lib.REFINE_SIGNATURES['occ4d_refine_expand_f32']
    assert res is ctypes.c_int and len(args) == 15 and args[3] is ctypes.c_int64 and args[13] is ctypes.c_int64


def test_twin_exports_and_binds_the_prototypes(twin):
    lib = pk._lib.lib()
    handle = ctypes.CDLL(pk.cpu_twin.LIB)
    for name, (res, args) in pk._lib.REFINE_SIGNATURES.items():
        assert hasattr(handle, name), name
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_restatement_on_a_grid_worked_by_hand():
    """5 x 1 x 3 points, b = 2: blocks (3, 1, 2); the representatives are x = 1, 3, 4 and z = 1, 2."""
    counts = (5, 1, 3)
    assert rc.n_blocks(counts, 2) == (3, 1, 2)
    assert rc.representative_index(counts, 2).reshape(-1).tolist() == [4, 5, 10, 11, 13, 14]
    assert rc.block_of_points(counts, 2).tolist() == [0, 0, 1, 0, 0, 1, 2, 2, 3, 2, 2, 3, 4, 4, 5]
    density = np.array([0.1, 0.1, 0.1, 0.1, 0.1, np.nan], np.float32)           # block 5 = (2, 0, 1) is hot
    active, key = rc.restate_mark(density, counts, 2, 0, 0.46)
    assert active.tolist() == [0, 0, 0, 0, 0, 1] and key.tolist() == [0] * 15       # (that block is its representative alone)
    active, key = rc.restate_mark(density, counts, 2, 1, 0.46)
    assert active.tolist() == [0, 0, 1, 1, 1, 1] and key.tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 0, 0]
    assert rc.restate_mark(np.full(6, 0.46, np.float32), counts, 2, 0, 0.46)[0].all()            # d == low is hot
    assert not rc.restate_mark(np.full(6, np.nextafter(np.float32(0.46), np.float32(0))), counts, 2, 2, 0.46)[0].any()


@pytest.mark.parametrize('counts', rc.GRIDS, ids=lambda c: '%dx%dx%d' % c)
def test_entry_point_matrix(twin, counts):
    assert rc.check_matrix(counts, CPU) == rc.cells_of(counts) == 252


def test_entry_points_on_more_than_1024_tiles(twin):
    rc.check_large(CPU)


def test_expand_guard(twin):
    rc.check_expand_guard(CPU)


def test_repeatable(twin):
    for _ in range(2):
        rc.check_cell(CPU, (17, 9, 33), 3, 1, 1, 5, True, 'pool', np.random.default_rng(3))


def test_gathered_rows_get_a_slot_of_their_kind():
    """inference._like_slots: distinct positions, a ninth slot (position % 9 == 8) for exactly the odd rows, in order within
    a kind without gaps among that kind's positions, and _slots_len = the last position + 1."""
    inf = pk.inference
    rng = np.random.default_rng(11)
    for m, p_odd in ((0, 0.0), (1, 0.0), (1, 1.0), (8, 0.0), (9, 0.0), (17, 1.0), (100, 1 / 9), (1000, 0.5), (1000, 0.0), (37, 1.0)):
        odd = torch.from_numpy(rng.uniform(size=m) < p_odd)
        slot = inf._like_slots(odd).numpy()
        n_odd = int(odd.sum())
        assert slot.shape == (m,) and len(set(slot.tolist())) == m
        assert np.array_equal(slot % 9 == 8, odd.numpy())
        assert slot[odd.numpy()].tolist() == [9 * r + 8 for r in range(n_odd)]
        assert slot[~odd.numpy()].tolist() == [p for p in range(9 * m + 9) if p % 9 != 8][:m - n_odd]
        assert inf._slots_len(m - n_odd, n_odd) == (int(slot.max()) + 1 if m else 0)
        assert inf._slots_len(m - n_odd, n_odd) <= 9 * max(n_odd, 1) + (m - n_odd) * 9 // 8 + 1
    idx = torch.arange(5000)
    assert np.array_equal(inf._dense_slot_is_odd(idx, 512).numpy(), (np.arange(5000) % 512) % 9 == 8)
    assert inf._slot_batch(512) == (512, 504) and inf._slot_batch(32768) == (32256, 32256) and inf._slot_batch(5) == (5, 5)


def test_argument_errors(twin):
    rc.check_argument_errors(CPU)


def test_grid_refine_validates_its_ranges():
    G = pk.inference.GridRefine
    r = G(low=0.25)
    assert (r.block, r.low, r.dilate) == (2, 0.25, 1) and (G(8, 0.5, 0).block, G(3, 1, 2).dilate) == (8, 2)
    with pytest.raises(TypeError):
        G()
    with pytest.raises(TypeError):
        G(2)
    for bad in (dict(block=1), dict(block=9), dict(block=2.0), dict(dilate=-1), dict(dilate=3), dict(dilate=True), dict(low=float('nan'))):
        with pytest.raises(ValueError):
            G(**{**dict(low=0.5), **bad})
    sig = inspect.signature(pk.inference.perform_inference).parameters
    assert sig['refine'].default is None and inspect.signature(pk.evaluation.evaluate_clip).parameters['refine'].default is None
    assert inspect.signature(pk.inference.infer_device).parameters['grid_counts'].default is None


def test_grid_counts_is_what_the_sampler_generates(twin):
    for num, min_z, cb, kind, mode in ((1500, -1.0, 5.0, 'greater', 4), (4000, -0.5, 16.0, 'carla', 4), (777, -0.5, 16.0, 'carla', 2)):
        counts = pk.geometry.grid_counts(num, min_z, cb, kind, mode)
        pts = pk.geometry.sample_implicit_points_blind_device(num, min_z, cb, 1, kind, mode, 'grid', CPU)
        assert isinstance(counts, tuple) and pts.shape[0] == counts[0] * counts[1] * counts[2] >= num
        z = pts[:, 2].numpy()
        assert (np.diff(z[:counts[2]]) > 0).all() and (counts[2] == pts.shape[0] or z[counts[2]] == z[0])      # z fastest


@pytest.mark.parametrize('dilate', [0, 1])
def test_single_run_equals_the_restatement_on_the_dense_output(twin, shared, dilate):
    rc.check_single_run(shared, dilate)


def test_low_0_is_the_dense_result_and_low_2_decodes_the_representatives_only(twin, shared):
    rc.check_low_extremes(shared)


def test_track_mode_all_device_merge_equals_host_merge(twin, shared):
    rc.check_track_all(shared)


def test_scorers_see_the_expanded_array(twin, shared):
    rc.check_scorers(shared)


def test_evaluate_clip_passes_refine_through(twin, shared):
    rc.check_clip(shared)


def test_refine_none_is_untouched(twin, shared, monkeypatch):
    rc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(twin, shared):
    rc.check_value_errors(shared)
