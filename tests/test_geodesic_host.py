"""Shortest free-space paths over the grid (include/ext/occ4d_geodesic.h, geodesic.py, inference.perform_inference(route=...))
through the g++ twin, without a GPU: the header and its binding, the three restatements against each other, the entry points against
them over the case matrix of tests/geodesic_cases.py, the traced paths, the rejected calls, the option object and the host helpers,
and perform_inference / evaluate_clip with a Route on the tracking fixture -- everything EQUAL, no tolerance.  The twin and the HIP
kernels share the neighbour table, the relax step, the parent rule and the trace (csrc/geodesic_math.hpp), but not the tiling: the twin
relaxes the whole grid as one tile, in place.  tests/test_gpu_geodesic.py runs the same comparisons on the device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import geodesic_cases as gc
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
    assert lib.ADDON_HEADERS['GEODESIC'] == 'ext/occ4d_geodesic.h'
    for table in (lib.FEATURE_HEADERS, lib.EXTENSION_HEADERS, lib.STRUCT_EXTENSION_HEADERS):
        assert 'GEODESIC' not in table
    with open(lib.GEODESIC_HEADER_PATH) as f:
        text = f.read()
    assert lib.GEODESIC_SIGNATURES == lib.parse_prototypes(text, lib._STRUCTS) and sorted(lib.GEODESIC_SIGNATURES) == gc.SYMBOLS
    for name in gc.SYMBOLS:
        assert lib.ADDON_SIGNATURES[name] == lib.GEODESIC_SIGNATURES[name]
        for other in (lib.SIGNATURES, lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
            assert name not in other
    k = lib.GEODESIC_CONSTANTS
    assert k['NONE'] == gc.NONE == 2 ** 31 - 1 == pk.geodesic.NONE and k['MAX_AXIS'] == 512 == lib.DISTANCE_CONSTANTS['MAX_AXIS']
    assert gc.TILE == (k['TILE_X'], k['TILE_Y'], k['TILE_Z']) and k['TILE_X'] * k['TILE_Y'] * k['TILE_Z'] <= 1024
    assert lib.ABI_VERSION == 5
    I, P = ctypes.c_int, ctypes.c_void_p
    assert lib.GEODESIC_SIGNATURES['occ4d_geodesic_grid_i32'] == (I, [P, I, I, I, I, P, I, I, I, I, I, I, I, P, P, P, P, P])
    assert lib.GEODESIC_SIGNATURES['occ4d_geodesic_trace_i32'] == (I, [P, P, I, P, I, I, P, P, P])
    # the default rounds: twice the sum of the tile counts, 64 on the project's grid with the tile the figures were derived for
    assert pk.ops.geodesic_default_rounds((96, 96, 58)) == 2 * sum(-(-c // t) for c, t in zip((96, 96, 58), gc.TILE))
    assert gc.TILE != (8, 8, 8) or pk.ops.geodesic_default_rounds((96, 96, 58)) == 64
    assert pk.ops.geodesic_default_rounds((1, 1, 1)) == 6 and pk.ops.geodesic_work_len(64) == 65 and pk.ops.geodesic_work_len(0) == 1


def test_twin_exports_and_binds_the_prototypes(twin):
    lib = pk._lib.lib()
    handle = ctypes.CDLL(pk.cpu_twin.LIB)
    for name, (res, args) in pk._lib.GEODESIC_SIGNATURES.items():
        assert hasattr(handle, name), name
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_restatements_on_cases_worked_by_hand():
    gc.check_by_hand()


def test_the_three_restatements_agree():
    """The numpy relaxation, the heapq Dijkstra and scipy's Dijkstra on the explicit graph, before anything is compared with them."""
    if gc.check_restatements_agree() == 0:
        pytest.skip('scipy is not installed: the relaxation and the heapq Dijkstra agree')


def test_the_serpentine_needs_more_rounds_than_it_is_given():
    assert gc.check_serpentine_needs_more_rounds() > 1


@pytest.mark.parametrize('name', gc.CONVERGED)
def test_case_equals_the_restatements(twin, name):
    gc.check(name, CPU)


def test_serpentine_with_one_round_and_solved(twin):
    gc.check_serpentine(CPU)


@pytest.mark.parametrize('name', gc.TRACED)
def test_traced_paths(twin, name):
    gc.check_trace(name, CPU)


def test_trace_of_the_serpentine(twin):
    gc.check_trace_of_serpentine(CPU)


def test_resume_goes_on_from_the_cost_it_is_given(twin):
    """One round, then three more with resume: the fixed point of a single call, in place."""
    c = gc.BY_NAME['%dx%dx%d-random40-corners-c26' % gc.BIG]
    clear, seeds = torch.from_numpy(c['clear']), torch.from_numpy(c['seeds'])
    cost, status, _ = pk.ops.grid_geodesic(clear, c['counts'], seeds, rounds=1)
    assert status.tolist() == [0, 1]
    again, status, parent = pk.ops.grid_geodesic(clear, c['counts'], None, rounds=3, parent=True, resume=cost)
    assert again.data_ptr() == cost.data_ptr() and status[0] == 1
    assert np.array_equal(again.numpy(), gc.expected(c['name'])[0]) and np.array_equal(parent.numpy(), gc.expected(c['name'])[1])


def test_argument_errors(twin):
    gc.check_argument_errors(CPU)


def test_option_object_and_grid_index():
    r = pk.geodesic.Route([5, 7])
    assert (r.goals, r.min_clear, r.connectivity, r.steps, r.rounds, r.parent, r.path_cap) == (None, 1, 26, (3, 4, 5), None, False, None)
    assert r.seeds[0] == 'flat' and r.seeds[1].dtype == np.int32 and r.seeds[1].tolist() == [5, 7]
    r = pk.geodesic.Route(np.array([[0.5, 0.5, 0.5]]), [3], min_clear=np.int64(9), connectivity=6, steps=[1, np.int32(2), 3], rounds=7, parent=1,
                          path_cap=40)
    assert r.seeds[0] == 'world' and r.goals[0] == 'flat' and (r.min_clear, r.steps, r.rounds, r.parent, r.path_cap) == (9, (1, 2, 3), 7, True, 40)
    seeds, goals, cap = r.resolve((2, 3, 4), (0.0, 0.0, 0.0), (1.0, 0.5, 0.25))
    assert seeds.dtype == np.int32 and seeds.tolist() == [(0 * 3 + 1) * 4 + 2] and goals.tolist() == [3] and cap == 40
    assert pk.geodesic.Route([0]).resolve((2, 3, 4), (0, 0, 0), (1, 1, 1))[1:] == (None, 16) and 'steps=(1, 2, 3)' in repr(r)
    for kw, text in ((dict(seeds=[[0.0, 1.0]]), 'seeds must be'), (dict(seeds=[0.5]), 'seeds must be'), (dict(seeds=[0], goals='x'), 'goals must be'),
                     (dict(seeds=[2 ** 31]), 'outside int32'), (dict(seeds=[0], steps=(3, 0, 5)), r'steps = \(3, 0, 5\) must be three integers >= 1'),
                     (dict(seeds=[0], steps=(3.0, 4, 5)), 'three integers'), (dict(seeds=[0], steps=(3, 4)), 'three integers'),
                     (dict(seeds=[0], connectivity=8), 'connectivity = 8 must be 6, 18 or 26'), (dict(seeds=[0], min_clear=1.5), 'min_clear'),
                     (dict(seeds=[0], rounds=-1), 'rounds = -1'), (dict(seeds=[0], rounds=65537), 'rounds = 65537'),
                     (dict(seeds=[0], path_cap=0), 'path_cap = 0')):
        with pytest.raises(ValueError, match=text):
            pk.geodesic.Route(**kw)
    # the cell that contains the point, in float64; the borders belong to the cell above, the far face to no cell
    frame = dict(mins=(-1.0, 0.0, 2.0), spacings=(0.5, 0.25, 1.0), counts=(4, 8, 2))
    pts = np.array([[-1.0, 0.0, 2.0], [0.99, 1.99, 3.99], [-0.5, 0.25, 3.0], [-0.75, 0.125, 2.5]])
    assert pk.geodesic.grid_index(pts, **frame).tolist() == [0, 63, (1 * 8 + 1) * 2 + 1, 0] and pk.geodesic.grid_index(pts, **frame).dtype == np.int64
    for bad in ([1.0, 0.0, 2.0], [-1.01, 0.0, 2.0], [0.0, 2.0, 2.0], [0.0, 0.0, 4.0], [np.nan, 0.0, 2.0], [np.inf, 0.0, 2.0]):
        with pytest.raises(ValueError, match='lies outside the grid'):
            pk.geodesic.grid_index(np.array([pts[0], bad]), **frame)
    with pytest.raises(ValueError, match=r'points must be \(S, 3\)'):
        pk.geodesic.grid_index(np.zeros((2, 2)), **frame)
    sig = inspect.signature(pk.inference.perform_inference).parameters
    assert sig['route'].default is None and list(sig)[-2:] == ['tracker', 'clearance']       # (pinned by tests/test_distance_host.py)
    sig = inspect.signature(pk.evaluation.evaluate_clip).parameters
    assert sig['route'].default is None and sig['routes'].default is None and list(sig)[-2:] == ['route', 'routes']
    assert 'geodesic' in pk.__all__


def test_metric_and_paths_to_world_against_numpy():
    cost = np.array([0, 3, 4, 5, 7, gc.NONE, gc.NONE - 1], np.int32)
    got = pk.geodesic.metric(torch.from_numpy(cost), 0.25)
    want = np.where(cost == gc.NONE, np.inf, cost.astype(np.float64) * (0.25 / 3.0)).astype(np.float32)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want) and got[5] == np.inf and got[1] == np.float32(0.25)
    assert pk.geodesic.metric(torch.from_numpy(cost), 2.0, step=1).tolist()[:5] == [0.0, 6.0, 8.0, 10.0, 14.0]
    with pytest.raises(AssertionError):
        pk.geodesic.metric(torch.zeros(3))
    paths = np.array([[23, 22, 1, -1], [5, -1, -1, -1], [-1, -1, -1, -1], [7, 6, 5, 4]], np.int32)
    lens = np.array([3, 1, 0, -6], np.int32)
    ways = pk.geodesic.paths_to_world(torch.from_numpy(paths), lens, (-1.0, 0.0, 2.0), (0.5, 0.25, 1.0), (2, 3, 4))
    assert [w.shape for w in ways] == [(3, 3), (1, 3), (0, 3), (4, 3)] and all(w.dtype == np.float64 for w in ways)
    assert ways[0].tolist() == [[-0.25, 0.625, 5.5], [-0.25, 0.625, 4.5], [-0.75, 0.125, 3.5]] and ways[1].tolist() == [[-0.75, 0.375, 3.5]]


def test_solve_is_the_piece(twin):
    """geodesic.solve: the keys it returns, rounds given or not, goals implying the parent on the way."""
    c = gc.BY_NAME['%dx%dx%d-random10-mid-c26' % gc.BIG]
    clear, seeds = torch.from_numpy(c['clear']), torch.from_numpy(c['seeds'])
    got = pk.geodesic.solve(clear, c['counts'], seeds)
    assert sorted(got) == ['cost', 'status'] and got['status'][0] == 1 and np.array_equal(got['cost'].numpy(), gc.expected(c['name'])[0])
    got = pk.geodesic.solve(clear, c['counts'], seeds, goals=torch.tensor([0, -4], dtype=torch.int32), rounds=5)
    assert sorted(got) == ['cost', 'path_len', 'paths', 'status'] and got['paths'].shape == (2, 4 * 17) and got['path_len'][1] == 0
    assert got['path_len'][0] >= 9 and got['paths'][0, 0] == 0
    with pytest.raises(ValueError, match='connectivity'):
        pk.geodesic.solve(clear, c['counts'], seeds, connectivity=7)
    with pytest.raises(ValueError, match='three integers'):
        pk.geodesic.solve(clear, c['counts'], seeds, steps=(1, 2))


def test_perform_inference_with_route(twin, shared):
    gc.check_end_to_end(shared)


def test_evaluate_clip_passes_route_through(twin, shared):
    gc.check_clip(shared)


def test_route_none_is_untouched(twin, shared, monkeypatch):
    gc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(twin, shared):
    gc.check_value_errors(shared)
