"""Shared by tests/test_geodesic_host.py (g++ twin) and tests/test_gpu_geodesic.py (HIP): the yardstick of the shortest free-space
paths over the grid -- three independent restatements of the rules of include/ext/occ4d_geodesic.h --, a restatement of the kernel's
synchronous block scheme (for the number of rounds a case needs), the case matrix, and the comparison, which is EQUAL everywhere:
integers only, no tolerance.

  (a) jacobi: a numpy int64 relaxation of the WHOLE grid, every point from its neighbours' values of the sweep before, iterated to
      its fixed point;
  (b) heap_dijkstra: heapq on grids of at most 4096 points;
  (c) scipy_dijkstra: scipy.sparse.csgraph.dijkstra on the explicit graph (None without scipy).

TILES.  The kernel relaxes tiles whose shape is IMPORTED from the header's constants (never copied): for every axis, grids whose
extent is tile - 1, tile, tile + 1 and 2 tile + 1."""
import functools
import heapq

import numpy as np
import pytest
import torch

import distance_cases as dc
import refine_cases as rc
import occlusions4d_amd as pk

SYMBOLS = ['occ4d_geodesic_grid_i32', 'occ4d_geodesic_trace_i32']
NONE = 2 ** 31 - 1
CANARY = -0x01234567
K = pk._lib.GEODESIC_CONSTANTS
TILE = (K['TILE_X'], K['TILE_Y'], K['TILE_Z'])
CHAMFER, UNIT = (3, 4, 5), (1, 1, 1)
LAST_STEP = 1073741823                # on (3, 1, 1): the longest path is 2 * 1073741823 = 2147483646 = INT32_MAX - 1, and one more is not
INF64 = np.int64(2) ** 62


def offsets(connectivity):
    """[(dx, dy, dz, kind)] in the header's NEIGHBOUR ORDER: c = 0 .. 26 without 13, kind = the axes changed, 1 .. 3."""
    rank = {6: 1, 18: 2, 26: 3}[connectivity]
    out = []
    for c in range(27):
        d = (c // 9 - 1, (c // 3) % 3 - 1, c % 3 - 1)
        kind = sum(x != 0 for x in d)
        if 0 < kind <= rank:
            out.append(d + (kind,))
    return out


def sources(clear, n, seeds, min_clear):
    """The seeds that are sources: in range and passable."""
    s = np.asarray(seeds, np.int64)
    s = s[(s >= 0) & (s < n)]
    return np.unique(s[clear[s] >= min_clear])


def shifted(a, d, fill):
    """b[i] = a[i + d] where i + d lies in the grid, else fill."""
    out = np.full_like(a, fill)
    src = tuple(slice(max(x, 0), a.shape[k] + min(x, 0)) for k, x in enumerate(d))
    dst = tuple(slice(max(-x, 0), a.shape[k] + min(-x, 0)) for k, x in enumerate(d))
    out[dst] = a[src]
    return out


# ---------------------------------------------------------------------------------------------------------------- the restatements
def jacobi(clear, counts, seeds, min_clear=1, connectivity=26, steps=CHAMFER):
    """(a) -> cost (n,) int32."""
    n = counts[0] * counts[1] * counts[2]
    clear = np.asarray(clear, np.int64)
    open_ = (clear >= min_clear).reshape(counts)
    cost = np.full(n, INF64)
    cost[sources(clear, n, seeds, min_clear)] = 0
    cost = cost.reshape(counts)
    while True:
        new = cost.copy()
        for dx, dy, dz, kind in offsets(connectivity):
            new = np.minimum(new, shifted(cost, (dx, dy, dz), INF64) + steps[kind - 1])
        new = np.where(open_, new, INF64)
        if np.array_equal(new, cost):
            break
        cost = new
    assert (cost[cost < INF64] <= NONE - 1).all()
    return np.where(cost >= INF64, NONE, cost).astype(np.int32).reshape(-1)


def heap_dijkstra(clear, counts, seeds, min_clear=1, connectivity=26, steps=CHAMFER):
    """(b) -> cost (n,) int32, in Python integers."""
    nx, ny, nz = counts
    n = nx * ny * nz
    open_ = (np.asarray(clear, np.int64) >= min_clear).tolist()
    dist = [None] * n
    heap = [(0, int(s)) for s in sources(np.asarray(clear, np.int64), n, seeds, min_clear)]
    moves = offsets(connectivity)
    while heap:
        d, p = heapq.heappop(heap)
        if dist[p] is not None:
            continue
        dist[p] = d
        ix, iy, iz = p // (ny * nz), (p // nz) % ny, p % nz
        for dx, dy, dz, kind in moves:
            jx, jy, jz = ix + dx, iy + dy, iz + dz
            if 0 <= jx < nx and 0 <= jy < ny and 0 <= jz < nz:
                q = (jx * ny + jy) * nz + jz
                if open_[q] and dist[q] is None:
                    heapq.heappush(heap, (d + steps[kind - 1], q))
    return np.array([NONE if d is None else d for d in dist], np.int64).astype(np.int32)


def scipy_dijkstra(clear, counts, seeds, min_clear=1, connectivity=26, steps=CHAMFER):
    """(c) -> cost (n,) int32 from the explicit graph, or None without scipy.  (float64 sums of integers below 2^53: exact.)"""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import dijkstra
    except ImportError:
        return None
    n = counts[0] * counts[1] * counts[2]
    clear = np.asarray(clear, np.int64)
    open_ = (clear >= min_clear).reshape(counts)
    index = np.arange(n, dtype=np.int64).reshape(counts)
    rows, cols, vals = [], [], []
    for dx, dy, dz, kind in offsets(connectivity):
        there = shifted(index, (dx, dy, dz), -1)
        ok = open_ & (there >= 0) & shifted(open_, (dx, dy, dz), False)
        rows.append(index[ok])
        cols.append(there[ok])
        vals.append(np.full(int(ok.sum()), float(steps[kind - 1])))
    src = sources(clear, n, seeds, min_clear)
    if len(src) == 0:
        return np.full(n, NONE, np.int32)
    graph = coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    d = dijkstra(graph, directed=True, indices=src, min_only=True)
    return np.where(np.isinf(d), float(NONE), d).astype(np.int64).astype(np.int32)


def parent_rule(cost, counts, connectivity=26, steps=CHAMFER):
    """The header's PARENT RULE applied to a cost array -> parent (n,) int32: the FIRST neighbour in order with cost + move == own."""
    n = counts[0] * counts[1] * counts[2]
    c = np.where(np.asarray(cost) == NONE, INF64, np.asarray(cost, np.int64)).reshape(counts)
    index = np.arange(n, dtype=np.int64).reshape(counts)
    parent = np.full(counts, -1, np.int64)
    for dx, dy, dz, kind in reversed(offsets(connectivity)):                  # reversed: the first in order is written last
        v = shifted(c, (dx, dy, dz), INF64)
        ok = (c > 0) & (c < INF64) & (v < INF64) & (v + steps[kind - 1] == c)
        parent[ok] = shifted(index, (dx, dy, dz), -1)[ok]
    return parent.astype(np.int32).reshape(-1)


def block_rounds(clear, counts, seeds, min_clear=1, connectivity=26, steps=CHAMFER, tile=TILE, limit=10 ** 4):
    """The kernel's block scheme, SYNCHRONOUS: in a round every tile relaxes its own points to their fixed point against the halo
    values of the round's start.  -> (cost (n,) int32, the number of rounds that changed a value).  The kernel's rounds may see a
    neighbour's newer value, which is lower: it needs at most as many."""
    n = counts[0] * counts[1] * counts[2]
    clear = np.asarray(clear, np.int64)
    open_ = (clear >= min_clear).reshape(counts)
    cost = np.full(n, INF64)
    cost[sources(clear, n, seeds, min_clear)] = 0
    cost = cost.reshape(counts)
    moves = offsets(connectivity)
    boxes = [tuple(slice(o, min(o + t, c)) for o, t, c in zip((x, y, z), tile, counts))
             for x in range(0, counts[0], tile[0]) for y in range(0, counts[1], tile[1]) for z in range(0, counts[2], tile[2])]
    for changed in range(limit):
        padded = np.pad(cost, 1, constant_values=INF64)
        new = cost.copy()
        for box in boxes:
            halo = tuple(slice(s.start, s.stop + 2) for s in box)
            local = padded[halo].copy()
            own = np.zeros(local.shape, bool)
            own[1:-1, 1:-1, 1:-1] = open_[box]
            while True:
                best = local.copy()
                for dx, dy, dz, kind in moves:
                    best = np.minimum(best, shifted(local, (dx, dy, dz), INF64) + steps[kind - 1])
                best = np.where(own, best, local)
                if np.array_equal(best, local):
                    break
                local = best
            new[box] = local[1:-1, 1:-1, 1:-1]
        if np.array_equal(new, cost):
            return np.where(cost >= INF64, NONE, cost).astype(np.int32).reshape(-1), changed
        cost = new
    raise AssertionError('block_rounds: no fixed point within %d rounds' % limit)


# ---------------------------------------------------------------------------------------------------------------- the patterns
def random_clear(counts, blocked, seed):
    """1 where passable, 0 where blocked: the fraction `blocked` of the points."""
    n = counts[0] * counts[1] * counts[2]
    return (np.random.default_rng(seed).random(n) >= blocked).astype(np.int32)


def wall_clear(counts, axis):
    """A wall one point thick right behind the first tile border of `axis` (in the middle of a short axis), with ONE hole, in the
    corner (0, 0) of the wall."""
    clear = np.ones(counts, np.int32)
    at = TILE[axis] if counts[axis] > TILE[axis] + 1 else counts[axis] // 2
    where = [slice(None)] * 3
    where[axis] = at
    clear[tuple(where)] = 0
    hole = [0, 0, 0]
    hole[axis] = at
    clear[tuple(hole)] = 1
    return clear.reshape(-1)


SERPENTINE = (2 * TILE[0] + 1, 2 * TILE[1] + 2, 2)


def serpentine_clear(counts=SERPENTINE):
    """Walls at every odd ix over all of y and z, with one hole each, at iy = 0 and iy = ny - 1 in turn: the only way from ix = 0
    to the last plane runs the length of y in every corridor, over the y tile borders again and again."""
    clear = np.ones(counts, np.int32)
    for k, ix in enumerate(range(1, counts[0], 2)):
        clear[ix] = 0
        clear[ix, counts[1] - 1 if k % 2 == 0 else 0, :] = 1
    return clear.reshape(-1)


def corners(counts):
    return [(x * counts[1] + y) * counts[2] + z for x in sorted({0, counts[0] - 1}) for y in sorted({0, counts[1] - 1})
            for z in sorted({0, counts[2] - 1})]


@functools.lru_cache(maxsize=None)
def real_dist2(counts):
    """A real clearance: ops.grid_distance of a random field at 6 % solid through the g++ twin (restated by tests/distance_cases.py)."""
    n = counts[0] * counts[1] * counts[2]
    field = np.random.default_rng(77).random(n, dtype=np.float32)
    dist2 = dc.restate(field, counts, 0.94)[0]
    dist2.setflags(write=False)
    return dist2


# ---------------------------------------------------------------------------------------------------------------- the matrix
def case(name, counts, clear, seeds, min_clear=1, connectivity=26, steps=CHAMFER, parent=True):
    return dict(name=name, counts=tuple(counts), clear=np.array(clear, np.int32).reshape(-1), seeds=np.asarray(seeds, np.int32),
                min_clear=min_clear, connectivity=connectivity, steps=tuple(steps), parent=parent)


def edge_grids():
    """For every axis: its extent tile - 1, tile, tile + 1 and 2 tile + 1, the two other axes 5 and 3 points."""
    out = []
    for axis in range(3):
        for extent in (TILE[axis] - 1, TILE[axis], TILE[axis] + 1, 2 * TILE[axis] + 1):
            counts = [5, 3, 5]
            counts[axis] = extent
            counts[(axis + 1) % 3] = 9 if extent > TILE[axis] else 3             # the longer ones cross a second axis' border too
            out.append(tuple(counts))
    return out


SMALL = [(1, 1, 1), (1, 1, 2), (512, 1, 2)]
BIG = (2 * TILE[0] + 1, 2 * TILE[1] + 1, 2 * TILE[2] + 1)
GRIDS = SMALL + edge_grids() + [BIG]


def _cases():
    out = []
    for counts in GRIDS:
        n = counts[0] * counts[1] * counts[2]
        g = '%dx%dx%d' % counts
        mid = n // 2
        ones = np.ones(n, np.int32)
        for connectivity in (6, 18, 26):
            steps = UNIT if connectivity == 6 else CHAMFER
            tag = '-c%d' % connectivity
            out.append(case(g + '-free-corner0' + tag, counts, ones, [0], connectivity=connectivity, steps=steps))
            out.append(case(g + '-random10-mid' + tag, counts, random_clear(counts, 0.1, 31), [mid, mid + 1, mid - 1],
                            connectivity=connectivity, steps=steps))
            out.append(case(g + '-random40-corners' + tag, counts, random_clear(counts, 0.4, 32), corners(counts), connectivity=connectivity,
                            steps=steps, parent=connectivity != 18))
        out.append(case(g + '-free-units-c26', counts, ones, [n - 1], steps=UNIT))
        out.append(case(g + '-free-chamfer-c6', counts, ones, corners(counts), connectivity=6, steps=CHAMFER))
        out.append(case(g + '-blocked', counts, np.zeros(n, np.int32), [0, mid, n - 1]))
        out.append(case(g + '-no-seed', counts, random_clear(counts, 0.1, 33), []))
        blocked_mid = random_clear(counts, 0.1, 34)
        blocked_mid[mid] = 0
        out.append(case(g + '-seed-not-passable', counts, blocked_mid, [mid]))
        out.append(case(g + '-seed-not-passable-and-one', counts, blocked_mid, [mid] + np.flatnonzero(blocked_mid)[-1:].tolist()))
        out.append(case(g + '-seeds-out-of-range', counts, ones, [-1, n, n + 7, -2 ** 31, 2 ** 31 - 1]))
        out.append(case(g + '-seeds-out-of-range-and-one', counts, ones, [n, mid, -5, mid], parent=False))
        for axis in range(3):
            if counts[axis] >= 3:
                out.append(case(g + '-wall%d' % axis, counts, wall_clear(counts, axis), [n - 1], connectivity=(6, 18, 26)[axis]))
        if n >= 100:
            for min_clear in (1, 9):
                out.append(case(g + '-dist2-clear%d' % min_clear, counts, real_dist2(counts), corners(counts), min_clear=min_clear))
    for k, seeds in enumerate(([0], [2], [1], [0, 2])):                      # the last legal step: costs up to INT32_MAX - 1
        out.append(case('3x1x1-last-step-%d' % k, (3, 1, 1), [1, 1, 1], seeds, connectivity=6, steps=(LAST_STEP, 1, 1)))
    out.append(case('3x1x1-last-corner-step', (3, 1, 1), [5, 5, 5], [2], min_clear=5, steps=(2, 7, LAST_STEP)))
    out.append(case('serpentine', SERPENTINE, serpentine_clear(), [0]))
    return out


CASES = _cases()
NAMES = [c['name'] for c in CASES]
BY_NAME = dict(zip(NAMES, CASES))
assert len(BY_NAME) == len(CASES)
CONVERGED = [n for n in NAMES if n != 'serpentine']       # at the default rounds; the serpentine is the case that is not


def _rules(c):
    return c['clear'], c['counts'], c['seeds'], c['min_clear'], c['connectivity'], c['steps']


def points(c):
    return c['counts'][0] * c['counts'][1] * c['counts'][2]


@functools.lru_cache(maxsize=None)
def expected(name):
    """Restatement (a) of a case and the parent rule applied to it, computed once per process; the arrays are read-only."""
    c = BY_NAME[name]
    cost = jacobi(*_rules(c))
    got = (cost, parent_rule(cost, c['counts'], c['connectivity'], c['steps']))
    for a in got:
        a.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def expected_heap(name):
    c = BY_NAME[name]
    return heap_dijkstra(*_rules(c)) if points(c) <= 4096 else None


@functools.lru_cache(maxsize=None)
def expected_scipy(name):
    return scipy_dijkstra(*_rules(BY_NAME[name]))


# ---------------------------------------------------------------------------------------------------------------- the comparison
def filled(count, device):
    return torch.full((count,), CANARY, dtype=torch.int32, device=device)


def run(c, device, rounds=None):
    """The case through ops.grid_geodesic into buffers with one canary word behind each -> numpy dict(cost, status, parent or None,
    work)."""
    n = points(c)
    rounds = pk.ops.geodesic_default_rounds(c['counts']) if rounds is None else rounds
    out = (filled(n + 1, device), filled(3, device), filled(n + 1, device) if c['parent'] else None)
    work = filled(pk.ops.geodesic_work_len(rounds) + 1, device)
    cost, status, parent = pk.ops.grid_geodesic(torch.from_numpy(c['clear']).to(device), c['counts'], torch.from_numpy(c['seeds']).to(device),
                                                c['min_clear'], c['connectivity'], c['steps'], rounds, c['parent'], out=out, work=work)
    assert cost.data_ptr() == out[0].data_ptr() and cost.shape == (n,) and status.shape == (2,) and (parent is None) == (not c['parent'])
    return dict(cost=out[0].cpu().numpy(), status=out[1].cpu().numpy(), parent=None if out[2] is None else out[2].cpu().numpy(),
                work=work.cpu().numpy())


def canaries_intact(got, c):
    n = points(c)
    assert got['cost'][n:].tolist() == [CANARY] and got['status'][2:].tolist() == [CANARY] and got['work'][-1] == CANARY, c['name']
    assert got['parent'] is None or got['parent'][n:].tolist() == [CANARY], c['name']
    return True


def same(got, name):
    """A CONVERGED run against the required results: status[0] == 1 is ASSERTED; cost equal to (a), and to (b) and (c) where they
    apply; parent equal to the header's rule applied to the restated cost; the canary words untouched."""
    c = BY_NAME[name]
    n = points(c)
    want_cost, want_parent = expected(name)
    assert canaries_intact(got, c)
    rounds = len(got['work']) - 2
    assert got['status'][0] == 1 and 0 <= got['status'][1] < rounds, (name, got['status'][:2])
    cost = got['cost'][:n]
    assert cost.dtype == np.int32 and np.array_equal(cost, want_cost), name
    for other in (expected_heap(name), expected_scipy(name)):
        assert other is None or np.array_equal(cost, other), name
    open_ = c['clear'] >= c['min_clear']
    src = sources(c['clear'].astype(np.int64), n, c['seeds'], c['min_clear'])
    assert (cost[~open_] == NONE).all() and (cost[src] == 0).all() and ((cost == 0).sum() == len(src)), name
    if c['parent']:
        assert np.array_equal(got['parent'][:n], want_parent), name
        assert ((want_parent >= 0) == ((cost > 0) & (cost != NONE))).all(), name          # a converged cost leaves no reached point without one
    return True


def check(name, device):
    assert same(run(BY_NAME[name], device), name), name


def check_by_hand():
    """The restatements on cases worked by hand, and what the patterns of the matrix are there for."""
    # a line of five with a blocked point: nothing passes
    assert jacobi([1, 1, 0, 1, 1], (1, 1, 5), [0]).tolist() == [0, 3, NONE, NONE, NONE]
    # a 1 x 3 x 3 plane, seed in the corner: 3 along an axis, 4 across, 5 never (one plane); at connectivity 6 the corner costs 6
    assert jacobi(np.ones(9), (1, 3, 3), [0]).tolist() == [0, 3, 6, 3, 4, 7, 6, 7, 8]
    assert jacobi(np.ones(9), (1, 3, 3), [0], connectivity=6).tolist() == [0, 3, 6, 3, 6, 9, 6, 9, 12]
    assert jacobi(np.ones(8), (2, 2, 2), [0]).tolist() == [0, 3, 3, 4, 3, 4, 4, 5]
    # BOTH ends of a move must be passable, and no more: the diagonal between two blocked points is a legal move
    assert jacobi([1, 0, 0, 1], (1, 2, 2), [0]).tolist() == [0, NONE, NONE, 4]
    assert jacobi([1, 0, 0, 1], (1, 2, 2), [0], connectivity=6).tolist() == [0, NONE, NONE, NONE]
    # the parent is the FIRST neighbour in raster order: point 4 of the plane is reached from 0 (4), point 8 from 4; point 5 = (1, 2)
    # at cost 7 from 1 = (0, 1) at 3 + 4, which comes before 4 = (1, 1) at 4 + 3
    assert parent_rule(jacobi(np.ones(9), (1, 3, 3), [0]), (1, 3, 3)).tolist() == [-1, 0, 1, 0, 0, 1, 3, 3, 4]
    # min_clear is a >= comparison on int32
    assert jacobi([4, 9, 8, 9], (1, 1, 4), [1], min_clear=9).tolist() == [NONE, 0, NONE, NONE]
    assert jacobi([-5, -7, -5], (1, 1, 3), [0], min_clear=-5, steps=(2, 2, 2)).tolist() == [0, NONE, NONE]
    # the last legal step
    assert expected('3x1x1-last-step-0')[0].tolist() == [0, LAST_STEP, 2 * LAST_STEP] and 2 * LAST_STEP == NONE - 1
    assert expected('3x1x1-last-step-2')[0].tolist() == [LAST_STEP, 0, LAST_STEP] and expected('3x1x1-last-step-2')[1].tolist() == [1, -1, 1]
    for counts in GRIDS:
        g = '%dx%dx%d' % counts
        n = counts[0] * counts[1] * counts[2]
        for name in (g + '-blocked', g + '-no-seed', g + '-seed-not-passable', g + '-seeds-out-of-range'):
            assert (expected(name)[0] == NONE).all() and (expected(name)[1] == -1).all(), name
        assert (expected(g + '-seed-not-passable-and-one')[0] == 0).sum() == (BY_NAME[g + '-seed-not-passable-and-one']['clear'] > 0).any() and (expected(g + '-seeds-out-of-range-and-one')[0] == 0).sum() == 1
        far = expected(g + '-free-units-c26')[0]
        assert far[0] == max(c - 1 for c in counts) and far[n - 1] == 0                  # the chessboard distance
        assert expected(g + '-free-corner0-c6')[0][n - 1] == sum(c - 1 for c in counts)  # the city-block distance
        for axis in range(3):
            if counts[axis] >= 3:                                                         # the wall is closed but for its hole
                name = g + '-wall%d' % axis
                free = jacobi(np.ones(n), counts, [n - 1], 1, BY_NAME[name]['connectivity'])
                assert expected(name)[0][0] != NONE and (n < 100 or (expected(name)[0] > free).any()), name
    assert SMALL[2][0] == K['MAX_AXIS'] and len(GRIDS) == 16 and BIG[0] * BIG[1] * BIG[2] < 10 ** 4


def check_restatements_agree():
    """(a), (b) and (c) give the same cost wherever each applies, BEFORE anything is compared with them."""
    heaps = scipys = 0
    for name in NAMES:
        a, b, c = expected(name)[0], expected_heap(name), expected_scipy(name)
        heaps += b is not None
        scipys += c is not None
        assert b is None or np.array_equal(a, b), name
        assert c is None or np.array_equal(a, c), name
    assert heaps == sum(points(c) <= 4096 for c in CASES) > 300 and scipys in (0, len(NAMES))
    return scipys


def check_serpentine_needs_more_rounds():
    """The restatement of the block scheme with the header's tile: the serpentine needs more changing rounds than the one it is
    given, more even than the default; its fixed point is that of (a)."""
    c = BY_NAME['serpentine']
    cost, changed = block_rounds(*_rules(c))
    assert np.array_equal(cost, expected('serpentine')[0]) and (cost[c['clear'] > 0] != NONE).all()
    assert changed > pk.ops.geodesic_default_rounds(c['counts']) > 1, changed
    # and on a free grid the scheme needs about one round per tile along the way
    free = block_rounds(np.ones(points(c), np.int32), c['counts'], [0])
    assert np.array_equal(free[0], jacobi(np.ones(points(c)), c['counts'], [0])) and free[1] <= sum(-(-n // t) for n, t in zip(c['counts'], TILE))
    return changed


def check_serpentine(device):
    """rounds = 1: not converged, every value an upper bound, the seeds 0; geodesic.solve(rounds=None) goes on to the fixed point."""
    c = BY_NAME['serpentine']
    n = points(c)
    want = expected('serpentine')[0]
    got = run(c, device, rounds=1)
    assert canaries_intact(got, c)
    assert got['status'][:2].tolist() == [0, 1]
    assert (got['cost'][:n].astype(np.int64) >= want).all() and got['cost'][0] == 0 and (got['cost'][:n] == 0).sum() == 1
    assert (got['cost'][:n][c['clear'] == 0] == NONE).all()
    solved = pk.geodesic.solve(torch.from_numpy(c['clear']).to(device), c['counts'], torch.from_numpy(c['seeds']).to(device), parent=True)
    assert sorted(solved) == ['cost', 'parent', 'status'] and solved['status'][0] == 1 and solved['status'][1] >= 1
    assert np.array_equal(solved['cost'].cpu().numpy(), want) and np.array_equal(solved['parent'].cpu().numpy(), expected('serpentine')[1])
    # rounds = 0: the seeds alone
    got = run(c, device, rounds=0)
    assert canaries_intact(got, c) and got['status'][:2].tolist() == [0, 0] and (got['cost'][:n] != NONE).sum() == 1 and got['cost'][0] == 0
    assert (got['parent'][:n] == -1).all()


# ---------------------------------------------------------------------------------------------------------------- the trace
def check_path(c, cost, seeds, goal, row, length):
    """One traced path: consecutive points are neighbours under the connectivity, all are passable, the step costs sum to
    cost[goal], it starts at the goal and ends at a seed."""
    nx, ny, nz = c['counts']
    path = row[:length].astype(np.int64)
    assert path[0] == goal and path[-1] in seeds and cost[path[-1]] == 0 and (row[length:] == -1).all()
    assert (c['clear'][path] >= c['min_clear']).all() and len(set(path.tolist())) == length
    xyz = np.stack([path // (ny * nz), (path // nz) % ny, path % nz], -1)
    kinds = (np.abs(np.diff(xyz, axis=0)) == 1).sum(1)
    assert (np.abs(np.diff(xyz, axis=0)) <= 1).all() and (kinds >= 1).all() and (kinds <= {6: 1, 18: 2, 26: 3}[c['connectivity']]).all()
    assert int(np.asarray(c['steps'], np.int64)[kinds - 1].sum()) == cost[goal]


def check_trace(name, device):
    """ops.geodesic_trace over EVERY point of the case as a goal, and goals out of range."""
    c = BY_NAME[name]
    n = points(c)
    assert c['parent']
    cost, status, parent = pk.ops.grid_geodesic(torch.from_numpy(c['clear']).to(device), c['counts'], torch.from_numpy(c['seeds']).to(device),
                                                c['min_clear'], c['connectivity'], c['steps'], parent=True)
    assert status.cpu().tolist()[0] == 1 and np.array_equal(cost.cpu().numpy(), expected(name)[0])
    goals = np.concatenate([np.arange(n), [-1, n, -2 ** 31, 2 ** 31 - 1]]).astype(np.int32)
    cap = min(n, 512)                                                        # (asserted below: no path of these cases is longer)
    bufs = (filled(len(goals) * cap + 1, device), filled(len(goals) + 1, device))
    paths, path_len = pk.ops.geodesic_trace(cost, parent, torch.from_numpy(goals).to(device), cap, out=bufs)
    assert paths.shape == (len(goals), cap) and path_len.shape == (len(goals),)
    assert bufs[0].cpu()[-1] == CANARY and bufs[1].cpu()[-1] == CANARY
    paths, path_len, cost = paths.cpu().numpy(), path_len.cpu().numpy(), cost.cpu().numpy()
    seeds = set(sources(c['clear'].astype(np.int64), n, c['seeds'], c['min_clear']).tolist())
    assert (path_len[n:] == 0).all() and (paths[n:] == -1).all() and (path_len >= 0).all()
    assert ((path_len[:n] == 0) == (cost == NONE)).all() and (paths[:n][cost == NONE] == -1).all() and (path_len[:n][cost == 0] == 1).all()
    for goal in np.flatnonzero(cost != NONE):
        check_path(c, cost, seeds, goal, paths[goal], path_len[goal])
    # a cap one short of the longest path: -needed, the row filled up to cap, the canary intact
    goal = int(np.argmax(path_len[:n]))
    needed = int(path_len[goal])
    if needed >= 2:
        bufs = (filled(2 * (needed - 1) + 1, device), filled(3, device))
        short, short_len = pk.ops.geodesic_trace(torch.from_numpy(cost).to(device), parent, torch.tensor([goal, goal], dtype=torch.int32, device=device),
                                                 needed - 1, out=bufs)
        assert short_len.cpu().tolist() == [-needed, -needed] and bufs[0].cpu()[-1] == CANARY and bufs[1].cpu()[-1] == CANARY
        assert np.array_equal(short.cpu().numpy(), np.stack([paths[goal][:needed - 1]] * 2))
        exact, exact_len = pk.ops.geodesic_trace(torch.from_numpy(cost).to(device), parent, torch.tensor([goal], dtype=torch.int32, device=device), needed)
        assert exact_len.cpu().tolist() == [needed] and np.array_equal(exact.cpu().numpy()[0], paths[goal][:needed])
    none, none_len = pk.ops.geodesic_trace(torch.from_numpy(cost).to(device), parent, torch.tensor([goal], dtype=torch.int32, device=device), 0)
    assert none.shape == (1, 0) and none_len.cpu().tolist() == [-needed if needed else 0]
    return int((cost != NONE).sum())


TRACED = ['%dx%dx%d-random40-corners-c26' % BIG, '%dx%dx%d-random10-mid-c6' % edge_grids()[3], '%dx%dx%d-wall0' % edge_grids()[7],
          '%dx%dx%d-dist2-clear9' % BIG, '1x1x1-free-corner0-c26', '1x1x2-blocked', '512x1x2-free-chamfer-c6']
assert all(BY_NAME[n]['parent'] for n in TRACED)


def check_trace_of_serpentine(device):
    """The longest path of the matrix: through every corridor."""
    c = BY_NAME['serpentine']
    solved = pk.geodesic.solve(torch.from_numpy(c['clear']).to(device), c['counts'], torch.from_numpy(c['seeds']).to(device),
                               goals=torch.tensor([points(c) - 1], dtype=torch.int32, device=device), path_cap=points(c))
    assert sorted(solved) == ['cost', 'path_len', 'paths', 'status']
    cost, length = solved['cost'].cpu().numpy(), int(solved['path_len'].cpu()[0])
    assert length > (SERPENTINE[0] // 2) * (SERPENTINE[1] - 2)
    check_path(c, cost, {0}, points(c) - 1, solved['paths'].cpu().numpy()[0], length)


# ---------------------------------------------------------------------------------------------------------------- the rejected calls
def check_argument_errors(device):
    """ops.grid_geodesic / geodesic_trace: rejected arguments raise AssertionError with the library's text (the table of both
    libraries' texts is tests/test_gpu_geodesic_contract_texts.py); an empty grid is a no-op."""
    z = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
    call = lambda **k: pk.ops.grid_geodesic(**dict(dict(clear=z(30) + 1, counts=(3, 2, 5), seeds=z(1)), **k))
    for kw, text in ((dict(connectivity=8), 'connectivity = 8 must be 6, 18 or 26'), (dict(steps=(3, 0, 5)), 'step_face = 3, step_edge = 0, step_corner = 5 must be >= 1'),
                     (dict(rounds=-1), r'rounds = -1 must be in \[0, 65536\]'), (dict(rounds=65537), 'rounds = 65537 must be in'),
                     (dict(clear=z(513), counts=(1, 513, 1)), 'nx = 1, ny = 513, nz = 1 must be <= 512'),
                     (dict(clear=z(3), counts=(3, 1, 1), steps=(1, LAST_STEP + 1, 1)), r'the longest path 2147483648 = \(3 - 1\) \* 1073741824 exceeds INT32_MAX - 1'),
                     (dict(clear=z(29)), r'clear must be \(30,\)'), (dict(clear=torch.zeros(30, device=device)), 'clear must be torch.int32'),
                     (dict(seeds=z(2, 2)), r'seeds must be \(S,\)'), (dict(out=(z(29), None, None)), 'out cost must be a contiguous'),
                     (dict(out=(None, z(1), None)), 'out status must be a contiguous'), (dict(out=(None, None, z(30))), 'without parent=True'),
                     (dict(rounds=4, work=z(4)), 'work must be a contiguous'), (dict(resume=z(29)), 'resume must be a contiguous')):
        with pytest.raises(AssertionError, match=text):
            call(**kw)
    for counts in ((0, 2, 5), (3, 0, 0)):
        cost, status, parent = call(clear=z(0), counts=counts, parent=True)
        assert cost.shape == (0,) and parent.shape == (0,) and status.tolist() == [0, 0] and cost.dtype == torch.int32
    cost, status, parent = call(seeds=z(0))
    assert parent is None and cost.tolist() == [NONE] * 30 and status.tolist() == [1, 0]
    trace = lambda **k: pk.ops.geodesic_trace(**dict(dict(cost=z(30), parent=z(30) - 1, goals=z(2), cap=4), **k))
    for kw, text in ((dict(cap=-1), 'cap = -1 must be >= 0'), (dict(parent=z(29)), 'cost and parent must be contiguous'),
                     (dict(goals=z(2, 2)), r'goals must be \(G,\)'), (dict(out=(z(7), None)), 'out paths must be a contiguous')):
        with pytest.raises(AssertionError, match=text):
            trace(**kw)
    paths, path_len = trace(goals=z(0))
    assert paths.shape == (0, 4) and path_len.shape == (0,)
    paths, path_len = trace()
    assert paths.tolist() == [[0, -1, -1, -1]] * 2 and path_len.tolist() == [1, 1]


# ---------------------------------------------------------------------------------------------------------------- end to end
KEYS = ('clearance', 'route')


def without(result):
    return {k: v for k, v in result.items() if k not in KEYS}


def world_of(points_query, index):
    return np.asarray(points_query[index, :3], np.float64)


def check_result(got, counts, route, seeds, goals):
    """result['route'] against restatement (a) run over the RETURNED clearance; seeds / goals: the flat indices the route's points mean."""
    n = counts[0] * counts[1] * counts[2]
    r, dist2 = got['route'], got['clearance']['dist2']
    assert sorted(r) == sorted(['cost', 'status'] + ['parent'] * route.parent + ['paths', 'path_len'] * (route.goals is not None))
    assert all(isinstance(a, np.ndarray) and a.dtype == np.int32 for a in r.values()) and r['cost'].shape == (n,) and r['status'].shape == (2,)
    assert r['status'][0] == 1                                               # converged: asserted, not assumed
    cost = jacobi(dist2, counts, seeds, route.min_clear, route.connectivity, route.steps)
    assert np.array_equal(r['cost'], cost) and (cost[seeds] == 0).all() and ((cost != NONE) & (cost > 0)).any()
    if route.parent:
        assert np.array_equal(r['parent'], parent_rule(cost, counts, route.connectivity, route.steps))
    if route.goals is not None:
        cap = route.path_cap or 4 * max(counts)
        assert r['paths'].shape == (len(goals), cap) and r['path_len'].shape == (len(goals),)
        c = dict(counts=counts, clear=dist2, min_clear=route.min_clear, connectivity=route.connectivity, steps=route.steps)
        for g, goal in enumerate(goals):
            if cost[goal] == NONE:
                assert r['path_len'][g] == 0 and (r['paths'][g] == -1).all()
            else:
                check_path(c, cost, set(int(s) for s in seeds), goal, r['paths'][g], int(r['path_len'][g]))
    return cost


def fixture_points(shared):
    """Seeds and goals on the fixture: the first and the last free query as seeds; as goals the query farthest from them, two more
    that a path reaches, and a solid one."""
    density = np.ascontiguousarray(shared.dense['implicit_output'][:, 0])
    free, solid = np.flatnonzero(density < np.float32(0.5)), np.flatnonzero(density >= np.float32(0.5))
    assert len(free) > 100 and len(solid) > 0
    seeds = free[[0, -1]]
    cost = jacobi(dc.restate(density, rc.COUNTS, 0.5)[0], rc.COUNTS, seeds)
    reached = np.flatnonzero((cost != NONE) & (cost > 0))
    assert len(reached) > 100
    return seeds, np.concatenate([[reached[np.argmax(cost[reached])]], reached[[len(reached) // 2, 7]], solid[:1]])


def check_end_to_end(shared):
    counts = rc.COUNTS
    seeds, goals = fixture_points(shared)
    frame = pk.geometry.grid_frame(rc.CASE['num_sample'], shared.inputs[3]['min_z'], shared.inputs[3]['cube_bounds'], 'greater', 4)
    assert tuple(frame[0]) == counts
    pq = shared.dense['points_query']
    # world points: the queries' own coordinates mean the queries
    assert np.array_equal(pk.geodesic.grid_index(world_of(pq, seeds), frame[1], frame[2], counts), seeds)
    assert np.array_equal(pk.geodesic.grid_index(world_of(pq, goals) + 0.3 * np.asarray(frame[2]), frame[1], frame[2], counts), goals)
    route = pk.geodesic.Route(world_of(pq, seeds), world_of(pq, goals), parent=True)
    got = rc.infer(shared.device, shared.inputs, clearance=pk.distance.Clearance(), route=route)
    cost = check_result(got, counts, route, seeds, goals)
    assert cost[goals[-1]] == NONE and (cost[goals[:-1]] != NONE).all()       # the solid goal is not reached, the free ones are
    rc.same_result(without(got), shared.dense)
    ways = pk.geodesic.paths_to_world(got['route']['paths'], got['route']['path_len'], frame[1], frame[2], counts)
    assert len(ways) == 4 and ways[3].shape == (0, 3) and np.allclose(ways[0][0], world_of(pq, goals[:1])[0], atol=1e-5)
    assert np.allclose(ways[0], pq[got['route']['paths'][0][:len(ways[0])], :3], atol=1e-5)
    # flat indices, the options, no goals: a robot of radius 2 at connectivity 6 counting steps
    route = pk.geodesic.Route(seeds.astype(np.int64), min_clear=4, connectivity=6, steps=(1, 1, 1), rounds=20)
    got = rc.infer(shared.device, shared.inputs, clearance=pk.distance.Clearance(nearest=True), route=route)
    seeds4 = seeds[got['clearance']['dist2'][seeds] >= 4]
    wide = jacobi(got['clearance']['dist2'], counts, seeds4, 4, 6, (1, 1, 1))
    assert sorted(got['route']) == ['cost', 'status'] and got['route']['status'][0] == 1 and np.array_equal(got['route']['cost'], wide)
    assert ((wide == NONE) | (got['clearance']['dist2'] >= 4)).all()
    rc.same_result(without(got), shared.dense)
    # under refine and in track_mode 'all': the route on the clearance the call returns
    route = pk.geodesic.Route(seeds, goals, path_cap=64)
    got = rc.infer(shared.device, shared.inputs, refine=pk.inference.GridRefine(2, 0.46, 1), clearance=pk.distance.Clearance(), route=route)
    dc.check_result(got, counts, pk.distance.Clearance())
    check_result(got, counts, route, seeds[got['clearance']['dist2'][seeds] >= 1], goals)
    got = rc.infer(shared.device, shared.inputs, track_mode='all', clearance=pk.distance.Clearance(), route=route)
    dc.check_result(got, counts, pk.distance.Clearance())
    check_result(got, counts, route, seeds[got['clearance']['dist2'][seeds] >= 1], goals)
    rc.same_result(without(got), shared.dense_all)


def check_clip(shared):
    """evaluate_clip(clearance=..., route=..., routes=[]) over two frames: one dict per frame, that of the perform_inference call."""
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = rc.clip_inputs(shared)
    seeds, goals = fixture_points(shared)
    route = pk.geodesic.Route(seeds, goals)
    clearances, routes = [], []
    option = pk.distance.Clearance()
    clip = pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True, clearance=option, clearances=clearances,
                                       route=route, routes=routes)
    dense = pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True)
    assert len(clip) == len(dense) == len(clearances) == len(routes) == 2
    for t in range(2):
        for got, want in zip(clip[t], dense[t]):
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        assert sorted(routes[t]) == ['cost', 'path_len', 'paths', 'status'] and routes[t]['status'][0] == 1
        assert np.array_equal(routes[t]['cost'], jacobi(clearances[t]['dist2'], rc.COUNTS, seeds[clearances[t]['dist2'][seeds] >= 1]))
    with pytest.raises(ValueError, match='routes'):
        pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', clearance=option, clearances=[], route=route)
    with pytest.raises(ValueError, match='route needs clearance'):
        pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', route=route, routes=[])
    with pytest.raises(ValueError, match='route must be a geodesic.Route'):
        pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', clearance=option, clearances=[], route=[0], routes=[])


def check_none_is_untouched(shared, monkeypatch):
    """route=None: no new key, neither entry point is called, the result is that of the call without it; with a route still one
    host wait, and exactly the two library calls."""
    def forbidden(*a, **k):
        raise AssertionError('route=None must not reach the geodesic entry points')
    for name in ('grid_geodesic', 'geodesic_trace'):
        monkeypatch.setattr(pk.ops, name, forbidden)
    monkeypatch.setattr(pk.geodesic, 'solve', forbidden)
    L = pk._lib.lib()
    for name in SYMBOLS:
        monkeypatch.setattr(L, name, forbidden)
    res = rc.infer(shared.device, shared.inputs, clearance=pk.distance.Clearance(), route=None)
    assert 'route' not in res and sorted(res) == sorted(list(shared.dense) + ['clearance'])
    rc.same_result(without(res), shared.dense)
    res = rc.infer(shared.device, shared.inputs)
    assert sorted(res) == sorted(shared.dense)
    rc.same_result(res, shared.dense)
    monkeypatch.undo()
    calls = rc.count_waits(monkeypatch)
    calls['launched'] = []

    def recorded(name, fn):
        def call(*a, **k):
            calls['launched'].append(name)
            return fn(*a, **k)
        return call
    for name in SYMBOLS:
        monkeypatch.setattr(L, name, recorded(name, getattr(L, name)))
    seeds, goals = fixture_points(shared)
    rc.infer(shared.device, shared.inputs, clearance=pk.distance.Clearance(), route=pk.geodesic.Route(seeds, goals, parent=True))
    assert calls['wait'] == 1 and calls['launched'] == SYMBOLS


def check_value_errors(shared):
    seeds, _ = fixture_points(shared)
    route, option = pk.geodesic.Route(seeds), pk.distance.Clearance()
    with pytest.raises(ValueError, match="route needs point_sample_mode 'grid'"):
        rc.infer(shared.device, shared.inputs, route=route, point_sample_mode='random')
    with pytest.raises(ValueError, match='route needs clearance'):
        rc.infer(shared.device, shared.inputs, route=route)
    with pytest.raises(ValueError, match='route must be a geodesic.Route or None'):
        rc.infer(shared.device, shared.inputs, clearance=option, route=[0])
    with pytest.raises(ValueError, match='lies outside the grid'):
        rc.infer(shared.device, shared.inputs, clearance=option, route=pk.geodesic.Route([[1e3, 0.0, 0.0]]))
    with pytest.raises(ValueError, match='lies outside the grid'):
        rc.infer(shared.device, shared.inputs, clearance=option, route=pk.geodesic.Route(seeds, [[0.0, float('nan'), 0.0]]))


# ---------------------------------------------------------------------------------------------------------------- a second handle
def run_raw(L, c, rounds=None):
    """The case on HOST arrays through the entry point of a plain library handle `L` (the g++ twin loaded beside the HIP library,
    never enabled) -> numpy dict(cost, status, parent or None) with the canary words as run() returns them."""
    import ctypes
    nx, ny, nz = c['counts']
    n = nx * ny * nz
    rounds = pk.ops.geodesic_default_rounds(c['counts']) if rounds is None else rounds
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    cost, status, work = np.full(n + 1, CANARY, np.int32), np.full(3, CANARY, np.int32), np.full(rounds + 2, CANARY, np.int32)
    parent = np.full(n + 1, CANARY, np.int32) if c['parent'] else None
    assert L.occ4d_geodesic_grid_i32(ptr(c['clear']), c['min_clear'], nx, ny, nz, ptr(c['seeds']), len(c['seeds']), c['connectivity'],
                                     *c['steps'], rounds, 0, ptr(work), ptr(cost), ptr(parent), ptr(status), None) == pk._lib.OK
    assert work[-1] == CANARY
    return dict(cost=cost, status=status, parent=parent)
