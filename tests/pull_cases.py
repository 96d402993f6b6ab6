"""Straight free legs over the query grid (include/ext/occ4d_pull.h): the restatement of the header, written from the header, the
cases and the checks shared by tests/test_pull_host.py (through the g++ twin) and tests/test_gpu_pull.py (on the device).

FREE / HIT stand on sight_cases.walk_scalar, THE WALK restated in Python integers (imported, not copied); PULL is a plain loop over
all candidates j from the far end.  Everything is compared EQUAL.  The one tolerance, of the polyline lengths, is derived at
LENGTH_MARGIN.  No grid is larger than 33 x 34 x 35, but for the two of THRESHOLD_GRIDS, which stand either side of the size at
which the pull kernel changes its path; they carry hand-made chains only."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import geodesic_cases as gc
import refine_cases as rc
import sight_cases as sc
import occlusions4d_amd as pk

SYMBOLS = ['occ4d_pull_bits_i32', 'occ4d_pull_pairs_u32', 'occ4d_pull_paths_i32']
OPS = ['grid_blocked_bits', 'grid_segments', 'geodesic_pull']
CANARY = -0x35a5a5a7
I32 = torch.int32
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
# polyline_length(waypoints) <= polyline_length(paths) * (1 + LENGTH_MARGIN): the triangle inequality in exact arithmetic.  In float64
# each of the at most 400 legs is a correctly rounded square root of an exactly representable sum (relative error 2^-53 after the
# squares' own rounding, < 3 * 2^-53 in all), and a sum of 400 non-negative terms adds at most 400 * 2^-53: together below
# 403 * 2^-53 = 4.5e-14 on either side, 9e-14 for both < 1e-12.
LENGTH_MARGIN = 1e-12


# ---------------------------------------------------------------------------------------------------------------- the restatement
def blocked_of(clear, min_clear):
    """BLOCKED: !(clear >= min_clear) -> (n,) bool."""
    return ~(np.asarray(clear, np.int64) >= int(min_clear))


def cell_of(counts, p):
    return [p // (counts[1] * counts[2]), p // counts[2] % counts[1], p % counts[2]]


def hit_scalar(blocked, counts, a, b):
    """HIT(a, b) over blocked (n,) bool, the first rule that applies."""
    n = counts[0] * counts[1] * counts[2]
    if not (0 <= a < n and 0 <= b < n):
        return -2
    if blocked[a]:
        return a
    if blocked[b]:
        return b
    return sc.walk_scalar(blocked.reshape(counts), counts, cell_of(counts, a), cell_of(counts, b))


def free_scalar(blocked, counts, a, b):
    return hit_scalar(blocked, counts, a, b) == -1


def pull_scalar(blocked, counts, row, length):
    """PULL of one chain -> (waypoints (cap,) int32, waypoint_len, the number of fallback legs that are NOT free themselves -- the
    legs the fallback exists for; a fallback leg in open space is free like any other): every j from the far end."""
    cap = len(row)
    out = np.full(cap, -1, np.int32)
    if length <= 0 or length > cap:
        return out, length, 0
    k, count, fallbacks = 0, 0, 0
    while True:
        out[count] = row[k]
        count += 1
        if k >= length - 1:
            return out, count, fallbacks
        for j in range(length - 1, k + 1, -1):
            if free_scalar(blocked, counts, int(row[k]), int(row[j])):
                k = j
                break
        else:
            fallbacks += not free_scalar(blocked, counts, int(row[k]), int(row[k + 1]))
            k += 1


def pull_all(blocked, counts, paths, path_len):
    rows = [pull_scalar(blocked, counts, row, int(length)) for row, length in zip(paths, path_len)]
    way = np.stack([r[0] for r in rows]) if rows else np.zeros((0, paths.shape[1]), np.int32)
    return way, np.array([r[1] for r in rows], np.int32), sum(r[2] for r in rows)


# ---------------------------------------------------------------------------------------------------------------- running a call
def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def on(device, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def full(device, *shape):
    return torch.full(shape, CANARY, dtype=I32, device=device)


def raw_bits(L, device, clear, min_clear):
    """occ4d_pull_bits_i32 on the plain handle L -> numpy words; a canary word behind the output."""
    n = len(clear)
    words = (n + 31) // 32
    bits, clear = full(device, words + 1), on(device, clear)                           # (named: alive across the call)
    assert L.occ4d_pull_bits_i32(ptr(clear), min_clear, n, ptr(bits), None) == pk._lib.OK, L.occ4d_last_error()
    bits = bits.cpu().numpy()
    assert bits[words] == CANARY
    return bits[:words]


def raw_pairs(L, device, bits, counts, a, b):
    hit = full(device, len(a) + 2)
    bits, a, b = on(device, bits), on(device, a), on(device, b)                         # (named: alive across the call)
    out = hit[1:]
    assert L.occ4d_pull_pairs_u32(ptr(bits), *counts, ptr(a), ptr(b), len(a), ptr(out), None) == pk._lib.OK, L.occ4d_last_error()
    hit = hit.cpu().numpy()
    assert hit[0] == CANARY and hit[-1] == CANARY
    return hit[1:-1]


def raw_paths(L, device, bits, counts, paths, path_len):
    goals, cap = paths.shape
    way, length = full(device, goals * cap + 2), full(device, goals + 2)
    bits, paths, path_len = on(device, bits), on(device, paths), on(device, path_len)   # (named: alive across the call)
    assert L.occ4d_pull_paths_i32(ptr(bits), *counts, ptr(paths), ptr(path_len), goals, cap, ptr(way[1:]), ptr(length[1:]), None) == pk._lib.OK, \
        L.occ4d_last_error()
    way, length = way.cpu().numpy(), length.cpu().numpy()
    assert way[0] == CANARY and way[-1] == CANARY and length[0] == CANARY and length[-1] == CANARY
    return way[1:-1].reshape(goals, cap), length[1:-1]


def equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), what


# ---------------------------------------------------------------------------------------------------------------- bits
BIT_LENGTHS = (0, 1, 31, 32, 33, 65, 1000)       # (1000 is no multiple of 64, nor of 32)
MIN_CLEARS = (1, 4, INT32_MIN, INT32_MAX)


def check_bits(device, twin_handle=None):
    """ops.grid_blocked_bits EQUAL to the packed restatement, twice, and to the raw entry point of the loaded library and the twin."""
    calls = 0
    for n in BIT_LENGTHS:
        rng = np.random.default_rng(n)
        clear = rng.integers(-3, 9, size=n).astype(np.int32)
        if n:                                                                          # (the extremes among the values)
            clear[::7] = INT32_MAX
            clear[3::7] = INT32_MIN
        for min_clear in MIN_CLEARS:
            want = sc.pack(blocked_of(clear, min_clear))
            for _ in range(2):
                got = pk.ops.grid_blocked_bits(on(device, clear), min_clear)
                assert got.dtype == I32 and got.device.type == torch.device(device).type
                equal(got.cpu().numpy(), want, (n, min_clear))
                calls += 1
            equal(raw_bits(pk._lib.lib(), device, clear, min_clear), want, (n, min_clear, 'raw'))
            if twin_handle is not None:
                equal(raw_bits(twin_handle, 'cpu', clear, min_clear), want, (n, min_clear, 'twin'))
    # a column view is read as it stands
    wide = np.random.default_rng(5).integers(0, 3, size=(77, 3)).astype(np.int32)
    equal(pk.ops.grid_blocked_bits(on(device, wide)[:, 1], 1).cpu().numpy(), sc.pack(blocked_of(wide[:, 1], 1)), 'column')
    assert pk._lib.lib().occ4d_pull_bits_i32(None, 1, 0, None, None) == pk._lib.OK          # n == 0 touches no pointer
    return calls


# ---------------------------------------------------------------------------------------------------------------- pairs
PAIR_GRIDS = [(1, 1, 1), (1, 1, 7), (5, 1, 4), (6, 7, 5), (33, 34, 35)]
PAIR_GRID_IDS = ['%dx%dx%d' % g for g in PAIR_GRIDS]
# the field kinds of the sight matrix that an int32 clearance has (no NaN, no second column), plus all-free and all-blocked:
# random shares of blocked points, a column of a wider array, and a clearance with several values cut at min_clear = 4
FIELDS = ['all-free', 'share-0.1', 'share-0.45', 'all-blocked', 'strided', 'levels']
ALL_PAIRS_UP_TO = 210
RANDOM_PAIRS = 4096


def field_of(kind, counts):
    """-> (clear: an (n,) int32 numpy view, a column of an (n, 3) array for 'strided'; min_clear)."""
    n = int(np.prod(counts))
    rng = np.random.default_rng([PAIR_GRIDS.index(tuple(counts)), FIELDS.index(kind)])
    if kind == 'all-free':
        return np.full(n, 7, np.int32), 1
    if kind == 'all-blocked':
        return np.zeros(n, np.int32), 1
    if kind.startswith('share-'):
        return (rng.random(n) >= float(kind[6:])).astype(np.int32), 1
    if kind == 'strided':
        return (rng.random((n, 3)) >= 0.3).astype(np.int32)[:, 1], 1
    return rng.integers(0, 30, size=n).astype(np.int32), 4


def pairs_of(counts):
    """(a, b) int32: every pair of a grid of at most 210 points, else 4096 seeded random ones -- half of them near each other, so
    that walks between free points get through --; in both cases followed by the index values -1 and n on either side and a == b."""
    n = int(np.prod(counts))
    if n <= ALL_PAIRS_UP_TO:
        a, b = (x.reshape(-1) for x in np.meshgrid(np.arange(n), np.arange(n), indexing='ij'))
    else:
        rng = np.random.default_rng(n)
        a = rng.integers(0, n, size=RANDOM_PAIRS)
        b = rng.integers(0, n, size=RANDOM_PAIRS)
        cells = np.stack(np.unravel_index(a[::2], counts), 1) + rng.integers(-4, 5, size=(len(a[::2]), 3))
        b[::2] = np.ravel_multi_index(np.clip(cells, 0, np.asarray(counts) - 1).T, counts)
    edge = [(-1, 0), (0, -1), (n, 0), (0, n), (-1, n), (n - 1, n - 1), (0, 0), (INT32_MIN, 0), (0, INT32_MAX)]
    return (np.concatenate([a, [e[0] for e in edge]]).astype(np.int32), np.concatenate([b, [e[1] for e in edge]]).astype(np.int32))


@functools.lru_cache(maxsize=None)
def expected_hits(counts, kind):
    """HIT of every pair of a case by the restatement: computed once, shared, never changed."""
    clear, min_clear = field_of(kind, counts)
    blocked = blocked_of(clear, min_clear)
    a, b = pairs_of(counts)
    want = np.array([hit_scalar(blocked, counts, int(x), int(y)) for x, y in zip(a, b)], np.int32)
    want.setflags(write=False)
    return want


def check_pairs(counts, device, twin_handle=None):
    """geodesic.straight over every field EQUAL to the restatement, twice; the raw entry point with canaries; device and twin bit
    for bit.  -> the number of library calls compared."""
    n = int(np.prod(counts))
    a, b = pairs_of(counts)
    calls = 0
    for kind in FIELDS:
        clear, min_clear = field_of(kind, counts)
        want = expected_hits(tuple(counts), kind)
        blocked = blocked_of(clear, min_clear)
        assert ((want >= -2) & (want < n)).all() and blocked[want[want >= 0]].all(), kind          # every hit >= 0 is a blocked cell
        assert (want[-9:-4] == -2).all() and (want[-2:] == -2).all(), kind                     # the index values -1, n and beyond
        dev_clear = sc.column_on(device, clear)
        for _ in range(2):
            got = pk.geodesic.straight(dev_clear, counts, on(device, a), on(device, b), min_clear)
            assert got.dtype == I32 and got.device.type == torch.device(device).type
            equal(got.cpu().numpy(), want, (counts, kind))
            calls += 1
        got = got.cpu().numpy()
        assert blocked[got[got >= 0]].all(), kind
        bits = sc.pack(blocked)
        equal(raw_pairs(pk._lib.lib(), device, bits, counts, a, b), want, (counts, kind, 'raw'))
        if twin_handle is not None:
            equal(raw_pairs(twin_handle, 'cpu', bits, counts, a, b), want, (counts, kind, 'twin'))
    return calls


def check_pair_counts(device, twin_handle=None):
    """P = 0, 1, 63, 64, 65: the first P pairs of the 6 x 7 x 5 case; P == 0 touches no pointer."""
    counts, kind = (6, 7, 5), 'share-0.45'
    clear, min_clear = field_of(kind, counts)
    bits = sc.pack(blocked_of(clear, min_clear))
    a, b = pairs_of(counts)
    pick = np.random.default_rng(3).permutation(len(a))
    for P in (0, 1, 63, 64, 65):
        sel = pick[:P]
        want = expected_hits(counts, kind)[sel]
        equal(pk.ops.grid_segments(on(device, bits), counts, on(device, a[sel]), on(device, b[sel])).cpu().numpy(), want, P)
        equal(raw_pairs(pk._lib.lib(), device, bits, counts, a[sel], b[sel]), want, (P, 'raw'))
        if twin_handle is not None:
            equal(raw_pairs(twin_handle, 'cpu', bits, counts, a[sel], b[sel]), want, (P, 'twin'))
    for L in [pk._lib.lib()] + ([twin_handle] if twin_handle is not None else []):
        assert L.occ4d_pull_pairs_u32(None, 6, 7, 5, None, None, 0, None, None) == pk._lib.OK
    # an empty grid: every index is outside, blocked is not read
    hit = pk.ops.grid_segments(torch.zeros(0, dtype=I32, device=device), (0, 3, 3), on(device, np.array([0, -1], np.int32)),
                               on(device, np.array([0, 5], np.int32)))
    assert hit.cpu().tolist() == [-2, -2]


def library_free(device, clear, counts, min_clear=1):
    """FREE(a, b) of every pair of grid points, from the library -> (n, n) bool, and the hits."""
    n = int(np.prod(counts))
    a, b = (x.reshape(-1).astype(np.int32) for x in np.meshgrid(np.arange(n), np.arange(n), indexing='ij'))
    hit = pk.geodesic.straight(on(device, clear), counts, on(device, a), on(device, b), min_clear).cpu().numpy().reshape(n, n)
    return hit == -1, hit


def check_consequences(device):
    """On what the LIBRARY returns: FREE is symmetric while HIT is not; a one-cell-thick wall that is face-, edge- or corner-
    connected separates its two sides; every hit >= 0 is a blocked cell; without a wall every pair is free."""
    counts = (6, 7, 5)
    n = 6 * 7 * 5
    asymmetric = 0
    for share, seed in ((0.15, 1), (0.3, 2), (0.45, 3)):
        clear = (np.random.default_rng(seed).random(n) >= share).astype(np.int32)
        free, hit = library_free(device, clear, counts)
        assert np.array_equal(free, free.T) and np.array_equal(free.diagonal(), clear >= 1), share
        assert (clear[hit[hit >= 0]] < 1).all() and (hit >= -1).all(), share
        asymmetric += int((hit != hit.T).sum())
    assert asymmetric > 0                                                              # the blocker depends on the direction
    ix, iy, iz = np.indices(counts)
    for name, side in (('face', ix - 3), ('staircase', ix + iy - 5), ('corner', ix + iy + iz - 8)):
        clear = (side != 0).astype(np.int32).reshape(-1)
        free, hit = library_free(device, clear, counts)
        s = side.reshape(-1)
        across = (s[:, None] < 0) & (s[None, :] > 0)
        assert across.sum() > 500 and not free[across].any() and not free.T[across].any(), name
        assert (s[hit[across]] == 0).all() and np.array_equal(free, free.T), name
    assert library_free(device, np.ones(n, np.int32), counts)[0].all()


# ---------------------------------------------------------------------------------------------------------------- pull
def serpentine(counts):
    """gc.serpentine_clear: walls at every odd ix with one gap each, at iy = ny - 1 and iy = 0 in turn; the seed at flat index 0,
    the goal the last free point."""
    clear = gc.serpentine_clear(counts)
    return clear, [0], [int(np.flatnonzero(clear >= 1)[-1])]


def dist2_of(solid):
    """The exact squared distance of every point to the nearest solid one, by brute force."""
    cells = np.stack(np.nonzero(np.ones(solid.shape, bool)), 1)
    sites = np.stack(np.nonzero(solid), 1)
    return ((cells[:, None, :] - sites[None, :, :]) ** 2).sum(2).min(1).astype(np.int32)


def _pull_cases():
    """name -> dict(counts, clear, min_clear, seeds, goals, cap[, points, waypoints: the pinned counts of goal 0])."""
    cases = {}

    def add(name, counts, clear, seeds, goals, cap=None, min_clear=1, **pinned):
        cases[name] = dict(counts=counts, clear=np.asarray(clear, np.int32).reshape(-1), min_clear=min_clear, seeds=np.asarray(seeds, np.int32),
                           goals=np.asarray(goals, np.int32), cap=cap, **pinned)
    n = 9 * 7 * 5
    add('all-free-corner-to-corner', (9, 7, 5), np.ones(n), [0], [n - 1], points=9, waypoints=2)
    add('goal-is-a-seed-L1', (9, 7, 5), np.ones(n), [17], [17], points=1, waypoints=1)
    add('neighbour-L2', (9, 7, 5), np.ones(n), [17], [17 + 35 + 5 + 1], points=2, waypoints=2)
    walled = np.ones((9, 7, 5), np.int32)
    walled[4] = 0
    add('unreached-goal', (9, 7, 5), walled, [0], [n - 1], points=0, waypoints=0)
    add('cap-too-small', (9, 7, 5), np.ones(n), [0], [n - 1, 105, 0], cap=3, points=-9, waypoints=-9)
    add('no-goals', (9, 7, 5), np.ones(n), [0], [])
    add('five-goals', (9, 7, 5), (np.random.default_rng(8).random(n) >= 0.2), [0, n - 1], [n // 2, 3, n - 2, -1, n])
    add('serpentine-24x24x1', (24, 24, 1), *serpentine((24, 24, 1)), cap=400, points=277, waypoints=36)       # a second round of 256
    add('serpentine-33x20x2', (33, 20, 2), *serpentine((33, 20, 2)), cap=400, points=324, waypoints=50)
    m = 10 * 9 * 4
    for seed in range(6):
        clear = (np.random.default_rng(100 + seed).random(m) >= 0.3).astype(np.int32)
        free = np.flatnonzero(clear >= 1)
        add('random30-%d' % seed, (10, 9, 4), clear, free[:1], free[[-1, -2, len(free) // 2, len(free) // 3]])
    # one solid cell: at min_clear = 1 the row beside it is a free leg, at min_clear = 4 (a robot of radius 2) it is not
    solid = np.zeros((9, 9, 1), bool)
    solid[4, 4, 0] = True
    graze = dist2_of(solid)
    add('graze-min-clear-1', (9, 9, 1), graze, [3], [8 * 9 + 3], min_clear=1, points=9, waypoints=2)
    add('graze-min-clear-4', (9, 9, 1), graze, [3], [8 * 9 + 3], min_clear=4)
    return cases


PULL_CASES = _pull_cases()
PULL_NAMES = list(PULL_CASES)
RANDOM30 = [name for name in PULL_NAMES if name.startswith('random30-')]


def solve_case(c, device):
    got = pk.geodesic.solve(on(device, c['clear']), c['counts'], on(device, c['seeds']), on(device, c['goals']), c['min_clear'],
                            path_cap=c['cap'], pull=True)
    assert int(got['status'][0]) == 1 or c['clear'].size == 0
    return {k: v.cpu().numpy() for k, v in got.items()}


def check_pulled(c, paths, path_len, way, way_len):
    """The consequences of the rules on one case's output -> the number of legs that are no free segment."""
    blocked = blocked_of(c['clear'], c['min_clear'])
    counts = c['counts']
    kept = 0
    for row, L, out, W in zip(paths, path_len, way, way_len):
        if L <= 0:
            assert W == L and (out == -1).all()
            continue
        chain, points = [int(v) for v in row[:L]], [int(v) for v in out[:W]]
        assert 1 <= W <= L and (out[W:] == -1).all() and points[0] == chain[0] and points[-1] == chain[-1]
        at = [0]
        for v in points[1:]:                                                           # a subsequence: positions strictly ascending
            at.append(chain.index(v, at[-1] + 1))
        for k0, k1 in zip(at, at[1:]):
            if not free_scalar(blocked, counts, chain[k0], chain[k1]):
                assert k1 == k0 + 1, (chain[k0], chain[k1])                            # ... or one original move of the chain
                kept += 1
    spacings = (0.5, 0.25, 2.0)
    long = pk.geodesic.polyline_length(paths, path_len, spacings, counts)
    short = pk.geodesic.polyline_length(way, way_len, spacings, counts)
    reached = path_len > 0
    assert np.isnan(long[~reached]).all() and np.isnan(short[~reached]).all()
    assert (short[reached] <= long[reached] * (1 + LENGTH_MARGIN)).all(), (short, long)
    return kept


def check_pull_case(name, device, twin_handle=None):
    """solve(..., pull=True) twice with equal bits, EQUAL to the restatement on the library's own paths; the pinned counts; the
    consequences; the raw entry point with canaries on the loaded library and on the twin.  -> the fallback legs."""
    c = PULL_CASES[name]
    first, second = solve_case(c, device), solve_case(c, device)
    for key in first:
        equal(second[key], first[key], (name, key))
    paths, path_len, way, way_len = (first[k] for k in ('paths', 'path_len', 'waypoints', 'waypoint_len'))
    G = len(c['goals'])
    cap = c['cap'] or 4 * max(c['counts'])
    assert paths.shape == way.shape == (G, cap) and path_len.shape == way_len.shape == (G,) and way.dtype == way_len.dtype == np.int32
    blocked = blocked_of(c['clear'], c['min_clear'])
    want_way, want_len, fallbacks = pull_all(blocked, c['counts'], paths, path_len)
    equal(way, want_way, name)
    equal(way_len, want_len, name)
    if 'points' in c:
        assert (int(path_len[0]), int(way_len[0])) == (c['points'], c['waypoints']), (name, path_len, way_len)
    assert check_pulled(c, paths, path_len, way, way_len) == fallbacks
    bits = sc.pack(blocked)
    for L, dev in [(pk._lib.lib(), device)] + ([(twin_handle, 'cpu')] if twin_handle is not None else []):
        got = raw_paths(L, dev, bits, c['counts'], paths, path_len)
        equal(got[0], way, (name, 'raw', dev))
        equal(got[1], way_len, (name, 'raw', dev))
    return fallbacks


def check_pinned_shapes(device):
    """What the cases are there for, on the library's output."""
    got = solve_case(PULL_CASES['all-free-corner-to-corner'], device)
    assert got['waypoints'][0, :3].tolist() == [9 * 7 * 5 - 1, 0, -1]                    # exactly [goal, seed]
    got = solve_case(PULL_CASES['cap-too-small'], device)
    assert got['path_len'].tolist() == [-9, -4, 1] and got['waypoint_len'].tolist() == [-9, -4, 1]      # negative lengths pass through
    assert (got['waypoints'][:2] == -1).all() and got['waypoints'][2].tolist() == [0, -1, -1]
    got = solve_case(PULL_CASES['no-goals'], device)
    assert got['waypoints'].shape == (0, 36) and got['waypoint_len'].shape == (0,)
    # a leg that grazes the solid cell at min_clear = 1 is rejected at min_clear = 4
    one, four = PULL_CASES['graze-min-clear-1'], PULL_CASES['graze-min-clear-4']
    a, b = on(device, four['goals']), on(device, four['seeds'])
    assert pk.geodesic.straight(on(device, one['clear']), (9, 9, 1), a, b, 1).cpu().tolist() == [-1]
    assert pk.geodesic.straight(on(device, one['clear']), (9, 9, 1), a, b, 4).cpu().tolist() == [5 * 9 + 3]     # dist2 = 2 < 4, first from the goal
    wide = solve_case(four, device)
    assert solve_case(one, device)['waypoint_len'].tolist() == [2] and wide['waypoint_len'][0] > 2
    assert (four['clear'][wide['waypoints'][0, :wide['waypoint_len'][0]]] >= 4).all()


def check_hand_chains(device, L):
    """Hand-made chains through the raw entry point: a value outside [0, n) in mid-chain, a blocked point in mid-chain, L > cap,
    L <= 0; EQUAL to the restatement, canaries round every output; n_goals == 0 and n == 0 touch no pointer."""
    counts = (6, 7, 5)
    n = 6 * 7 * 5
    clear = np.ones(n, np.int32)
    clear[[40, 41, 100]] = 0
    blocked = blocked_of(clear, 1)
    cap = 12
    chains = [([0, 1, 2, 3, 4, 39, 74], 7),                                             # free all along: [0, 74]
              ([0, 1, n, 3, 4, 39, 74], 7), ([0, 1, -1, 3, 4], 5), ([INT32_MIN, 3, INT32_MAX], 3),      # outside in mid-chain, at the ends
              ([0, 5, 40, 41, 100], 5), ([40, 5, 0], 3), ([0, 5, 41], 3),                # a blocked point in mid-chain, in front, behind
              ([0, 1, 2], 13), ([0, 1, 2], INT32_MAX), ([0, 1, 2], 0), ([0, 1, 2], -5), ([0, 1, 2], INT32_MIN),
              (list(range(12)), 12), ([7], 1)]
    paths = np.full((len(chains), cap), -1, np.int32)
    for row, (values, _) in zip(paths, chains):
        row[:len(values)] = values
    path_len = np.array([length for _, length in chains], np.int32)
    want_way, want_len, fallbacks = pull_all(blocked, counts, paths, path_len)
    assert want_way[0, :3].tolist() == [0, 74, -1] and fallbacks > 4 and want_len[7:12].tolist() == [13, INT32_MAX, 0, -5, INT32_MIN]
    assert want_way[4, :want_len[4]].tolist() == [0, 5, 40, 41, 100]                    # into the blocked point and out of it by single moves
    bits = sc.pack(blocked)
    for _ in range(2):
        way, way_len = raw_paths(L, device, bits, counts, paths, path_len)
        equal(way, want_way, 'hand-made chains')
        equal(way_len, want_len, 'hand-made chains')
    assert L.occ4d_pull_paths_i32(None, 6, 7, 5, None, None, 0, 12, None, None, None) == pk._lib.OK
    assert L.occ4d_pull_paths_i32(None, 6, 0, 5, None, None, 3, 12, None, None, None) == pk._lib.OK
    way, way_len = raw_paths(L, device, bits, counts, np.zeros((3, 0), np.int32), np.array([0, 2, -1], np.int32))      # cap == 0
    assert way.shape == (3, 0) and way_len.tolist() == [0, 2, -1]


LDS_WORDS = pk._lib.PULL_CONSTANTS['LDS_WORDS']
# The two grids either side of the size at which the pull kernel takes its other path (it walks a copy of the bits in LDS while
# ceil(n / 32) <= LDS_WORDS, global memory above): exactly LDS_WORDS words, the largest staged copy, and the first grid beyond.  Far
# larger than every other case, because that size is where the path changes; the chains are hand-made and short, so the
# restatement takes a second.
THRESHOLD_GRIDS = [(512, 512, 4), (512, 512, 5)]


def check_threshold(counts, device, L):
    """Hand-made chains on a sparse random field through the raw entry point, EQUAL to the restatement, twice."""
    n = counts[0] * counts[1] * counts[2]
    assert ((n + 31) // 32 <= LDS_WORDS) == (counts == THRESHOLD_GRIDS[0]) and (512 * 512 * 4 + 31) // 32 == LDS_WORDS
    rng = np.random.default_rng(counts[2])
    blocked = rng.random(n) < 0.001
    cap, rows = 12, 4
    paths = rng.integers(0, n, size=(rows, cap)).astype(np.int32)
    paths[0, 0], paths[0, -1], paths[1, 3] = n - 1, 0, n                               # the last word, the first, a value outside
    near = np.array(np.unravel_index(paths[2, 0], counts))                             # row 2: a chain of points near each other
    for k in range(1, cap):
        near = np.clip(near + rng.integers(-9, 10, size=3), 0, np.asarray(counts) - 1)
        paths[2, k] = sc.flat_of(counts, near)
    blocked[paths[:, 0]] = False
    path_len = np.array([cap, cap, cap, 5], np.int32)
    want_way, want_len, _ = pull_all(blocked, counts, paths, path_len)
    assert (want_len >= 2).all() and (want_len < path_len).any() and (want_len > 2).any()      # some legs free, some not
    bits = sc.pack(blocked)
    for _ in range(2):
        way, way_len = raw_paths(L, device, bits, counts, paths, path_len)
        equal(way, want_way, counts)
        equal(way_len, want_len, counts)


def check_argument_errors(device):
    clear = on(device, np.ones(30, np.int32))
    bits = pk.ops.grid_blocked_bits(clear, 1)
    idx = on(device, np.zeros(4, np.int32))
    paths, length = on(device, np.zeros((2, 4), np.int32)), on(device, np.ones(2, np.int32))
    seg = lambda **k: pk.ops.grid_segments(**dict(dict(blocked=bits, counts=(3, 2, 5), a=idx, b=idx), **k))
    pull = lambda **k: pk.ops.geodesic_pull(**dict(dict(blocked=bits, counts=(3, 2, 5), paths=paths, path_len=length), **k))
    big = torch.zeros(17, dtype=I32, device=device)
    for call, kw, text in ((seg, dict(counts=(513, 1, 1), blocked=big), 'occ4d_pull_pairs_u32: nx = 513, ny = 1, nz = 1 must be <= 512'),
                           (pull, dict(counts=(1, 513, 1), blocked=big), 'occ4d_pull_paths_i32: nx = 1, ny = 513, nz = 1 must be <= 512'),
                           (seg, dict(blocked=bits[:0]), 'blocked must be'), (pull, dict(counts=(3, 2, 50)), 'blocked must be'),
                           (seg, dict(b=idx[:3]), 'a and b must be'), (pull, dict(path_len=length[:1]), 'paths and path_len must be'),
                           (pull, dict(paths=paths[0]), 'paths and path_len must be')):
        with pytest.raises(AssertionError, match=text):
            call(**kw)
    for bad in (dict(a=idx.to(torch.int64)), dict(blocked=bits.to(torch.float32))):
        with pytest.raises(AssertionError):
            seg(**bad)
    with pytest.raises(AssertionError):
        pk.ops.grid_blocked_bits(clear.to(torch.float32), 1)
    with pytest.raises(ValueError, match='pull=True needs goals'):
        pk.geodesic.solve(clear, (3, 2, 5), idx[:1], pull=True)
    way, way_len = pk.ops.geodesic_pull(torch.zeros(0, dtype=I32, device=device), (0, 3, 3), paths, on(device, np.zeros(2, np.int32)))
    assert (way.cpu().numpy() == -1).all() and way_len.cpu().tolist() == [0, 0]          # an empty grid: the trace leaves no chain


# ---------------------------------------------------------------------------------------------------------------- host pieces
def check_polyline_length():
    counts, spacings = (4, 5, 6), (0.5, 0.25, 2.0)
    flat = lambda *c: sc.flat_of(counts, c)
    paths = np.array([[flat(0, 0, 0), flat(1, 1, 1), flat(1, 1, 3), -1], [flat(3, 4, 5), -1, -1, -1], [flat(0, 0, 0), flat(3, 0, 0), -1, -1],
                      [-1] * 4, [flat(0, 0, 0), flat(0, 1, 0), flat(0, 2, 0), flat(0, 3, 0)]], np.int32)
    path_len = np.array([3, 1, 2, 0, -7], np.int32)
    want = [np.sqrt(0.25 + 0.0625 + 4.0) + 4.0, 0.0, 1.5, np.nan, np.nan]
    for args in ((paths, path_len), (torch.from_numpy(paths), torch.from_numpy(path_len))):
        got = pk.geodesic.polyline_length(*args, spacings, counts)
        assert got.dtype == np.float64 and got.shape == (5,) and np.array_equal(got, np.array(want), equal_nan=True)
    assert pk.geodesic.polyline_length(paths[:0], path_len[:0], spacings, counts).shape == (0,)


def check_paths_to_world_takes_waypoints(device):
    c = PULL_CASES['serpentine-24x24x1']
    got = solve_case(c, device)
    mins, spacings = (-1.0, 2.0, 0.5), (0.5, 0.25, 2.0)
    ways = pk.geodesic.paths_to_world(got['waypoints'], got['waypoint_len'], mins, spacings, c['counts'])
    full = pk.geodesic.paths_to_world(got['paths'], got['path_len'], mins, spacings, c['counts'])
    assert len(ways) == 1 and ways[0].shape == (36, 3) and full[0].shape == (277, 3)
    assert np.array_equal(ways[0][0], full[0][0]) and np.array_equal(ways[0][-1], full[0][-1])
    cells = np.array([cell_of(c['counts'], int(p)) for p in got['waypoints'][0, :36]])
    assert np.array_equal(ways[0], np.asarray(mins) + (cells + 0.5) * np.asarray(spacings))
    length = np.sqrt((np.diff(ways[0], axis=0) ** 2).sum(1)).sum()
    assert np.isclose(length, pk.geodesic.polyline_length(got['waypoints'], got['waypoint_len'], spacings, c['counts'])[0], rtol=1e-12, atol=0)


def check_route_option():
    R = pk.geodesic.Route
    assert list(__import__('inspect').signature(R.__init__).parameters)[-1] == 'pull'    # the LAST keyword
    assert R([0]).pull is False and R([0], [1], pull=True).pull is True and R([0], [1], pull=1).pull is True
    with pytest.raises(ValueError, match='pull=True needs goals'):
        R([0], pull=True)
    assert repr(R([0], [1], pull=True)).endswith(', pull=True)') and repr(R([0])).endswith(', path_cap=None, pull=False)')
    assert len(R([0], [1], pull=True).resolve((3, 3, 3), (0, 0, 0), (1, 1, 1))) == 3     # resolve keeps its three values
    for name in ('straight', 'pull', 'polyline_length'):
        assert callable(getattr(pk.geodesic, name))


# ---------------------------------------------------------------------------------------------------------------- end to end
NEW_KEYS = ('waypoints', 'waypoint_len')


def check_route_result(shared, got, route):
    """The new keys EQUAL to geodesic.pull on the call's own dist2, paths and path_len, and to the restatement."""
    device = shared.device
    r, dist2 = got['route'], got['clearance']['dist2']
    assert all(k in r for k in NEW_KEYS) and r['waypoints'].dtype == r['waypoint_len'].dtype == np.int32
    assert isinstance(r['waypoints'], np.ndarray) and r['waypoints'].shape == r['paths'].shape and r['waypoint_len'].shape == r['path_len'].shape
    way, way_len = pk.geodesic.pull(on(device, dist2), rc.COUNTS, on(device, r['paths']), on(device, r['path_len']), route.min_clear)
    equal(r['waypoints'], way.cpu().numpy(), 'waypoints')
    equal(r['waypoint_len'], way_len.cpu().numpy(), 'waypoint_len')
    want = pull_all(blocked_of(dist2, route.min_clear), rc.COUNTS, r['paths'], r['path_len'])
    equal(r['waypoints'], want[0], 'waypoints restated')
    equal(r['waypoint_len'], want[1], 'waypoint_len restated')
    c = dict(clear=dist2, min_clear=route.min_clear, counts=rc.COUNTS)
    check_pulled(c, r['paths'], r['path_len'], r['waypoints'], r['waypoint_len'])
    return r


def check_end_to_end(shared, monkeypatch):
    """perform_inference(clearance=, route=Route(seeds, goals, pull=True)): the new keys under the call's one host wait, every
    other key EQUAL to the pull=False call bit for bit."""
    seeds, goals = gc.fixture_points(shared)
    for kw in (dict(parent=True), dict(min_clear=2, path_cap=64)):
        route = pk.geodesic.Route(seeds, goals, pull=True, **kw)
        calls = rc.count_waits(monkeypatch)
        got = rc.infer(shared.device, shared.inputs, clearance=pk.distance.Clearance(), route=route)
        assert calls['wait'] == 1                                                       # they come home under the call's one host wait
        monkeypatch.undo()
        r = check_route_result(shared, got, route)
        assert (r['waypoint_len'][:3] >= 1).all() and r['waypoint_len'][3] == 0 and (r['waypoint_len'] <= r['path_len']).all()
        assert (r['waypoint_len'][:3] < r['path_len'][:3]).any()                        # something was pulled straight
        plain = rc.infer(shared.device, shared.inputs, clearance=pk.distance.Clearance(), route=pk.geodesic.Route(seeds, goals, **kw))
        assert sorted(got) == sorted(plain) and sorted(set(r) - set(plain['route'])) == sorted(NEW_KEYS)
        for key in plain['route']:
            equal(r[key], plain['route'][key], key)
        equal(got['clearance']['dist2'], plain['clearance']['dist2'], 'dist2')
        rc.same_result(gc.without(got), gc.without(plain))
        rc.same_result(gc.without(got), shared.dense)


def check_clip(shared):
    """evaluate_clip(clearance=, route=Route(.., pull=True), routes=[]): one dict per output frame, with the new keys."""
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = rc.clip_inputs(shared)
    seeds, goals = gc.fixture_points(shared)
    route = pk.geodesic.Route(seeds, goals, pull=True)
    clearances, routes = [], []
    clip = pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True, clearance=pk.distance.Clearance(),
                                       clearances=clearances, route=route, routes=routes)
    dense = pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True)
    assert len(clip) == len(dense) == len(routes) == 2
    for t in range(2):
        for got, want in zip(clip[t], dense[t]):
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        assert sorted(routes[t]) == ['cost', 'path_len', 'paths', 'status', 'waypoint_len', 'waypoints']
        check_route_result(shared, dict(route=routes[t], clearance=clearances[t]), route)


def check_pull_false_is_untouched(shared, monkeypatch):
    """pull=False: today's keys, and no new entry point called; pull=True: exactly the two new library calls, once each."""
    def forbidden(*a, **k):
        raise AssertionError('pull=False must not reach the pull entry points')
    for name in OPS:
        monkeypatch.setattr(pk.ops, name, forbidden)
    for name in ('pull', 'straight', '_pull_paths'):
        monkeypatch.setattr(pk.geodesic, name, forbidden)
    L = pk._lib.lib()
    for name in SYMBOLS:
        monkeypatch.setattr(L, name, forbidden)
    seeds, goals = gc.fixture_points(shared)
    res = rc.infer(shared.device, shared.inputs, clearance=pk.distance.Clearance(), route=pk.geodesic.Route(seeds, goals, parent=True))
    assert sorted(res['route']) == ['cost', 'parent', 'path_len', 'paths', 'status']
    rc.same_result(gc.without(res), shared.dense)
    res = rc.infer(shared.device, shared.inputs, clearance=pk.distance.Clearance(), route=pk.geodesic.Route(seeds, goals, pull=False))
    assert sorted(res['route']) == ['cost', 'path_len', 'paths', 'status']
    monkeypatch.undo()
    launched = []

    def recorded(name, fn):
        def call(*a, **k):
            launched.append(name)
            return fn(*a, **k)
        return call
    for name in SYMBOLS + gc.SYMBOLS:
        monkeypatch.setattr(L, name, recorded(name, getattr(L, name)))
    rc.infer(shared.device, shared.inputs, clearance=pk.distance.Clearance(), route=pk.geodesic.Route(seeds, goals, pull=True))
    assert launched == gc.SYMBOLS + ['occ4d_pull_bits_i32', 'occ4d_pull_paths_i32']
