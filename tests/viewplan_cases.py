"""The case matrix of the next best view (include/ext/occ4d_viewplan.h, ops.grid_visible / ops.viewplan_greedy, sight.plan,
sight.NextView) and a RESTATEMENT of the header's rules, written from the header and not from csrc/viewplan_math.hpp: per candidate
the lockstep walk of tests/sight_cases.py (imported, which restates occ4d_sight.h), then DEAD, RANGE and the target rule in numpy
int64, and GREEDY in Python integers over np.unpackbits.  tests/test_viewplan_host.py runs the checks through the g++ twin,
tests/test_gpu_viewplan.py on the device; everything is compared EQUAL, there is no tolerance."""
import ctypes
import functools
import inspect

import numpy as np
import pytest
import torch

import raycast_cases as yc
import refine_cases as rc
import sight_cases as sc
import occlusions4d_amd as pk

SYMBOLS = ['occ4d_viewplan_visible_u32', 'occ4d_viewplan_greedy_u32']
OPS = ['grid_visible', 'viewplan_greedy', 'viewplan_work_len']
CANARY = sc.CANARY
I32 = torch.int32
FAR = 2 ** 20
MAX_CANDIDATES, MAX_PICKS = 4096, 32


# ---------------------------------------------------------------------------------------------------------------- the restatement
def unpack(words, n):
    """BITS read back: (..., W) int32 words -> (..., n) bool; asserts that the unused bits of the last word are 0."""
    w = np.ascontiguousarray(words, dtype=np.int32)
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (-1,)), axis=-1, bitorder='little').astype(bool)
    assert not bits[..., n:].any(), 'unused bits are set'
    return bits[..., :n]


@functools.lru_cache(maxsize=None)
def blockers(counts, kind, candidate):
    """The walk of every query towards one live candidate over a field of sight_cases: computed once, shared, never changed."""
    full = sc.blockers_lockstep(sc.field_of(kind, counts)['member'].reshape(counts), counts, candidate)
    full.setflags(write=False)
    return full


def restate_vis(solid, counts, targets, candidates, max_dist2=-1, weights=(1, 1, 1), walk=None):
    """VIS -> (C, n) bool.  solid (n,) bool, targets (n,) bool, candidates (C, 3) integers, any values; walk(c) -> the (n,) blockers
    towards the candidate c, default the lockstep walk of sight_cases."""
    n = int(np.prod(counts))
    solid = np.asarray(solid, bool).reshape(counts)
    q = np.stack(np.unravel_index(np.arange(n, dtype=np.int64), counts), 1).astype(np.int64)
    out = np.zeros((len(candidates), n), bool)
    for i, c in enumerate(np.asarray(candidates, np.int64).tolist()):
        if any(abs(x) > FAR for x in c):                                             # DEAD: beyond 2^20
            continue
        if sc.inside(counts, c) and solid[tuple(c)]:                                 # DEAD: in a solid cell
            continue
        d = np.asarray(c, np.int64)[None, :] - q
        in_range = np.ones(n, bool) if max_dist2 < 0 else (np.asarray(weights, np.int64)[None, :] * d * d).sum(1) <= max_dist2
        blocker = sc.blockers_lockstep(solid, counts, c) if walk is None else walk(tuple(c))
        out[i] = np.asarray(targets, bool) & in_range & (blocker == -1)
    return out


def as_int(words):
    """(W,) int32 words -> one Python integer whose bit p is BIT p, through np.unpackbits."""
    bits = np.unpackbits(np.ascontiguousarray(words, dtype=np.int32).view(np.uint8), bitorder='little')
    return int.from_bytes(np.packbits(bits, bitorder='little').tobytes(), 'little')


def popcount(x):
    return bin(x).count('1')


def restate_greedy(vis_words, target_words, k):
    """GREEDY in Python integers -> (gain (C,), picks (k,), pick_gain (k,), status (2,)) int32."""
    rows = [as_int(r) for r in vis_words]
    remaining = as_int(target_words)
    total = popcount(remaining)
    gain = [popcount(r & remaining) for r in rows]
    picks, pick_gain, dead = [], [], False
    for _ in range(k):
        count = [popcount(r & remaining) for r in rows]
        best = max(count) if count else 0
        if dead or best == 0:
            dead = True
            picks.append(-1), pick_gain.append(0)
            continue
        c = count.index(best)                                                         # the lowest c that attains it
        picks.append(c), pick_gain.append(best)
        remaining &= ~rows[c]
    i32 = lambda v: np.array(v, np.int32).reshape(-1)
    return i32(gain), i32(picks), i32(pick_gain), i32([total, popcount(remaining)])


# ---------------------------------------------------------------------------------------------------------------- the case matrix
GRIDS = [(1, 1, 1), (1, 1, 70), (3, 2, 5), (9, 10, 11), (17, 9, 33), (20, 17, 13)]
GRID_IDS = ['%dx%dx%d' % g for g in GRIDS]
FIELDS = ['share-0', 'share-0.1', 'share-0.45', 'share-1', 'strided', 'mask']
TARGETS = ['none', 'all', 'random', 'look-1', 'look-3', 'runs', 'last']
K_VALUES = (0, 1, 4, 7)


def candidate_count(counts, kind):
    """C = 1, 3, 65 and 130 over the matrix: the large ones where the restatement's walks stay cheap."""
    if counts == (1, 1, 1):
        return 1
    if counts == (3, 2, 5):
        return 65
    if counts == (9, 10, 11) and kind in ('share-0.1', 'share-0.45'):
        return 130
    return 3 if kind != 'share-1' else 1


def candidates_of(counts, C):
    """C lattice candidates: inside the grid (free or solid, as the field has it), on the hull, outside, at +-2^20, beyond it (DEAD),
    random ones round the grid, and -- from 65 on -- duplicates of the first ones at the end."""
    nx, ny, nz = counts
    rng = np.random.default_rng([GRIDS.index(tuple(counts)), C, 3])
    inside = lambda: tuple(int(rng.integers(c)) for c in counts)
    if C == 1:
        return np.array([inside()], np.int32)
    if C == 3:
        return np.array([inside(), (FAR, -FAR, 500), (FAR + 1, 0, 0)], np.int32)
    fixed = [inside(), inside(), inside(), (0, 0, 0), (nx - 1, ny - 1, nz - 1), (nx - 1, 0, nz // 2), (-1, -1, -1), (nx, ny // 2, -3),
             (FAR, -FAR, 500), (-FAR, 0, FAR), (FAR + 1, 0, 0), (0, -FAR - 1, 0), (2 ** 31 - 1, -2 ** 31, 5), (0, 0, 2 ** 31 - 1)]
    more = [tuple(int(rng.integers(-3, c + 3)) for c in counts) for _ in range(C - len(fixed) - 8)]
    rows = fixed + more
    return np.array(rows + rows[:8], np.int64).astype(np.int32)


def targets_of(kind, field, counts):
    """(n,) bool: the points that count."""
    n = int(np.prod(counts))
    rng = np.random.default_rng([GRIDS.index(tuple(counts)), TARGETS.index(kind), 5])
    if kind == 'none':
        return np.zeros(n, bool)
    if kind == 'all':
        return np.ones(n, bool)
    if kind == 'random':
        return rng.random(n) < 0.4
    if kind.startswith('look-'):                                                      # the seen == 0 set of a sight.look
        return (sc.expected(tuple(counts), field, int(kind[5:])) >= 0).all(0)
    if kind == 'runs':                                                                # whole 64-point runs empty: the wave skip
        t = rng.random(n) < 0.5
        t[:(n // 64 // 2 + 1) * 64] = False
        t[3 * 64:5 * 64] = False
        return t
    t = np.zeros(n, bool)
    t[n - 1] = True
    return t


def ranges_of(counts):
    """(max_dist2, weights): no limit, 0, a value that cuts the grid, under both weightings."""
    mid = max(1, (max(counts) // 3) ** 2)
    return [(-1, (1, 1, 1)), (0, (1, 1, 1)), (mid, (1, 1, 1)), (-5, (3, 1, 2)), (0, (3, 1, 2)), (2 * mid, (3, 1, 2))]


def combos(counts):
    """(target kind, (max_dist2, weights), k) of one (grid, field): every range under the random targets, one in turn under the
    others."""
    ranges = ranges_of(counts)
    out = [('random', r, K_VALUES[i % 4]) for i, r in enumerate(ranges)]
    out += [(kind, ranges[i % len(ranges)], K_VALUES[(i + 1) % 4]) for i, kind in enumerate(TARGETS) if kind != 'random']
    return out


# ---------------------------------------------------------------------------------------------------------------- running a call
ptr, on = sc.ptr, sc.on


def bits_on(device, f):
    return pk.ops.grid_solid_bits(sc.column_on(device, f['values']), f['level'], sc.column_on(device, f['mask']), f['mask_level'])


def run_ops(device, bits, counts, targets, candidates, max_dist2, weights, k):
    """ops.grid_visible + ops.viewplan_greedy on the loaded library -> numpy (vis, gain, picks, pick_gain, status)."""
    tw = on(device, sc.pack(targets))
    vis = pk.ops.grid_visible(bits, counts, tw, on(device, candidates), None if max_dist2 == -1 else max_dist2, weights)
    out = pk.ops.viewplan_greedy(vis, tw, k)
    assert all(t.dtype == I32 and t.device.type == torch.device(device).type for t in (vis,) + out)
    return (vis.cpu().numpy(),) + tuple(t.cpu().numpy() for t in out)


def run_raw(L, device, solid, counts, targets, candidates, max_dist2, weights, k):
    """The two entry points on the plain library handle `L` with tensors of `device`, every output and the work array with a canary
    word behind it -> numpy (vis, gain, picks, pick_gain, status); asserts that nothing else was written."""
    nx, ny, nz = counts
    n, C = nx * ny * nz, len(candidates)
    W = (n + 31) // 32
    full = lambda count: torch.full((count + 1,), CANARY, dtype=I32, device=device)
    sizes = dict(vis=C * W, gain=C, picks=k, pick_gain=k, status=2, work=W + C + 2)
    assert sizes['work'] == pk.ops.viewplan_work_len(C, W)
    buf = {name: full(count) for name, count in sizes.items()}
    sw, tw, cd = on(device, sc.pack(solid)), on(device, sc.pack(targets)), on(device, np.ascontiguousarray(candidates, np.int32))
    assert L.occ4d_viewplan_visible_u32(ptr(sw), nx, ny, nz, ptr(tw), ptr(cd), C, *weights, max_dist2, ptr(buf['vis']), None) == pk._lib.OK, \
        L.occ4d_last_error()
    assert L.occ4d_viewplan_greedy_u32(ptr(buf['vis']), C, W, ptr(tw), k, ptr(buf['work']), ptr(buf['gain']), ptr(buf['picks']),
                                       ptr(buf['pick_gain']), ptr(buf['status']), None) == pk._lib.OK, L.occ4d_last_error()
    got = {name: t.cpu().numpy() for name, t in buf.items()}
    for name, count in sizes.items():
        assert got[name][count] == CANARY, name
    return (got['vis'][:C * W].reshape(C, W),) + tuple(got[name][:sizes[name]] for name in ('gain', 'picks', 'pick_gain', 'status'))


NAMES = ('vis', 'gain', 'picks', 'pick_gain', 'status')


def same(got, want, what):
    for g, w, key in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, key, g, w)


def identities(got, targets, what):
    """The consequences of the rules that hold for every call, on what the library returned."""
    vis, gain, picks, pick_gain, status = got
    n = len(targets)
    seen_by = unpack(vis, n)
    assert not (seen_by & ~targets[None, :]).any(), what                              # vis & ~targets == 0
    assert np.array_equal(gain, seen_by.sum(1)) and status[0] == targets.sum(), what
    live = picks[picks >= 0]
    assert len(set(live.tolist())) == len(live) and ((live >= 0) & (live < len(gain))).all(), what     # never picked twice
    assert (np.diff(pick_gain) <= 0).all() and (pick_gain[picks < 0] == 0).all() and (pick_gain[picks >= 0] > 0).all(), what
    assert status[0] - status[1] == pick_gain.sum(), what
    assert (np.diff((picks < 0).astype(int)) >= 0).all(), what                        # behind a -1 only -1
    assert status[1] == (targets & ~seen_by[live].any(0)).sum(), what


# ---------------------------------------------------------------------------------------------------------------- the checks
def check_grid(counts, device, twin_handle=None):
    """Every cell of the matrix on one grid through ops, twice with equal bits, EQUAL to the restatement; with `twin_handle` (a plain
    handle of the g++ twin beside the HIP library) also bit-equal to the twin on host arrays, through the raw entry points with
    canaries.  -> (calls compared, candidates that were live inside the grid, candidates DEAD in a solid cell)."""
    calls = live_inside = dead_solid = 0
    n = int(np.prod(counts))
    for kind in FIELDS:
        f = sc.field_of(kind, counts)
        solid = f['member']
        C = candidate_count(counts, kind)
        cand = candidates_of(counts, C)
        for c in cand.tolist():
            if sc.inside(counts, c):
                live_inside += not solid.reshape(counts)[tuple(c)]
                dead_solid += bool(solid.reshape(counts)[tuple(c)])
        bits = bits_on(device, f)
        assert np.array_equal(bits.cpu().numpy(), sc.pack(solid))
        for target_kind, (max_dist2, weights), k in combos(counts):
            targets = targets_of(target_kind, kind, counts)
            what = '%s %s %s C%d d2=%d w=%s k=%d' % (counts, kind, target_kind, C, max_dist2, weights, k)
            seen_by = restate_vis(solid, counts, targets, cand, max_dist2, weights, walk=lambda c: blockers(tuple(counts), kind, c))
            vis_words = np.stack([sc.pack(row) for row in seen_by]).reshape(C, (n + 31) // 32)
            want = (vis_words,) + restate_greedy(vis_words, sc.pack(targets), k)
            got = run_ops(device, bits, counts, targets, cand, max_dist2, weights, k)
            same(got, want, what)
            same(run_ops(device, bits, counts, targets, cand, max_dist2, weights, k), got, what + ' again')
            calls += 2
            if twin_handle is not None:
                same(run_raw(twin_handle, 'cpu', solid, counts, targets, cand, max_dist2, weights, k), got, what + ' twin')
            identities(got, targets, what)
    return calls, live_inside, dead_solid


def check_raw_canaries(device, L):
    """The raw entry points write their words and nothing behind them; n == 0 and C == 0 touch no pointer."""
    for counts, kind in (((3, 2, 5), 'mask'), ((9, 10, 11), 'share-0.1'), ((1, 1, 70), 'share-0.45')):
        f = sc.field_of(kind, counts)
        cand = candidates_of(counts, 65)
        targets = targets_of('random', kind, counts)
        n = int(np.prod(counts))
        for k in (0, 5):
            seen_by = restate_vis(f['member'], counts, targets, cand, 40, (3, 1, 2))
            vis_words = np.stack([sc.pack(row) for row in seen_by]).reshape(65, (n + 31) // 32)
            same(run_raw(L, device, f['member'], counts, targets, cand, 40, (3, 1, 2), k),
                 (vis_words,) + restate_greedy(vis_words, sc.pack(targets), k), (counts, k))
    OK = pk._lib.OK
    assert L.occ4d_viewplan_visible_u32(None, 0, 4, 4, None, None, 7, 1, 1, 1, -1, None, None) == OK
    assert L.occ4d_viewplan_visible_u32(None, 4, 4, 4, None, None, 0, 1, 1, 1, 5, None, None) == OK
    assert L.occ4d_viewplan_greedy_u32(None, 0, 6, None, 3, None, None, None, None, None, None) == OK
    assert L.occ4d_viewplan_greedy_u32(None, 5, 0, None, 0, None, None, None, None, None, None) == OK


def greedy_raw(L, device, rows, target_word, k):
    """GREEDY alone on hand-written words -> numpy (gain, picks, pick_gain, status)."""
    C, W = np.asarray(rows).shape
    as_words = lambda a: on(device, np.asarray(a, np.int64).astype(np.uint32).view(np.int32).reshape(np.shape(a)))
    vis, tw = as_words(rows), as_words(target_word)
    out = [torch.full((m + 1,), CANARY, dtype=I32, device=device) for m in (C, k, k, 2)]
    work = torch.full((W + C + 3,), CANARY, dtype=I32, device=device)
    assert L.occ4d_viewplan_greedy_u32(ptr(vis), C, W, ptr(tw), k, ptr(work), *(ptr(t) for t in out), None) == pk._lib.OK, L.occ4d_last_error()
    got = [t.cpu().numpy() for t in out]
    assert all(g[-1] == CANARY for g in got) and work.cpu().numpy()[-1] == CANARY
    return tuple(g[:-1] for g in got)


def check_greedy_by_hand(device, L):
    """GREEDY on rows written out by hand: the tie goes to the lower index, identical rows, a second-best row that loses to a
    smaller one once the best has been taken, -1 tails, zero targets, k = 0, and a row count and a word count past one pass of the
    picking workgroup and of a counting slice."""
    bit = lambda *ps: sum(1 << p for p in ps)
    rows = [[bit(0, 1, 2, 3, 4, 5)], [bit(3, 4, 5, 6, 7)], [bit(6, 7, 8)], [bit(0, 1, 2, 3, 4, 5)], [bit(9)]]
    target = [bit(*range(10))]
    # round 0: counts 6 5 3 6 1 -> 0 (the tie with 3 goes to the lower); left 6 7 8 9.  round 1: 0 2 3 0 1 -> 2: row 1, second on its
    # own, loses to row 2.  left 9.  round 2: row 4.  round 3: nothing is left.
    gain, picks, pick_gain, status = greedy_raw(L, device, rows, target, 5)
    assert gain.tolist() == [6, 5, 3, 6, 1] and picks.tolist() == [0, 2, 4, -1, -1] and pick_gain.tolist() == [6, 3, 1, 0, 0]
    assert status.tolist() == [10, 0]
    gain, picks, pick_gain, status = greedy_raw(L, device, rows, target, 2)
    assert picks.tolist() == [0, 2] and pick_gain.tolist() == [6, 3] and status.tolist() == [10, 1]
    gain, picks, pick_gain, status = greedy_raw(L, device, rows, target, 0)
    assert gain.tolist() == [6, 5, 3, 6, 1] and picks.shape == (0,) and status.tolist() == [10, 10]
    # the targets limit what counts: only bits 3 and 9
    gain, picks, pick_gain, status = greedy_raw(L, device, rows, [bit(3, 9)], 3)
    assert gain.tolist() == [1, 1, 0, 1, 1] and picks.tolist() == [0, 4, -1] and pick_gain.tolist() == [1, 1, 0] and status.tolist() == [2, 0]
    # zero targets, and rows that see nothing
    gain, picks, pick_gain, status = greedy_raw(L, device, rows, [0], 3)
    assert not gain.any() and picks.tolist() == [-1, -1, -1] and not pick_gain.any() and status.tolist() == [0, 0]
    gain, picks, pick_gain, status = greedy_raw(L, device, [[0], [0]], target, 32)
    assert not gain.any() and (picks == -1).all() and picks.shape == (32,) and status.tolist() == [10, 10]
    # the sign bit and every bit of a word
    gain, picks, pick_gain, status = greedy_raw(L, device, [[bit(31)], [2 ** 32 - 1]], [2 ** 32 - 1], 2)
    assert gain.tolist() == [1, 32] and picks.tolist() == [1, -1] and status.tolist() == [32, 0]
    # 1500 candidates (two passes of the picking workgroup) over 4100 words (two counting slices), against the restatement
    rng = np.random.default_rng(11)
    C, W = 1500, 4100
    vis = rng.integers(0, 2 ** 32, size=(C, W), dtype=np.uint64) & rng.integers(0, 2 ** 32, size=(C, W), dtype=np.uint64)
    vis[1400] = vis[7]                                                                # identical rows far apart
    tw = rng.integers(0, 2 ** 32, size=W, dtype=np.uint64)
    got = greedy_raw(L, device, vis, tw, 3)
    want = restate_greedy(vis.astype(np.uint32).view(np.int32), tw.astype(np.uint32).view(np.int32), 3)
    for g, w, key in zip(got, want, NAMES[1:]):
        assert np.array_equal(g, w), key
    # the last candidate the header admits wins a round
    vis = np.zeros((MAX_CANDIDATES, 2), np.uint64)
    vis[MAX_CANDIDATES - 1] = (5, 2 ** 32 - 1)
    vis[1023:1025, 1] = 3
    gain, picks, pick_gain, status = greedy_raw(L, device, vis, [7, 2 ** 32 - 1], 3)
    assert picks.tolist() == [MAX_CANDIDATES - 1, -1, -1] and pick_gain.tolist() == [34, 0, 0] and status.tolist() == [35, 1]
    assert gain[1023] == gain[1024] == 2 and gain.sum() == 38


def check_wall_by_hand(device):
    """A one-cell wall x == 3 across the 9 x 10 x 11 grid, the sensor far out on the low side: with m_x >= 1000 every walk towards it
    steps along x alone until it has left the grid, so the sensor sees x <= 3 -- the wall's near face included -- and nothing of
    x >= 4: 5 * 10 * 11 = 550 unseen points.  A candidate at (6, 5, 5), behind the wall, sees all 550 (free space, itself included);
    within max_dist2 = 4 the lattice ball of radius 2, 1 + 6 + 12 + 8 + 6 = 33 points, all of them in x >= 4.  A candidate beside the
    sensor sees none; one in the wall is DEAD."""
    counts = (9, 10, 11)
    ix = np.indices(counts)[0]
    solid = (ix == 3).reshape(-1)
    out = on(device, solid.astype(np.float32)[:, None])
    seen, _ = pk.sight.look(out, counts, [(-1000, 5, 5)], 0.5)
    assert np.array_equal(seen.cpu().numpy() == 0, (ix >= 4).reshape(-1))
    cand = [(6, 5, 5), (-1000, 6, 5), (3, 5, 5), (6, 5, 5)]
    got = pk.sight.plan(out, counts, seen, cand, k=3, level=0.5, keep_vis=True)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert got['gain'].tolist() == [550, 0, 0, 550] and got['picks'].tolist() == [0, -1, -1]           # the tie goes to the lower index
    assert got['pick_gain'].tolist() == [550, 0, 0] and got['status'].tolist() == [550, 0]
    assert np.array_equal(unpack(got['vis'], 990)[0], (ix >= 4).reshape(-1)) and not got['vis'][1:3].any()
    got = pk.sight.plan(out, counts, seen, cand, k=2, level=0.5, max_dist2=4)
    assert got['gain'].tolist() == [33, 0, 0, 33] and got['picks'].tolist() == [0, -1] and got['status'].tolist() == [550, 517]
    got = pk.sight.plan(out, counts, seen, cand, k=1, level=0.5, max_dist2=4, weights=(4, 1, 1))         # dx = 0: 13 points, dx = +-1: 1 each
    assert got['gain'].tolist() == [15, 0, 0, 15]
    got = pk.sight.plan(out, counts, seen, cand, k=2, level=0.5, among='solid')                        # every wall cell is seen: no target
    assert not got['gain'].any() and got['picks'].tolist() == [-1, -1] and got['status'].tolist() == [0, 0]


def check_consequences(device):
    """On what the LIBRARY returns: row c of vis is the packed bit 0 of sight.look(origins=[c]).seen, ANDed with the targets, for every
    live candidate without a range limit; a dead candidate's row is 0."""
    counts = (9, 10, 11)
    for kind in ('share-0.1', 'share-0.45'):
        f = sc.field_of(kind, counts)
        solid = f['member'].reshape(counts)
        bits = bits_on(device, f)
        origins = sc.origins_of(counts, 3)
        seen_now, _ = pk.ops.grid_sight(bits, counts, origins)
        targets = pk.ops.grid_blocked_bits(seen_now, 1)
        assert np.array_equal(unpack(targets.cpu().numpy(), 990), seen_now.cpu().numpy() == 0)
        cand = candidates_of(counts, 65)
        cand = cand[(np.abs(cand.astype(np.int64)) <= FAR).all(1)]
        vis = pk.ops.grid_visible(bits, counts, targets, on(device, cand)).cpu().numpy()
        assert not (vis & ~targets.cpu().numpy()[None, :]).any()
        for i, c in enumerate(cand.tolist()):
            if sc.inside(counts, c) and solid[tuple(c)]:
                assert not vis[i].any(), c
                continue
            seen_c, _ = pk.ops.grid_sight(bits, counts, [c])
            want = pk.ops.grid_blocked_bits(1 - (seen_c & 1), 1) & targets            # pack(bit 0 of seen) & targets
            assert np.array_equal(vis[i], want.cpu().numpy()), c


def check_argument_errors(device):
    f = sc.field_of('share-0.45', (9, 10, 11))
    bits = bits_on(device, f)
    targets = on(device, sc.pack(np.ones(990, bool)))
    cand = on(device, np.zeros((2, 3), np.int32))
    vis_of = lambda **k: pk.ops.grid_visible(**dict(dict(solid_bits=bits, counts=(9, 10, 11), targets=targets, candidates=cand), **k))
    for kw, text in ((dict(candidates=on(device, np.zeros((MAX_CANDIDATES + 1, 3), np.int32))), r'C = 4097 must be in \[0, 4096\]'),
                     (dict(weights=(0, 1, 1)), r'wx = 0, wy = 1, wz = 1 must be in \[1, 1024\]'),
                     (dict(weights=(1, 1025, 1)), 'wx = 1, wy = 1025, wz = 1 must be in'),
                     (dict(counts=(513, 1, 1), solid_bits=torch.zeros(17, dtype=I32, device=device), targets=torch.zeros(17, dtype=I32, device=device)),
                      'occ4d_viewplan_visible_u32: nx = 513, ny = 1, nz = 1 must be <= 512'),
                     (dict(solid_bits=bits[:-1]), 'blocked must be'), (dict(targets=targets[:-1]), 'targets must be'),
                     (dict(candidates=on(device, np.zeros((2, 2), np.int32))), 'candidates must be'),
                     (dict(out=torch.zeros(5, dtype=I32, device=device)), 'out must be')):
        with pytest.raises(AssertionError, match=text):
            vis_of(**kw)
    with pytest.raises(AssertionError):
        vis_of(candidates=cand.to(torch.int64))
    vis = vis_of()
    assert vis.shape == (2, 31) and vis_of(max_dist2=-7).equal(vis) and vis_of(candidates=cand[:0]).shape == (0, 31)
    for kw, text in ((dict(k=-1), r'k = -1 must be in \[0, 32\]'), (dict(k=33), 'k = 33 must be in'),
                     (dict(targets=targets[:-1]), 'vis and targets must be'), (dict(work=torch.zeros(33, dtype=I32, device=device)), 'work must be')):
        with pytest.raises(AssertionError, match=text):
            pk.ops.viewplan_greedy(**dict(dict(vis=vis, targets=targets, k=1), **kw))
    assert pk.ops.viewplan_work_len(2, 31) == 35
    # the caller's buffers are used; an empty candidate list and an empty grid give zeros and -1
    work, bufs = torch.zeros(40, dtype=I32, device=device), tuple(torch.full((m,), 9, dtype=I32, device=device) for m in (4, 3, 3, 2))
    gain, picks, pick_gain, status = pk.ops.viewplan_greedy(vis, targets, 3, work=work, out=bufs)
    assert gain.data_ptr() == bufs[0].data_ptr() and gain.shape == (2,) and picks.shape == (3,) and status.cpu().tolist()[0] == 990
    for empty_vis, empty_targets in ((vis[:0], targets), (torch.zeros((2, 0), dtype=I32, device=device), targets[:0])):
        gain, picks, pick_gain, status = pk.ops.viewplan_greedy(empty_vis, empty_targets, 2)
        assert not gain.cpu().numpy().any() and picks.cpu().tolist() == [-1, -1] and pick_gain.cpu().tolist() == [0, 0] and status.cpu().tolist() == [0, 0]
    assert pk.ops.grid_visible(bits[:0], (0, 3, 3), targets[:0], cand).shape == (2, 0)


# ---------------------------------------------------------------------------------------------------------------- the module
def check_plan(device):
    """sight.plan on a dense output with select, channel, among, a host array and a device tensor of candidates, against the
    restatement; its ValueErrors."""
    rng = np.random.default_rng(6)
    counts = (9, 10, 11)
    out_np = rng.random((990, 3)).astype(np.float32)
    out = on(device, out_np)
    member = sc.member_of(out_np[:, 1], 0.7, out_np[:, 2], 0.2)
    origins = np.array([(4, -2, 5), (9, 10, 11)], np.int64)
    seen, _ = pk.sight.look(out, counts, origins, 0.7, select=(2, 0.2), channel=1)
    unseen = seen.cpu().numpy() == 0
    assert 0 < (unseen & member).sum() < unseen.sum() < 990                            # the fixture's condition
    cand = np.array([(0, 0, 0), (8, 9, 10), (4, 5, 5), (-3, 4, 20), (4, 5, 5), (9, -1, 3), (FAR, 0, -FAR)], np.int64)
    for among, targets in (('all', unseen), ('solid', unseen & member)):
        for max_dist2, weights in ((None, (1, 1, 1)), (30, (1, 2, 3))):
            seen_by = restate_vis(member, counts, targets, cand, -1 if max_dist2 is None else max_dist2, weights)
            vis_words = np.stack([sc.pack(row) for row in seen_by])
            want = dict(zip(NAMES, (vis_words,) + restate_greedy(vis_words, sc.pack(targets), 4)))
            for given in (cand, cand.tolist(), on(device, cand.astype(np.int32))):
                got = pk.sight.plan(out, counts, seen, given, k=4, level=0.7, select=(2, 0.2), among=among, max_dist2=max_dist2,
                                    weights=weights, channel=1, keep_vis=True)
                assert sorted(got) == sorted(NAMES) and all(v.dtype == I32 and v.device.type == torch.device(device).type for v in got.values())
                for key in NAMES:
                    assert np.array_equal(got[key].cpu().numpy(), want[key]), (among, max_dist2, key)
    assert sorted(pk.sight.plan(out, counts, seen, cand)) == ['gain', 'pick_gain', 'picks', 'status']
    # a device tensor is taken as it is: a candidate beyond 2^20 sees nothing there, and is a ValueError on the host
    beyond = np.array([(4, 5, 5), (0, FAR + 1, 0)], np.int64)
    got = pk.sight.plan(out, counts, seen, on(device, beyond.astype(np.int32)), k=2, level=0.7)
    assert got['gain'].cpu().numpy()[1] == 0 and got['picks'].cpu().tolist()[1] == -1
    good = dict(candidates_ijk=cand, level=0.7)
    for kw, text in ((dict(level=float('nan')), 'level is NaN'), (dict(candidates_ijk=beyond), 'a candidate lies beyond 2\\^20 cells'),
                     (dict(candidates_ijk=np.zeros((0, 3), np.int32)), r'C = 0 candidates, must be in \[1, 4096\]'),
                     (dict(candidates_ijk=np.zeros((MAX_CANDIDATES + 1, 3), np.int32)), 'C = 4097 candidates'),
                     (dict(candidates_ijk=on(device, np.zeros((MAX_CANDIDATES + 1, 3), np.int32))), 'C = 4097 candidates'),
                     (dict(candidates_ijk=[(0.5, 0, 0)]), r'candidates must be \(C, 3\) integers'),
                     (dict(candidates_ijk=[(0, 0)]), r'candidates must be \(C, 3\) integers'),
                     (dict(candidates_ijk=on(device, cand)), r'a candidates tensor must be \(C, 3\) int32'),
                     (dict(k=33), r'k = 33 must be an integer in \[0, 32\]'), (dict(k=-1), 'k = -1 must be'), (dict(k=1.5), 'k = 1.5 must be'),
                     (dict(among='free'), "among = 'free' must be 'all' or 'solid'"), (dict(weights=(1, 1)), 'weights = \\(1, 1\\) must be three'),
                     (dict(weights=(1, 0, 1)), 'must be three integers in \\[1, 1024\\]'), (dict(max_dist2=2 ** 63), 'must fit int64'),
                     (dict(max_dist2='far'), 'must be integers'), (dict(select=5), 'select = 5 must be')):
        with pytest.raises(ValueError, match=text):
            pk.sight.plan(out, counts, seen, **dict(good, **kw))


def check_cells_to_world():
    mins, spacings = (-1.0, 0.5, 2.0), (0.25, 0.5, 1.0)
    ijk = np.array([[0, 0, 0], [3, -2, 7], [-1, 40, 2]])
    world = pk.sight.cells_to_world(ijk, mins, spacings)
    assert world.dtype == np.float64 and world.tolist() == [[-0.875, 0.75, 2.5], [-0.125, -0.25, 9.5], [-1.125, 20.75, 4.5]]
    assert np.array_equal(pk.sight.grid_origin(world, mins, spacings), ijk)           # the centre of a cell snaps back to the cell
    assert pk.sight.cells_to_world(ijk[0], mins, spacings).shape == (3,)
    for bad in (np.zeros((2, 2), np.int64), np.zeros((2, 3))):
        with pytest.raises(ValueError, match='cells_to_world: ijk must be'):
            pk.sight.cells_to_world(bad, mins, spacings)


def check_option():
    NV = pk.sight.NextView
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    opt = NV(pts, k=2, among='solid', max_dist2=50, weights=(1, 1, 2), level=0.4, select=(1, 0.1))
    assert (opt.k, opt.among, opt.max_dist2, opt.weights, opt.level, opt.select) == (2, 'solid', 50, (1, 1, 2), 0.4, (1, 0.1))
    assert issubclass(NV, pk.products.LevelProduct) and NV.keyword == 'next_view' and NV.clip_list[0] == 'next_views' and NV.needs[0] == 'sight'
    assert NV.reads_grid and NV.into is None and 'C=2' in repr(opt) and "among='solid'" in repr(opt)
    doc = ' '.join(NV.__doc__.split())
    assert "SHOULD BE THE Sight OPTION'S" in doc and 'There is no checkpoint' in doc and 'No device value is read' in doc
    grid = pk.products.Grid(((9, 10, 11), (-1.0, 0.5, 2.0), (0.25, 0.5, 1.0)), 0.5, False, 13, 'cpu')
    level, ijk = opt.prepare(grid)
    assert level == 0.4 and ijk.dtype == np.int32 and ijk.tolist() == [[4, -1, -2], [8, 3, 1]]
    assert NV(pts).prepare(grid)[0] == 0.5 and NV(pts).k == 1 and NV(pts, k=0).k == 0
    for args, kw, text in (((np.zeros((0, 3)),), {}, r'NextView: C = 0 candidates, must be in \[1, 4096\]'),
                           ((np.zeros((MAX_CANDIDATES + 1, 3)),), {}, 'C = 4097 candidates'),
                           ((np.zeros((3, 2)),), {}, r'NextView: candidates must be \(C, 3\) world points'),
                           ((pts,), dict(k=33), r'NextView: k = 33 must be an integer in \[0, 32\]'),
                           ((pts,), dict(among='any'), "NextView: among = 'any' must be"),
                           ((pts,), dict(weights=(1, 2000, 1)), 'NextView: weights'),
                           ((pts,), dict(level=float('nan')), 'NextView: level is NaN'),
                           ((pts,), dict(select=7), 'NextView: select = 7 must be')):
        with pytest.raises(ValueError, match=text):
            NV(*args, **kw)
    with pytest.raises(ValueError, match='beyond 2\\^20 cells'):                        # in prepare(), before the encode
        NV(np.array([[0.0, 0.0, 2.0 + FAR + 1.5]])).prepare(grid)


def check_signatures():
    """next_view stands in front of the names the suite pins at the end of both signatures."""
    names = list(inspect.signature(pk.inference.perform_inference).parameters)
    assert names[-5:] == ['next_view', 'sight', 'segments', 'tracker', 'clearance']
    names = list(inspect.signature(pk.evaluation.evaluate_clip).parameters)
    assert names[-8:] == ['next_view', 'next_views', 'sight', 'sights', 'segments', 'parts', 'route', 'routes']
    for fn in (pk.inference.perform_inference, pk.evaluation.evaluate_clip):
        assert inspect.signature(fn).parameters['next_view'].default is None and 'next_view' in fn.__doc__


# ---------------------------------------------------------------------------------------------------------------- end to end
def world_candidates(shared):
    """Seven candidate positions round the fixture's grid -> (world points, their cells): inside, beside, above, two in one cell."""
    mins, spacings = yc.frame_of(shared)
    mins, spacings = np.asarray(mins, np.float64), np.asarray(spacings, np.float64)
    cells = np.array([[2.5, 10.25, 4.75], [16.5, 3.5, 2.5], [7.5, 7.25, 30.5], [-4.5, -4.5, 4.5], [2.75, 10.5, 4.25], [13.5, 13.5, 8.5],
                      [0.5, 0.5, 0.5]])
    return mins + cells * spacings, np.floor(cells).astype(np.int64)


def without(result):
    return {k: v for k, v in result.items() if k not in ('sight', 'next_view')}


def check_result(shared, result, option, ijk):
    """result['next_view'] EQUAL to sight.plan on the call's own implicit_output and seen, and to the restatement."""
    device = shared.device
    got = result['next_view']
    assert list(got) == ['gain', 'picks', 'pick_gain', 'status'] and all(isinstance(v, np.ndarray) and v.dtype == np.int32 for v in got.values())
    assert got['gain'].shape == (len(ijk),) and got['picks'].shape == got['pick_gain'].shape == (option.k,) and got['status'].shape == (2,)
    out, seen = result['implicit_output'], result['sight']['seen']
    level = 0.5 if option.level is None else option.level
    again = pk.sight.plan(on(device, out), rc.COUNTS, on(device, seen), ijk, option.k, level, option.select, option.among,
                          option.max_dist2, option.weights)
    member = sc.member_of(out[:, 0], level) if option.select is None else sc.member_of(out[:, 0], level, out[:, option.select[0]], option.select[1])
    targets = (seen == 0) & (member if option.among == 'solid' else True)
    seen_by = restate_vis(member, rc.COUNTS, targets, ijk, -1 if option.max_dist2 is None else option.max_dist2, option.weights)
    vis_words = np.stack([sc.pack(row) for row in seen_by])
    want = dict(zip(NAMES[1:], restate_greedy(vis_words, sc.pack(targets), option.k)))
    for key in NAMES[1:]:
        assert np.array_equal(got[key], again[key].cpu().numpy()) and np.array_equal(got[key], want[key]), key
    return got


def check_end_to_end(shared, monkeypatch):
    points, origins_ijk = sc.world_origins(shared)
    mins, spacings = yc.frame_of(shared)
    cand, cand_ijk = world_candidates(shared)
    assert pk.sight.grid_origin(cand, mins, spacings).tolist() == cand_ijk.tolist()
    look = pk.sight.Sight(origins=points[:1])
    option = pk.sight.NextView(cand, k=4)
    calls = rc.count_waits(monkeypatch)
    res = rc.infer(shared.device, shared.inputs, sight=look, next_view=option)
    assert calls['wait'] == 1                                                           # exactly one host wait
    monkeypatch.undo()
    got = check_result(shared, res, option, cand_ijk)
    assert got['status'][0] > 0 and got['picks'][0] >= 0 and (got['gain'] > 0).sum() >= 2                # the fixture's condition
    # next_view=None: every other key bit for bit, and next_view changes none of them
    alone = rc.infer(shared.device, shared.inputs, sight=look, next_view=None)
    assert 'next_view' not in alone and sorted(alone) == sorted(k for k in res if k != 'next_view')
    assert np.array_equal(alone['sight']['seen'], res['sight']['seen'])
    rc.same_result(without(alone), shared.dense)
    rc.same_result(without(res), shared.dense)
    # the amodally completed parts, a range, another level and a mask column; under refine and in track_mode 'all'
    look = pk.sight.Sight(origins=points[:2], level=0.48, select=(1, 0.1))
    option = pk.sight.NextView(cand, k=3, among='solid', max_dist2=150, weights=(1, 1, 2), level=0.48, select=(1, 0.1))
    res = rc.infer(shared.device, shared.inputs, sight=look, next_view=option, components=pk.components.Components())
    check_result(shared, res, option, cand_ijk)
    option = pk.sight.NextView(cand, k=0, level=0.48)
    res = rc.infer(shared.device, shared.inputs, refine=pk.inference.GridRefine(2, 0.46, 1), sight=look, next_view=option)
    assert check_result(shared, res, option, cand_ijk)['picks'].shape == (0,)
    option = pk.sight.NextView(cand, k=2, level=0.48)
    res = rc.infer(shared.device, shared.inputs, track_mode='all', sight=look, next_view=option)
    check_result(shared, res, option, cand_ijk)
    rc.same_result(without(res), shared.dense_all)


def check_clip(shared):
    """evaluate_clip(sight=, sights=[], next_view=, next_views=[]) over two frames: one dict per output frame, and the tuples of the
    clip as without."""
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = rc.clip_inputs(shared)
    points, _ = sc.world_origins(shared)
    cand, cand_ijk = world_candidates(shared)
    look, option, sights, views = pk.sight.Sight(origins=points[:1]), pk.sight.NextView(cand, k=2), [], []
    run = lambda **kw: pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True, **kw)
    clip = run(sight=look, sights=sights, next_view=option, next_views=views)
    dense = run()
    assert len(clip) == len(dense) == len(sights) == len(views) == 2
    for t in range(2):
        for got, want in zip(clip[t], dense[t]):
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        assert list(views[t]) == ['gain', 'picks', 'pick_gain', 'status'] and views[t]['gain'].shape == (len(cand_ijk),)
        assert views[t]['status'][0] == (sights[t]['seen'] == 0).sum()
    with pytest.raises(ValueError, match='next_views'):
        run(sight=look, sights=[], next_view=option)
    with pytest.raises(ValueError, match='next_view needs sight'):
        run(next_view=option, next_views=[])
    with pytest.raises(ValueError, match='next_view must be a sight.NextView'):
        run(sight=look, sights=[], next_view=look, next_views=[])


def check_none_is_untouched(shared, monkeypatch):
    """next_view=None: no new key and no entry point called, with sight and without."""
    def forbidden(*a, **k):
        raise AssertionError('next_view=None must not reach the viewplan entry points')
    for name in OPS[:2]:
        monkeypatch.setattr(pk.ops, name, forbidden)
    monkeypatch.setattr(pk.sight, 'plan', forbidden)
    L = pk._lib.lib()
    for name in SYMBOLS:
        monkeypatch.setattr(L, name, forbidden)
    res = rc.infer(shared.device, shared.inputs, next_view=None)
    assert sorted(res) == sorted(shared.dense)
    rc.same_result(res, shared.dense)
    points, _ = sc.world_origins(shared)
    res = rc.infer(shared.device, shared.inputs, sight=pk.sight.Sight(origins=points))
    assert sorted(res) == sorted(list(shared.dense) + ['sight'])


def check_value_errors(shared):
    points, _ = sc.world_origins(shared)
    cand, _ = world_candidates(shared)
    look, option = pk.sight.Sight(origins=points), pk.sight.NextView(cand)
    with pytest.raises(ValueError, match='next_view needs sight'):
        rc.infer(shared.device, shared.inputs, next_view=option)
    with pytest.raises(ValueError, match="needs point_sample_mode 'grid'"):
        rc.infer(shared.device, shared.inputs, sight=look, next_view=option, point_sample_mode='random')
    with pytest.raises(ValueError, match='next_view must be a sight.NextView or None'):
        rc.infer(shared.device, shared.inputs, sight=look, next_view=look)
    mins, spacings = yc.frame_of(shared)
    too_far = np.asarray(mins, np.float64) + np.array([[0.5, 0.5, FAR + 1.5]]) * np.asarray(spacings, np.float64)
    with pytest.raises(ValueError, match='beyond 2\\^20 cells'):                        # in prepare(), before the encode
        rc.infer(shared.device, shared.inputs, sight=look, next_view=pk.sight.NextView(too_far))
