"""Shared by tests/test_evidence_host.py (through the g++ twin) and tests/test_gpu_evidence.py (on the device): the numpy int64
restatement of include/ext/occ4d_evidence.h, written from the header -- the snap in float32, the walk vectorised over the returns and
looped over the steps, the marks with np.add.at and np.bitwise_or.at --, the case matrix of the two entry points with framed output
buffers, the walks worked by hand, the contention and drop cases, the two pins to the existing walk of sight.look, the consequences
and the end-to-end comparisons of perform_inference(evidence=...) on the refine fixture.  Everything is compared EQUAL: the product
is integers.

WHAT THE RESTATEMENT IS NOT INDEPENDENT OF.  Its walk follows the header's stepping term for term -- the same six terms, the same
`not (pyx < pxy)` tests as csrc/evidence_math.hpp --, so a mistake in the stepping rule itself would be shared by both and the
matrix would not see it.  The independence comes from elsewhere: the walks worked by hand and the two pins to sight.look, whose
walk is another function (csrc/sight_math.hpp) with tests of its own; the first of these covers the 5 x 4 x 3 grid only."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import raycast_cases as yc
import refine_cases as rc
import occlusions4d_amd as pk
from track_cases import same_result

F32, I32, I64 = np.float32, np.int32, np.int64
GRIDS = [(1, 1, 1), (5, 4, 3), (33, 2, 7), (70, 3, 5), (40, 40, 40), (128, 128, 65)]     # the last: above 2^20 cells
RETURN_COUNTS = [0, 1, 63, 64, 65, 1000]
SENSOR_COUNTS = [1, 3, 40]
PLACEMENTS = ['inside', 'outside', 'far', 'own']          # of a sensor: in the grid, outside it, 2^20 cells away, in its returns' own cell
MINS, SPACINGS = (-1.3, 0.7, -0.4), (0.25, 0.3, 0.2)
FAR = 2 ** 20
SYMBOLS = ['occ4d_evidence_carve_f32', 'occ4d_evidence_classify_f32']
CONSTANTS = dict(MAX_SENSORS=4096, MAX_COORD=2 ** 20, UNKNOWN=0, FREE=1, HIT=2)
PAD, SENTINEL = 5, 0x5A5A5A5A
EV = pk.evidence


# ---------------------------------------------------------------------------------------------------------------- restatement
def snap(returns, mins, spacings):
    """SNAP -> (g (R, 3) float32, ok (R,)): floorf((p - min) / spacing) per axis in float32; ok = fabsf(g) <= 2^20 on all axes."""
    p = np.asarray(returns, F32)[:, :3]
    with np.errstate(all='ignore'):
        g = np.floor((p - np.array(mins, F32)) / np.array(spacings, F32))
        assert g.dtype == F32
        ok = (np.abs(g) <= F32(FAR)).all(1)
    return g, ok


def restate_carve(returns, sensor, origins, counts, mins=MINS, spacings=SPACINGS):
    """-> dict(passed (W,) int32, hits (n,) int32, passes (n,) int32, status (4,) int32) of the header's rules, in int64."""
    nx, ny, nz = counts
    n = nx * ny * nz
    R, V = len(returns), len(origins)
    origins = np.asarray(origins, I64).reshape(V, 3)
    v = np.zeros(R, I64) if sensor is None else np.asarray(sensor, I64)
    ok_v = (v >= 0) & (v < V)
    o = origins[np.where(ok_v, v, 0)]
    ok_v &= (np.abs(o) <= FAR).all(1)
    g, ok_g = snap(returns, mins, spacings) if R else (np.zeros((0, 3), F32), np.zeros(0, bool))
    e = np.where(ok_g[:, None], g, 0).astype(I64)
    inside = ((e >= 0) & (e < np.array(counts, I64))).all(1)
    slot = np.where(~ok_v, 1, np.where(~ok_g, 2, np.where(~inside, 3, 0)))
    status = np.bincount(slot, minlength=4).astype(I32)
    live = slot == 0
    e, o = e[live], o[live]
    flat = lambda c: (c[:, 0] * ny + c[:, 1]) * nz + c[:, 2]
    hits, passes, words = np.zeros(n, I64), np.zeros(n, I64), np.zeros((n + 31) // 32, np.uint32)
    np.add.at(hits, flat(e), 1)
    c = e.copy()
    s = np.where(o > e, 1, -1)
    m = np.abs(o - e)
    mx, my, mz = m[:, 0], m[:, 1], m[:, 2]
    pxy, pyx, pxz, pzx, pyz, pzy = my.copy(), mx.copy(), mz.copy(), mx.copy(), mz.copy(), my.copy()
    active = np.ones(len(e), bool)
    for _ in range(nx + ny + nz):
        tx = active & (c[:, 0] != o[:, 0]) & ~(pyx < pxy) & ~(pzx < pxz)
        ty = active & (c[:, 1] != o[:, 1]) & ~(pxy < pyx) & ~(pzy < pyz)
        tz = active & (c[:, 2] != o[:, 2]) & ~(pxz < pzx) & ~(pyz < pzy)
        active &= tx | ty | tz
        c[:, 0] += np.where(tx, s[:, 0], 0)
        c[:, 1] += np.where(ty, s[:, 1], 0)
        c[:, 2] += np.where(tz, s[:, 2], 0)
        pxy, pxz = pxy + np.where(tx, 2 * my, 0), pxz + np.where(tx, 2 * mz, 0)
        pyx, pyz = pyx + np.where(ty, 2 * mx, 0), pyz + np.where(ty, 2 * mz, 0)
        pzx, pzy = pzx + np.where(tz, 2 * mx, 0), pzy + np.where(tz, 2 * my, 0)
        active &= ((c >= 0) & (c < np.array(counts, I64))).all(1)
        f = flat(c[active])
        np.add.at(passes, f, 1)
        np.bitwise_or.at(words, f >> 5, (np.uint32(1) << (f & 31).astype(np.uint32)))
        if not active.any():
            break
    return dict(passed=words.view(I32), hits=hits.astype(I32), passes=passes.astype(I32), status=status)


def bits_of(words, n):
    """(n,) bool of the bit array."""
    w = np.asarray(words).view(np.uint32)
    p = np.arange(n)
    return ((w[p >> 5] >> (p & 31).astype(np.uint32)) & 1).astype(bool) if n else np.zeros(0, bool)


def restate_classify(field, level, hits, passed=None, passes=None, min_pass=1, mask=None, mask_level=0.0):
    n = len(hits)
    with np.errstate(invalid='ignore'):
        solid = np.asarray(field, F32) >= F32(level)
        if mask is not None:
            solid &= np.asarray(mask, F32) >= F32(mask_level)
    free = passes >= min_pass if passes is not None else bits_of(passed, n)
    state = np.where(hits > 0, 2, np.where(free, 1, 0))
    code = (state + 3 * solid).astype(I32)
    return code, np.bincount(code, minlength=6).astype(I64)


# ---------------------------------------------------------------------------------------------------------------- the raw entry points
def framed(device, count, dtype=torch.int32):
    """A buffer of `count` elements between two frames of PAD sentinels -> (whole buffer, pointer to the payload)."""
    whole = torch.full((count + 2 * PAD,), SENTINEL, dtype=dtype, device=device)
    return whole, ctypes.c_void_p(whole.data_ptr() + PAD * whole.element_size())


def unframed(whole, count):
    a = whole.cpu().numpy()
    assert (a[:PAD] == SENTINEL).all() and (a[PAD + count:] == SENTINEL).all(), 'a frame was written'
    return a[PAD:PAD + count].copy()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def on(device, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def raw_carve(device, returns, sensor, origins, counts, counts_too, mins=MINS, spacings=SPACINGS, stride_pad=0):
    """occ4d_evidence_carve_f32 of the loaded library with framed outputs -> dict of numpy arrays; the frames are checked."""
    nx, ny, nz = counts
    n, R = nx * ny * nz, len(returns)
    wide = np.full((R, 3 + stride_pad), np.nan, F32)
    wide[:, :3] = returns
    ret, org = on(device, wide), on(device, np.asarray(origins, I32).reshape(-1, 3))
    sen = None if sensor is None else on(device, np.asarray(sensor, I32))
    W = (n + 31) // 32
    bufs = dict(passed=framed(device, W), hits=framed(device, n), passes=framed(device, n) if counts_too else (None, None),
                status=framed(device, 4))
    rc_ = pk._lib.lib().occ4d_evidence_carve_f32(
        ptr(ret), 3 + stride_pad, R, ptr(sen), ptr(org), len(org), nx, ny, nz, mins[0], spacings[0], mins[1], spacings[1], mins[2],
        spacings[2], bufs['passed'][1], bufs['hits'][1], bufs['passes'][1], bufs['status'][1], pk.ops._stream())
    pk._lib.check(rc_)
    sizes = dict(passed=W, hits=n, passes=n, status=4)
    return {name: unframed(whole, sizes[name]) for name, (whole, _) in bufs.items() if whole is not None}


def raw_classify(device, field, level, hits, passed=None, passes=None, min_pass=1, mask=None, mask_level=0.0, ld=1):
    """occ4d_evidence_classify_f32 with framed outputs and a field column of stride ld -> (code, totals)."""
    n = len(hits)
    wide = np.full((max(n, 1), ld), np.nan, F32)
    wide[:n, 0] = field
    f, h = on(device, wide), on(device, np.asarray(hits, I32))
    m = None if mask is None else on(device, np.asarray(mask, F32))
    w = None if passed is None else on(device, np.asarray(passed, I32))
    ps = None if passes is None else on(device, np.asarray(passes, I32))
    code, totals = framed(device, n), framed(device, 6, torch.int64)
    rc_ = pk._lib.lib().occ4d_evidence_classify_f32(ptr(f), ld, level, ptr(m), 1, mask_level, n, ptr(w), ptr(ps), min_pass, ptr(h), code[1],
                                                    totals[1], pk.ops._stream())
    pk._lib.check(rc_)
    return unframed(code[0], n), unframed(totals[0], 6)


# ---------------------------------------------------------------------------------------------------------------- cases
def centre(cells, mins=MINS, spacings=SPACINGS):
    """The centres of lattice cells, float32 world points."""
    return (np.asarray(mins, np.float64) + (np.asarray(cells, np.float64) + 0.5) * np.asarray(spacings, np.float64)).astype(F32)


def scene(counts, R, V, rng, shift=0):
    """(returns (R, 3) float32, sensor (R,) int32, origins (V, 3) int32): returns uniform in the grid's box grown by a tenth (some
    fall outside: dropped), sensor v of placement PLACEMENTS[(v + shift) % 4]; half the returns of an 'own' sensor lie in its cell."""
    n3 = np.array(counts, np.float64)
    lo, ext = np.asarray(MINS, np.float64), n3 * np.asarray(SPACINGS, np.float64)
    returns = (lo + (rng.random((R, 3)) * 1.2 - 0.1) * ext).astype(F32)
    sensor = rng.integers(0, V, R).astype(I32)
    origins = np.zeros((V, 3), I32)
    for v in range(V):
        kind = PLACEMENTS[(v + shift) % 4]
        if kind in ('inside', 'own'):
            origins[v] = [rng.integers(0, c) for c in counts]
        elif kind == 'outside':
            origins[v] = [rng.integers(-3 * c - 2, 4 * c + 2) for c in counts]
            origins[v, rng.integers(0, 3)] = -2 - rng.integers(0, 9)
        else:
            origins[v] = [(-FAR, FAR)[rng.integers(0, 2)], rng.integers(-FAR, FAR + 1), rng.integers(0, counts[2])]
        if kind == 'own':
            mine = np.flatnonzero(sensor == v)[::2]
            returns[mine] = centre(origins[v])
    return returns, sensor, origins


def same_carve(got, want, counts_too, tag):
    names = ['passed', 'hits', 'status'] + (['passes'] if counts_too else [])
    assert sorted(got) == sorted(names), (tag, sorted(got))
    for name in names:
        assert got[name].dtype == I32 and np.array_equal(got[name], want[name]), (tag, name)


def matrix_cells(counts):
    return [(R, V) for R in RETURN_COUNTS for V in SENSOR_COUNTS]


def check_matrix(counts, device):
    """Per (R, V): the raw carve with framed outputs EQUAL to the restatement, twice, once more with the returns permuted, with and
    without counts (passes > 0 equals the bits), with a null sensor table (V == 1) and with a row stride; then the raw classify on
    a random field from the bits and from the counts.  -> the number of cells."""
    nx, ny, nz = counts
    n = nx * ny * nz
    rng = np.random.default_rng(4100 + n)
    done = 0
    for i, (R, V) in enumerate(matrix_cells(counts)):
        returns, sensor, origins = scene(counts, R, V, rng, shift=i)
        want = restate_carve(returns, sensor, origins, counts)
        assert want['status'].sum() == R
        assert np.array_equal(bits_of(want['passed'], n), want['passes'] > 0)
        tag = (counts, R, V)
        for counts_too in (False, True):
            first = raw_carve(device, returns, sensor, origins, counts, counts_too, stride_pad=i % 3)
            same_carve(first, want, counts_too, tag)
            again = raw_carve(device, returns, sensor, origins, counts, counts_too)
            same_carve(again, first, counts_too, tag)
            order = rng.permutation(R)
            moved = raw_carve(device, returns[order], sensor[order], origins, counts, counts_too)
            same_carve(moved, first, counts_too, tag)
        if V == 1:
            same_carve(raw_carve(device, returns, None, origins, counts, True), want, True, tag)
        field = rng.random(n).astype(F32)
        mask = rng.random(n).astype(F32)
        for kw in (dict(passed=want['passed']), dict(passes=want['passes']), dict(passes=want['passes'], min_pass=2),
                   dict(passed=want['passed'], mask=mask, mask_level=0.3)):
            expect = restate_classify(field, 0.6, want['hits'], **kw)
            code, totals = raw_classify(device, field, 0.6, want['hits'], ld=1 + i % 3, **kw)
            assert code.dtype == I32 and totals.dtype == I64 and np.array_equal(code, expect[0]) and np.array_equal(totals, expect[1]), (tag, sorted(kw))
            assert totals.sum() == n
        done += 1
    return done


def check_capacity_near_side(device, counts):
    """One carve against the restatement on a grid whose bit array a workgroup stages in LDS beyond the default 64 KiB: the
    published 96 x 96 x 58 (66 816 bytes) and 128 x 128 x 64 = 2^20 cells, exactly OCC4D_EVIDENCE_LDS_WORDS (128 KiB), the last
    grid on this side of the capacity rule.  1000 returns, three sensors (one inside), with counts, framed outputs."""
    n = counts[0] * counts[1] * counts[2]
    assert 64 * 1024 < 4 * ((n + 31) // 32) <= 4 * pk._lib.EVIDENCE_CONSTANTS['LDS_WORDS']
    rng = np.random.default_rng(n)
    returns, sensor, origins = scene(counts, 1000, 3, rng)
    want = restate_carve(returns, sensor, origins, counts)
    assert want['status'][0] > 500 and want['passes'].max() > 50
    same_carve(raw_carve(device, returns, sensor, origins, counts, True), want, True, counts)
    same_carve(raw_carve(device, returns, sensor, origins, counts, False), want, False, counts)


def carve_cells(device, counts, cells, origins, sensor=None, counts_too=True):
    """evidence.carve of returns at the centres of `cells` -> numpy dict, passed as (n,) bool."""
    n = counts[0] * counts[1] * counts[2]
    got = EV.carve(on(device, centre(np.asarray(cells).reshape(-1, 3))), np.asarray(origins, I32).reshape(-1, 3), counts, MINS, SPACINGS,
                   sensor=None if sensor is None else on(device, np.asarray(sensor, I32)), counts_too=counts_too)
    out = {k: t.cpu().numpy() for k, t in got.items()}
    out['passed'] = bits_of(out['passed'], n)
    return out


def flat_of(counts, cells):
    c = np.asarray(cells, I64).reshape(-1, 3)
    return (c[:, 0] * counts[1] + c[:, 1]) * counts[2] + c[:, 2]


def check_hand_worked(device):
    """The walks worked by hand from the header, on the 5 x 4 x 3 grid: (return cell, sensor cell, the cells passed in order)."""
    counts = (5, 4, 3)
    cases = [
        ((4, 1, 1), (0, 1, 1), [(3, 1, 1), (2, 1, 1), (1, 1, 1), (0, 1, 1)]),                       # an axis ray, the sensor's cell included
        ((0, 0, 0), (3, 3, 0), [(1, 1, 0), (2, 2, 0), (3, 3, 0)]),                                  # an exact face diagonal: edge ties, no side cell
        ((0, 0, 0), (2, 2, 2), [(1, 1, 1), (2, 2, 2)]),                                             # an exact space diagonal: corner ties
        ((2, 1, 1), (2, 1, 7), [(2, 1, 2)]),                                                        # leaves the grid before its sensor
        ((3, 2, 1), (6, 5, 1), [(4, 3, 1)]),                                                        # ... diagonally
        ((0, 0, 0), (4, 2, 0), [(1, 0, 0), (1, 1, 0), (2, 1, 0), (3, 1, 0), (3, 2, 0), (4, 2, 0)]),  # t_x = 1/8 3/8 5/8 7/8, t_y = 1/4 3/4
        ((4, 3, 2), (-FAR, 3, 2), [(3, 3, 2), (2, 3, 2), (1, 3, 2), (0, 3, 2)]),                    # 2^20 cells away, along the axis
        ((1, 2, 0), (1, 2, 0), []),                                                                 # e == o: a hit and nothing else
    ]
    for e, o, passed in cases:
        got = carve_cells(device, counts, [e], [o])
        want_hits, want_pass = np.zeros(60, I32), np.zeros(60, I32)
        want_hits[flat_of(counts, e)] = 1
        want_pass[flat_of(counts, passed)] = 1
        assert np.array_equal(got['hits'], want_hits) and np.array_equal(got['passes'], want_pass), (e, o)
        assert np.array_equal(got['passed'], want_pass > 0) and got['status'].tolist() == [1, 0, 0, 0], (e, o)
        restated = restate_carve(centre([e]), None, [o], counts)
        assert np.array_equal(restated['passes'], want_pass) and np.array_equal(restated['hits'], want_hits), (e, o)


def check_contention(device):
    """All 1000 returns in one cell from one sensor: hits == 1000 there, passes == 1000 along the one walk."""
    counts = (40, 40, 40)
    e, o = (37, 5, 21), (2, 30, 8)
    got = carve_cells(device, counts, [e] * 1000, [o])
    want = restate_carve(centre([e]), None, [o], counts)
    assert want['passes'].max() == 1 and want['passes'].sum() >= 35
    assert np.array_equal(got['hits'], 1000 * want['hits']) and np.array_equal(got['passes'], 1000 * want['passes'])
    assert np.array_equal(got['passed'], want['passes'] > 0) and got['status'].tolist() == [1000, 0, 0, 0]


def check_drops(device):
    """One return of each kind that falls out, among 200 that do not: status counts them in the stated priority, the rest of the
    output equals the run without them."""
    counts, V = (33, 2, 7), 3
    rng = np.random.default_rng(77)
    returns, sensor, origins = scene(counts, 200, V, rng)
    origins[:2] = [[5, 1, 3], [-4, 0, 9]]
    origins[2] = [FAR + 1, 0, 0]                                   # an origin row out of range
    sensor[sensor == 2] = 0
    inside = centre([[3, 1, 2]])[0]
    bad = np.array([[np.nan, inside[1], inside[2]], [inside[0], np.inf, inside[2]], [MINS[0] + SPACINGS[0] * (FAR + 2.5), inside[1], inside[2]],
                    [MINS[0] - 0.5 * SPACINGS[0], inside[1], inside[2]], inside, inside, inside,
                    [np.nan, inside[1], inside[2]], [MINS[0] - 0.5 * SPACINGS[0], np.nan, inside[2]]], F32)
    bad_sensor = np.array([0, 1, 0, 1, V, -1, 2, V, 0], I32)       # the last two: sensor before NaN, NaN before outside
    clean = raw_carve(device, returns, sensor, origins, counts, True)
    base = clean['status'].copy()
    assert base[1] == 0 and base[2] == 0 and base[0] > 100
    where = rng.permutation(209)
    both = raw_carve(device, np.concatenate([returns, bad])[where], np.concatenate([sensor, bad_sensor])[where], origins, counts, True)
    assert (both['status'] - base).tolist() == [0, 4, 4, 1]
    for name in ('passed', 'hits', 'passes'):
        assert np.array_equal(both[name], clean[name]), name
    want = restate_carve(np.concatenate([returns, bad]), np.concatenate([sensor, bad_sensor]), origins, counts)
    same_carve(both, want, True, 'drops')


def check_pinned_to_the_walk_of_sight(device):
    """For a return cell q and a sensor cell o, and every other cell c made the ONLY solid (one solid cell can never trigger the
    SQUEEZE): sight.look hides q from o exactly when c is PASSED by the carve of a return at q's centre from o.  `Other` leaves out q
    and o: sight never tests the origin's own cell (its rule 6), the carve passes it (the sensor stood there) -- asserted apart."""
    counts = (5, 4, 3)
    pairs = [((4, 3, 2), (0, 0, 0)), ((0, 0, 0), (3, 3, 0)), ((0, 1, 0), (2, 3, 2)), ((4, 0, 1), (0, 2, 1)), ((1, 3, 2), (4, 1, 0)),
             ((3, 2, 1), (-3, -4, 1)), ((2, 2, 2), (9, 9, 9)), ((0, 3, 0), (FAR, 3 - FAR, 0))]
    cells = [(x, y, z) for x in range(5) for y in range(4) for z in range(3)]
    n = len(cells)
    for q, o in pairs:
        passed = carve_cells(device, counts, [q], [o])['passed']
        field = np.zeros((n, n), F32)                              # column c: cell c the only solid
        field[np.arange(n), np.arange(n)] = 1.0
        dense = on(device, field)
        hidden = np.array([not bool(pk.sight.look(dense, counts, np.asarray([o], I32), 0.5, channel=c)[0][flat_of(counts, q)[0]].item() & 1)
                           for c in range(n)])
        other = np.array([c != q and c != o for c in cells])
        assert np.array_equal(hidden[other], passed[other]), (q, o)
        assert passed[other].any() or o == (9, 9, 9)               # (that walk leaves the grid with its first step)
        if o in cells:
            assert passed[flat_of(counts, o)[0]] and not hidden[flat_of(counts, o)[0]]
        assert not passed[flat_of(counts, q)[0]]


def check_seen_solids_contradict_nothing(device, share, seed):
    """A random `share`-solid 40^3 field; the returns are the centres of the solid cells that sight.look reports seen from o:
    nothing is CONTRADICTED, and the HIT cells are exactly those cells."""
    counts = (40, 40, 40)
    n = 64000
    rng = np.random.default_rng(seed)
    field = (rng.random(n) < share).astype(F32)
    o = np.array([[19, 22, 17]], I32)
    field[flat_of(counts, o)] = 0.0
    dense = on(device, field[:, None])
    seen = pk.sight.look(dense, counts, o, 0.5)[0].cpu().numpy() & 1
    target = (field >= 0.5) & (seen == 1)
    cells = np.stack(np.unravel_index(np.flatnonzero(target), counts), 1)
    assert 50 < len(cells) < target.size
    got = EV.observe(dense, counts, MINS, SPACINGS, on(device, centre(cells)), centre(o).astype(np.float64), level=0.5)
    totals, code, hits = (got[k].cpu().numpy() for k in ('totals', 'code', 'hits'))
    assert totals[EV.CONTRADICTED] == 0 and totals[EV.MISSED] == 0
    assert np.array_equal(hits > 0, target) and (hits[target] == 1).all()
    assert np.array_equal(code == EV.CONFIRMED_SOLID, target) and got['status'].cpu().numpy().tolist() == [len(cells), 0, 0, 0]
    assert totals[EV.CONFIRMED_FREE] > 0 and totals[EV.COMPLETED] > 0


def check_consequences(device):
    counts = (40, 40, 40)
    n = 64000
    rng = np.random.default_rng(5)
    returns, sensor, origins = scene(counts, 1000, 3, rng)
    origins[:] = [[3, 4, 5], [-7, 20, 44], [39, 39, 0]]
    field = np.stack([rng.random(n), rng.random(n)], 1).astype(F32)
    dense = on(device, field)
    world = centre(origins).astype(np.float64)
    want = restate_carve(returns, sensor, origins, counts)
    for kw in (dict(), dict(counts_too=True), dict(counts_too=True, min_pass=2), dict(select=(1, 0.4))):
        got = {k: t.cpu().numpy() for k, t in EV.observe(dense, counts, MINS, SPACINGS, on(device, returns), world, sensor=on(device, sensor),
                                                         level=0.7, **kw).items()}
        keys = ['code', 'hits'] + (['passes'] if kw.get('counts_too') else []) + ['totals', 'status']
        assert list(got) == keys
        expect = restate_classify(field[:, 0], 0.7, want['hits'], passed=None if kw.get('counts_too') else want['passed'],
                                  passes=want['passes'] if kw.get('counts_too') else None, min_pass=kw.get('min_pass', 1),
                                  mask=field[:, 1] if 'select' in kw else None, mask_level=0.4)
        assert np.array_equal(got['code'], expect[0]) and np.array_equal(got['totals'], expect[1])
        assert got['totals'].sum() == n and np.array_equal(got['totals'], np.bincount(got['code'], minlength=6))
        assert np.array_equal(got['hits'], want['hits']) and np.array_equal(got['status'], want['status'])
    for call in (lambda: EV.observe(dense, counts, MINS, SPACINGS, on(device, returns), world, min_pass=2),
                 lambda: EV.Evidence(returns, world, min_pass=2),
                 lambda: EV.classify(dense, 0.5, EV.carve(on(device, returns), origins, counts, MINS, SPACINGS), min_pass=2)):
        with pytest.raises(ValueError, match='min_pass = 2 needs counts=True'):
            call()
    # by_label against numpy
    K = 7
    labels = rng.integers(-2, K + 2, n).astype(I32)
    code = restate_classify(field[:, 0], 0.7, want['hits'], passed=want['passed'])[0]
    table = EV.by_label(on(device, labels), K, on(device, code))
    expect = np.zeros((K, 6), I64)
    keep = (labels >= 0) & (labels < K)
    np.add.at(expect, (labels[keep], code[keep]), 1)
    assert table.dtype == torch.int64 and np.array_equal(table.cpu().numpy(), expect)
    assert np.array_equal(table.sum(1).cpu().numpy(), np.bincount(labels[keep], minlength=K))
    assert tuple(EV.by_label(on(device, labels), 0, on(device, code)).shape) == (0, 6)


def check_rates():
    r = EV.rates(np.array([10, 20, 3, 8, 2, 6]))
    assert r['contradicted'] == 2 / 16 and r['missed'] == 3 / 9 and r['completed'] == 8 / 16
    r = EV.rates(torch.tensor([[5, 5, 0, 0, 0, 0], [0, 0, 4, 1, 1, 0]]))
    assert np.isnan(r['contradicted'][0]) and np.isnan(r['missed'][0]) and np.isnan(r['completed'][0])
    assert r['contradicted'][1] == 0.5 and r['missed'][1] == 1.0 and r['completed'][1] == 0.5 and r['missed'].dtype == np.float64
    with pytest.raises(ValueError, match='must be'):
        EV.rates(np.zeros(5))
    assert (EV.UNKNOWN_FREE, EV.CONFIRMED_FREE, EV.MISSED, EV.COMPLETED, EV.CONTRADICTED, EV.CONFIRMED_SOLID) == (0, 1, 2, 3, 4, 5)
    assert (EV.UNKNOWN, EV.FREE, EV.HIT) == (0, 1, 2)


def check_argument_errors(device):
    """The library's own checks through the wrappers (AssertionError with the contract's text)."""
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=device)
    with pytest.raises(AssertionError, match=r'V = 4097 must be in \[1, 4096\]'):
        pk.ops.grid_carve(z(2, 3), z(4097, 3, dtype=torch.int32), (2, 2, 2), MINS, SPACINGS)
    with pytest.raises(AssertionError, match='must be <= 512'):
        pk.ops.grid_carve(z(2, 3), z(1, 3, dtype=torch.int32), (513, 1, 1), MINS, SPACINGS)
    with pytest.raises(AssertionError, match='spacing = .* must be finite and > 0'):
        pk.ops.grid_carve(z(2, 3), z(1, 3, dtype=torch.int32), (2, 2, 2), MINS, (0.1, 0.0, 0.1))
    with pytest.raises(AssertionError, match='min_pass = 0 must be >= 1'):
        pk.ops.grid_evidence(z(8), 0.5, z(8, dtype=torch.int32), passes=z(8, dtype=torch.int32), min_pass=0)
    with pytest.raises(AssertionError, match='min_pass = 2 needs passes'):
        pk.ops.grid_evidence(z(8), 0.5, z(8, dtype=torch.int32), passed=z(1, dtype=torch.int32), min_pass=2)
    with pytest.raises(ValueError, match='V = 0 sensors'):
        EV.carve(z(2, 3), np.zeros((0, 3), I32), (2, 2, 2), MINS, SPACINGS)
    with pytest.raises(ValueError, match='beyond 2\\^20 cells'):
        EV.carve(z(2, 3), np.array([[FAR + 1, 0, 0]]), (2, 2, 2), MINS, SPACINGS)
    with pytest.raises(ValueError, match='returns must be'):
        EV.carve(z(2, 2), np.zeros((1, 3), I32), (2, 2, 2), MINS, SPACINGS)
    with pytest.raises(ValueError, match='sensor must be'):
        EV.carve(z(2, 3), np.zeros((1, 3), I32), (2, 2, 2), MINS, SPACINGS, sensor=np.zeros(3, I32))
    # an origins tensor on the device is taken as it is: the kernel drops what is out of range
    got = EV.carve(z(2, 3) + torch.tensor(centre([0, 0, 0]), device=device), torch.tensor([[FAR + 1, 0, 0]], dtype=torch.int32, device=device),
                   (2, 2, 2), MINS, SPACINGS)
    assert got['status'].cpu().numpy().tolist() == [0, 2, 0, 0] and not got['hits'].cpu().numpy().any()


def check_option():
    """Evidence's own checks, without a library."""
    E = EV.Evidence
    pts, org = np.zeros((5, 4), F32), np.zeros((2, 3))
    opt = E(pts, org, sensor=[0, 1, 1, 0, 1], counts=True, min_pass=3)
    assert opt.min_pass == 3 and opt.counts and opt.sensor.dtype == torch.int32 and opt.level is None and opt.select is None
    assert E.keyword == 'evidence' and E.clip_list[0] == 'evidences' and 'Evidence(R=5, V=2' in repr(opt) and issubclass(E, pk.products.LevelProduct)
    for args, kw, text in (((pts, np.zeros((0, 3))), {}, 'V = 0 sensors'), ((pts, np.zeros((4097, 3))), {}, 'V = 4097 sensors'),
                           ((pts, np.zeros((2, 2))), {}, 'origins must be'), ((np.zeros((5, 2), F32), org), {}, 'returns must be'),
                           ((pts, org), dict(sensor=[0, 1]), 'sensor must be'), ((pts, org), dict(sensor=np.zeros(5)), 'sensor must be'),
                           ((pts, org), dict(level=float('nan')), 'NaN'), ((pts, org), dict(min_pass=0), 'min_pass = 0'),
                           ((pts, org), dict(min_pass=2), 'needs counts=True'), ((pts, org), dict(select=3), 'select')):
        with pytest.raises(ValueError, match=text):
            E(*args, **kw)
    for phrase in ('TIMELESS', 'no sensor noise model and no beam width', 'maximum range', 'NOT MEASURED', 'There is no checkpoint'):
        assert phrase in ' '.join(EV.__doc__.split()), phrase


def check_signatures():
    """evidence stands directly in front of sweep in perform_inference, evidence and evidences in evaluate_clip."""
    names = list(inspect.signature(pk.inference.perform_inference).parameters)
    assert names[names.index('sweep') - 1] == 'evidence' and names[-9] == 'evidence'
    names = list(inspect.signature(pk.evaluation.evaluate_clip).parameters)
    assert names[names.index('sweep') - 2:names.index('sweep')] == ['evidence', 'evidences']
    for fn in (pk.inference.perform_inference, pk.evaluation.evaluate_clip):
        assert inspect.signature(fn).parameters['evidence'].default is None and 'evidence.Evidence' in fn.__doc__
    assert inspect.signature(pk.evaluation.evaluate_clip).parameters['evidences'].default is None
    assert 'evidence.Evidence' in pk.products.__doc__


# ---------------------------------------------------------------------------------------------------------------- end to end
COUNTS = rc.COUNTS


def fixture_option(shared, **kw):
    """600 returns in and round the fixture's query grid from three sensors: one inside it, two outside."""
    mins, spacings = yc.frame_of(shared)
    lo, hi = yc.hull(COUNTS, mins, spacings)
    mid, ext = 0.5 * (lo + hi), hi - lo
    rng = np.random.default_rng(31)
    returns = np.concatenate([(mid + (rng.random((600, 3)) - 0.5) * 1.15 * ext).astype(F32), rng.random((600, 2)).astype(F32)], 1)
    origins = np.stack([mid + 0.1 * ext, mid + np.array([-0.8, -0.5, 0.4]) * np.linalg.norm(ext), mid + np.array([0.1, 0.9, 0.2]) * ext])
    return EV.Evidence(returns, origins, sensor=rng.integers(0, 3, 600), **kw)


def without(result):
    return {k: v for k, v in result.items() if k not in ('components', 'evidence')}


def check_product(shared, got, option, level=0.5):
    """result['evidence'] EQUAL to evidence.observe on the call's own implicit_output and to the restatement."""
    mins, spacings = yc.frame_of(shared)
    ev, output = got['evidence'], got['implicit_output']
    keys = ['code', 'hits'] + (['passes'] if option.counts else []) + ['totals', 'status']
    assert list(ev) == keys and all(isinstance(a, np.ndarray) for a in ev.values()), list(ev)
    alone = EV.observe(torch.from_numpy(output).to(shared.device), COUNTS, mins, spacings, option.returns, option.origins, sensor=option.sensor,
                       level=level, select=option.select, counts_too=option.counts, min_pass=option.min_pass)
    assert list(alone) == keys
    for name in keys:
        a, b = ev[name], alone[name].cpu().numpy()
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    cells = pk.sight.grid_origin(option.origins, mins, spacings)
    want = restate_carve(option.returns.numpy(), option.sensor.numpy(), cells, COUNTS, mins, spacings)
    sel = option.select
    code, totals = restate_classify(output[:, 0], level, want['hits'], passed=None if option.counts else want['passed'],
                                    passes=want['passes'] if option.counts else None, min_pass=option.min_pass,
                                    mask=None if sel is None else output[:, sel[0]], mask_level=0.0 if sel is None else sel[1])
    assert np.array_equal(ev['code'], code) and np.array_equal(ev['totals'], totals) and ev['totals'].dtype == I64
    assert np.array_equal(ev['hits'], want['hits']) and np.array_equal(ev['status'], want['status'])
    assert ev['status'][0] > 300 and ev['status'][3] > 0 and ev['totals'].sum() == rc.N_QUERIES
    assert (ev['totals'][[EV.UNKNOWN_FREE, EV.CONFIRMED_FREE, EV.MISSED]] > 0).all() and ev['totals'][3:].sum() > 0


def check_end_to_end(shared, monkeypatch):
    device = shared.device
    option = fixture_option(shared)
    calls = rc.count_waits(monkeypatch)
    res = rc.infer(device, shared.inputs, evidence=option)
    assert calls['wait'] == 1                                    # exactly one host wait
    monkeypatch.undo()
    check_product(shared, res, option)
    assert sorted(without(res)) == sorted(shared.dense)
    same_result(without(res), shared.dense)                       # every other key is bit-equal with and without the option
    track = pk.inference.get_track_idx(shared.inputs[3]['color_mode'])
    option = fixture_option(shared, level=0.47, select=(track, 0.1), counts=True, min_pass=2)
    res = rc.infer(device, shared.inputs, evidence=option)
    check_product(shared, res, option, level=0.47)
    same_result(without(res), shared.dense)
    # beside components: by_label on the call's own labels
    comp = pk.components.Components()
    res = rc.infer(device, shared.inputs, components=comp, evidence=fixture_option(shared))
    labels, K = res['components']['labels'], len(res['components']['table'])
    table = EV.by_label(torch.from_numpy(labels).to(device), K, torch.from_numpy(res['evidence']['code']).to(device)).cpu().numpy()
    assert K > 0 and np.array_equal(table.sum(1), np.bincount(labels[labels >= 0], minlength=K)) and (table[:, :3] == 0).all()
    # under refine and in track_mode 'all': the expanded / merged array is what is classified
    option = fixture_option(shared, counts=True)
    plain = rc.infer(device, shared.inputs, refine=pk.inference.GridRefine(2, 0.46, 1))
    res = rc.infer(device, shared.inputs, refine=pk.inference.GridRefine(2, 0.46, 1), evidence=option)
    check_product(shared, res, option)
    same_result({k: v for k, v in without(res).items() if k != 'refine'}, {k: v for k, v in plain.items() if k != 'refine'})
    res = rc.infer(device, shared.inputs, track_mode='all', evidence=option)
    check_product(shared, res, option)
    same_result(without(res), shared.dense_all)


def check_clip(shared):
    """evaluate_clip(evidence=..., evidences=[]): one dict per output frame, that of the perform_inference call; the tuples as without."""
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = rc.clip_inputs(shared)
    run = lambda **kw: pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True, **kw)
    option, evidences = fixture_option(shared, counts=True), []
    clip = run(evidence=option, evidences=evidences)
    dense = run()
    assert len(clip) == len(dense) == len(evidences) == 2
    for t in range(2):
        for got, want in zip(clip[t], dense[t]):
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        res = pk.inference.perform_inference(
            pcl.clone(), None, frames[t], [enc, dec], shared.device, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], t, None,
            sample_implicit=True, num_sample=rc.CASE['num_sample'], point_sample_mode='grid', batch_size=rc.CASE['batch_size'],
            predict_segmentation=False, track_mode='none', semantic_classes=13, density_threshold=0.5, data_kind='greater',
            cube_mode=4, compress_air=True, point_occupancy_radius=0.8, evidence=option)
        assert list(evidences[t]) == list(res['evidence']) == ['code', 'hits', 'passes', 'totals', 'status']
        for name, a in evidences[t].items():
            assert np.array_equal(a, res['evidence'][name]), name
    with pytest.raises(ValueError, match='evidences'):
        run(evidence=option)
    with pytest.raises(ValueError, match='evidences=<a list>'):
        run(evidence=option, evidences=())


def check_none_is_untouched(shared, monkeypatch):
    """evidence=None: no new key, one host wait, and neither the ops nor the entry points are reached."""
    def forbidden(*a, **k):
        raise AssertionError('evidence=None must not reach the evidence entry points')
    monkeypatch.setattr(pk.ops, 'grid_carve', forbidden)
    monkeypatch.setattr(pk.ops, 'grid_evidence', forbidden)
    L = pk._lib.lib()
    for name in SYMBOLS:
        monkeypatch.setattr(L, name, forbidden)
    calls = rc.count_waits(monkeypatch)
    res = rc.infer(shared.device, shared.inputs, evidence=None)
    assert calls == dict(wait=1)
    assert sorted(res) == sorted(shared.dense)
    same_result(res, shared.dense)


def check_value_errors(shared):
    option = fixture_option(shared)
    with pytest.raises(ValueError, match='evidence must be a evidence.Evidence or None'):
        rc.infer(shared.device, shared.inputs, evidence=pk.components.Components())
    with pytest.raises(ValueError, match="evidence needs point_sample_mode 'grid'"):
        rc.infer(shared.device, shared.inputs, evidence=option, point_sample_mode='random')
    far = EV.Evidence(option.returns, np.array([[1e9, 0.0, 0.0]]))
    with pytest.raises(ValueError, match='beyond 2\\^20 cells'):
        rc.infer(shared.device, shared.inputs, evidence=far)
