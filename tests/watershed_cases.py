"""The case matrix of the watershed segments (include/ext/occ4d_watershed.h, ops.grid_watershed, watershed.py) and a numpy /
Python-integer RESTATEMENT of the header's rules, written from the header and not from the kernels: the ascent on shifted arrays,
pointer doubling on the whole array, a dict union-find over the basins.  tests/test_watershed_host.py runs the checks through the
g++ twin, tests/test_gpu_watershed.py on the device; everything is compared EQUAL, there is no tolerance."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import refine_cases as rc
import occlusions4d_amd as pk

SYMBOLS = ['occ4d_watershed_label_i32', 'occ4d_watershed_peaks_i32']
INT32_MAX = 2 ** 31 - 1
CANARY = -0x5a5a5a5b
CONNECTIVITIES = (6, 18, 26)
I32 = torch.int32


# ---------------------------------------------------------------------------------------------------------------- the restatement
def offsets(connectivity):
    """The neighbour offsets of ADJACENCY, in raster order."""
    rank = {6: 1, 18: 2, 26: 3}[connectivity]
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if 1 <= sum(x != 0 for x in d) <= rank]


def shifted(volume, d, fill):
    """out[i] = volume[i + d], `fill` outside."""
    pad = np.pad(volume, 1, constant_values=fill)
    nx, ny, nz = volume.shape
    return pad[1 + d[0]:1 + d[0] + nx, 1 + d[1]:1 + d[1] + ny, 1 + d[2]:1 + d[2] + nz]


def restate_basins(height, counts, connectivity):
    """-> (level (n,) int64: the height of a member, 0 else; basin (n,) int64: the flat index of the maximum, -1 for no member; the
    doubling rounds it took)."""
    n = int(np.prod(counts))
    level = np.where(height >= 1, height, 0).astype(np.int64).reshape(counts)
    index = np.arange(n, dtype=np.int64).reshape(counts)
    best_h, best_i = level.copy(), index.copy()
    for d in offsets(connectivity):
        h, i = shifted(level, d, 0), shifted(index, d, -1)
        above = (h >= 1) & ((h > best_h) | ((h == best_h) & (i < best_i)))          # ORDER
        best_h, best_i = np.where(above, h, best_h), np.where(above, i, best_i)
    up = np.where(level >= 1, best_i, -1).reshape(-1)
    members = np.flatnonzero(up >= 0)
    rounds = 0
    while True:
        nxt = up.copy()
        nxt[members] = up[up[members]]
        if np.array_equal(nxt, up):
            break
        up, rounds = nxt, rounds + 1
    assert rounds <= max(n - 1, 0).bit_length(), 'pointer doubling needs at most ceil(log2 n) rounds'
    return level.reshape(-1), up, rounds


def restate(height, counts, connectivity, h, min_size=1):
    """The header's outputs for one call, every row (no cap) -> dict(labels (n,) int32, totals (4,) int32, table (K, 12) int64, peaks
    (K, 2) int32, basin (n,) int64)."""
    n = int(np.prod(counts))
    if n == 0:
        return dict(labels=np.zeros(0, np.int32), totals=np.zeros(4, np.int32), table=np.zeros((0, 12), np.int64),
                    peaks=np.zeros((0, 2), np.int32), basin=np.zeros(0, np.int64))
    level, basin, _ = restate_basins(height, counts, connectivity)
    parent = {int(b): int(b) for b in np.unique(basin[basin >= 0])}

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    lv, bs = level.reshape(counts), basin.reshape(counts)
    for d in offsets(connectivity):
        if d <= (0, 0, 0):
            continue                                                   # each pair once: the forward half
        hq, bq = shifted(lv, d, 0), shifted(bs, d, -1)
        both = (lv >= 1) & (hq >= 1) & (bs != bq)
        a, b, low = bs[both], bq[both], np.minimum(lv[both], hq[both])
        related = np.minimum(level[a], level[b]) - low <= h             # MERGE (peak(B) = level[B])
        for x, y in set(zip(a[related].tolist(), b[related].tolist())):
            x, y = find(x), find(y)
            if x != y:
                parent[max(x, y)] = min(x, y)
    rep = np.full(n, -1, np.int64)
    member = basin >= 0
    lookup = {b: find(b) for b in parent}
    rep[member] = [lookup[b] for b in basin[member].tolist()]
    segments = {}                                                       # rep -> its points, ascending
    for p in np.flatnonzero(member).tolist():
        segments.setdefault(int(rep[p]), []).append(p)
    ordered = sorted(segments.values(), key=lambda pts: pts[0])         # increasing ROOT
    kept = [pts for pts in ordered if len(pts) >= min_size]
    labels = np.full(n, -1, np.int32)
    table, peaks = np.zeros((len(kept), 12), np.int64), np.zeros((len(kept), 2), np.int32)
    for k, pts in enumerate(kept):
        pts = np.asarray(pts, np.int64)
        labels[pts] = k
        xyz = np.stack(np.unravel_index(pts, counts), 1).astype(np.int64)
        table[k] = [len(pts), pts[0], -1, *xyz.sum(0), *xyz.min(0), *xyz.max(0)]
        top = level[pts].max()
        peaks[k] = [pts[level[pts] == top][0], top]                     # the highest under ORDER
    totals = np.array([len(kept), sum(len(p) for p in kept), len(ordered), len(parent)], np.int32)
    return dict(labels=labels, totals=totals, table=table, peaks=peaks, basin=basin)


def restate_components(member, counts, connectivity, key=None):
    """The connected components of a member set, numbered in the order of their lowest flat index, by minimum propagation -> (n,)
    int32, -1 for no member.  With `key` (n,): only neighbours of one key are joined."""
    n = int(np.prod(counts))
    member = member.reshape(counts)
    key = np.zeros(counts, np.int64) if key is None else key.astype(np.int64).reshape(counts)
    label = np.where(member, np.arange(n, dtype=np.int64).reshape(counts), n)
    for _ in range(n + 1):
        new = label
        for d in offsets(connectivity):
            new = np.minimum(new, np.where(shifted(key, d, -2) == key, shifted(label, d, n), n))
        new = np.where(member, new, n)
        flat = new.reshape(-1)                                          # ... and a jump to the label's own label
        new = np.where(member, flat[np.minimum(new, n - 1)].reshape(counts), n)
        if np.array_equal(new, label):
            break
        label = new
    roots = np.unique(label[member])
    return np.where(member, np.searchsorted(roots, label), -1).astype(np.int32).reshape(-1)


def depth2(member, counts):
    """inside2 of distance.Clearance by brute force: per member the squared distance to the nearest non-member of the grid (a
    non-member beside a member: the nearest one always is), INT32_MAX without one; 0 for a non-member."""
    member = member.reshape(counts)
    out = np.zeros(counts, np.int64)
    if member.all():
        out[:] = INT32_MAX
        return out.reshape(-1).astype(np.int32)
    beside = np.zeros(counts, bool)
    for d in offsets(26):
        beside |= shifted(member, d, False)
    shell = np.argwhere(~member & beside).astype(np.int64)
    inner = np.argwhere(member).astype(np.int64)
    if len(inner):
        d2 = ((inner[:, None, :] - shell[None, :, :]) ** 2).sum(2).min(1)
        out[tuple(inner.T)] = d2
    return out.reshape(-1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- the cases
def _random(counts, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(counts))
    member = rng.random(n) < 0.8
    return np.where(member, rng.integers(1, 4, n), rng.integers(-2, 1, n)).astype(np.int32)       # many ties; negatives are no members


def _slab():
    """A 20 x 3 x 3 slab in 24 x 7 x 7: its inside2 is a ridge plateau of height 4 that crosses two tile borders."""
    counts = (24, 7, 7)
    member = np.zeros(counts, bool)
    member[2:22, 2:5, 2:5] = True
    return counts, depth2(member, counts)


def _u_plateau():
    """A U of one height in 9 x 10 x 11: both arms end in an index maximum of their own, joined at the far side."""
    counts = (9, 10, 11)
    h = np.zeros(counts, np.int32)
    h[4, 1:9, 2] = 7
    h[4, 1:9, 8] = 7
    h[4, 8, 2:9] = 7
    return counts, h.reshape(-1)


def _serpentine():
    """A corridor of one height through 16 x 16 x 16: rows joined at alternating ends, planes joined at alternating corners -- the
    longest chain, and at connectivity 6 a single path of over 1000 points."""
    counts = (16, 16, 16)
    h = np.zeros(counts, np.int32)
    for ix in range(0, 16, 2):
        for iy in range(0, 16, 2):
            h[ix, iy, :] = 5
            if iy + 1 < 15:
                h[ix, iy + 1, 15 if (iy // 2) % 2 == 0 else 0] = 5
        if ix + 1 < 15:
            h[ix + 1, 14 if (ix // 2) % 2 == 0 else 0, 0] = 5
    return counts, h.reshape(-1)


def _checkerboard():
    counts = (9, 10, 11)
    ix, iy, iz = np.indices(counts)
    return counts, np.where((ix + iy + iz) % 2 == 0, 2, 0).astype(np.int32).reshape(-1)


def _balls():
    """Two balls of radius 8 whose centres lie 13 apart, in 40 x 32 x 32: their inside2."""
    counts = (40, 32, 32)
    ix, iy, iz = np.indices(counts)
    member = np.zeros(counts, bool)
    for cx in (13, 26):
        member |= (ix - cx) ** 2 + (iy - 16) ** 2 + (iz - 16) ** 2 <= 64
    return counts, depth2(member, counts)


def _single():
    h = np.zeros(9 * 10 * 11, np.int32)
    h[517] = 3
    return (9, 10, 11), h


def _case(name, counts, height, min_sizes=(1,)):
    height = np.ascontiguousarray(height, np.int32)
    height.setflags(write=False)
    top = int(height.max()) if height.size else 0
    hs = sorted({0, 1, 2, max(top, 0)})
    return dict(name=name, counts=tuple(counts), height=height, hs=hs, min_sizes=min_sizes)


CASES = [_case('random-%dx%dx%d' % c, c, _random(c, 10 + i), (1, 5) if min(c) > 1 else (1,))
         for i, c in enumerate([(9, 10, 11), (17, 8, 9), (16, 16, 16), (1, 1, 30), (30, 1, 1), (1, 7, 1), (1, 1, 1)])]
CASES += [
    _case('empty-0x5x5', (0, 5, 5), np.zeros(0, np.int32)),
    _case('all-int32-max', (9, 10, 11), np.full(990, INT32_MAX, np.int32)),
    _case('all-zero', (9, 10, 11), np.zeros(990, np.int32)),
    _case('single-member', *_single()),
    _case('slab-ridge', *_slab()),
    _case('u-plateau', *_u_plateau()),
    _case('serpentine', *_serpentine()),
    _case('checkerboard', *_checkerboard()),
]
BY_NAME = {c['name']: c for c in CASES}
NAMES = list(BY_NAME)
CAP_CASE = 'random-9x10x11'
BALLS = _case('two-balls', *_balls())


@functools.lru_cache(maxsize=None)
def expected(name, connectivity, h, min_size=1):
    """The restatement of one call of a case: computed once, shared, never changed."""
    c = BALLS if name == 'two-balls' else BY_NAME[name]
    out = restate(c['height'], c['counts'], connectivity, h, min_size)
    for v in out.values():
        v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- running a call
def tensor_of(height, device):
    return torch.from_numpy(np.array(height, np.int32)).to(device)           # (a copy: the cases are read-only)


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def run_raw(L, device, height, counts, connectivity, h, min_size=1, cap=None):
    """The three entry points on the plain library handle `L` with tensors of `device` (the HIP library and the device, or the twin
    and the host), every buffer with a canary word or row behind it.  cap None: K = totals[0] is read first.  -> numpy dict(labels,
    totals, table, peaks), the rows below min(cap, K); asserts that nothing else was written."""
    nx, ny, nz = counts
    n = nx * ny * nz
    hgt = tensor_of(height, device)
    full = lambda shape, dtype=I32: torch.full(shape, CANARY, dtype=dtype, device=device)
    work, labels, totals = full((pk.ops.watershed_work_len(n) + 1,)), full((n + 1,)), full((5,))
    assert L.occ4d_watershed_label_i32(ptr(hgt) if n else None, nx, ny, nz, connectivity, h, min_size, ptr(work), ptr(labels), ptr(totals),
                                       None) == pk._lib.OK
    got_totals = totals.cpu().numpy()
    if n == 0:
        assert (got_totals == CANARY).all() and (labels.cpu().numpy() == CANARY).all()                # a no-op
        got_totals = np.concatenate([np.zeros(4, np.int32), got_totals[4:]])
        totals[:4] = 0
    assert got_totals[4] == CANARY and work[-1].item() == CANARY and labels[n].item() == CANARY
    kept = int(got_totals[0])
    cap = kept if cap is None else cap
    table, peaks = full((cap + 1, 12), torch.int64), full((cap + 1, 2))
    assert L.occ4d_components_table_i64(ptr(labels), None, nx, ny, nz, ptr(totals), ptr(table), cap, None) == pk._lib.OK
    assert L.occ4d_watershed_peaks_i32(ptr(hgt) if n else None, ptr(labels), n, ptr(totals), ptr(peaks), cap, None) == pk._lib.OK
    rows = min(cap, kept)
    table, peaks = table.cpu().numpy(), peaks.cpu().numpy()
    assert (table[rows:] == CANARY).all() and (peaks[rows:] == CANARY).all(), 'rows past min(cap, K) were written'
    return dict(labels=labels.cpu().numpy()[:n], totals=got_totals[:4], table=table[:rows], peaks=peaks[:rows])


def run_ops(device, height, counts, connectivity, h, min_size=1, cap=None):
    """ops.grid_watershed on the loaded library -> numpy dict(labels, totals, table, peaks)."""
    out = pk.ops.grid_watershed(tensor_of(height, device), counts, h, connectivity, min_size, cap)
    assert [t.dtype for t in out] == [I32, I32, torch.int64, I32] and all(t.device.type == torch.device(device).type for t in out)
    return dict(zip(('labels', 'totals', 'table', 'peaks'), (t.cpu().numpy() for t in out)))


def same(got, want, what, rows=None):
    for key in ('labels', 'totals', 'table', 'peaks'):
        w = want[key] if rows is None or key in ('labels', 'totals') else want[key][:rows]
        assert got[key].dtype == w.dtype and got[key].shape == w.shape and np.array_equal(got[key], w), (what, key)


def calls_of(c):
    return [(conn, h, m) for conn in CONNECTIVITIES for h in c['hs'] for m in c['min_sizes']]


# ---------------------------------------------------------------------------------------------------------------- the checks
def check(name, device, twin_handle=None):
    """Every call of a case through ops.grid_watershed, twice with equal bits, EQUAL to the restatement; with `twin_handle` (a plain
    handle of the g++ twin beside the HIP library) also bit-equal to the twin on host arrays."""
    c = BY_NAME[name]
    for conn, h, m in calls_of(c):
        want = expected(name, conn, h, m)
        what = '%s c%d h%d m%d' % (name, conn, h, m)
        got = run_ops(device, c['height'], c['counts'], conn, h, m)
        same(got, want, what)
        same(run_ops(device, c['height'], c['counts'], conn, h, m), got, what + ' again')
        if twin_handle is not None:
            same(run_raw(twin_handle, 'cpu', c['height'], c['counts'], conn, h, m), got, what + ' twin')


def check_by_hand():
    """The restatement on cases small enough to work out on paper."""
    # a line 3 1 2 2 -1 5: 0 climbs to itself (a maximum), 1 -> 0, 2 is a maximum (tie with 3: the lower index), 3 -> 2, 5 alone
    line = np.array([3, 1, 2, 2, -1, 5], np.int32)
    level, basin, _ = restate_basins(line, (1, 1, 6), 6)
    assert level.tolist() == [3, 1, 2, 2, 0, 5] and basin.tolist() == [0, 0, 2, 2, -1, 5]
    # basins 0 and 2 meet at the pair (1, 2): min(3, 2) - min(1, 2) = 1
    r = restate(line, (1, 1, 6), 6, 0)
    assert r['labels'].tolist() == [0, 0, 1, 1, -1, 2] and r['totals'].tolist() == [3, 5, 3, 3]
    assert r['peaks'].tolist() == [[0, 3], [2, 2], [5, 5]] and r['table'][:, :2].tolist() == [[2, 0], [2, 2], [1, 5]]
    r = restate(line, (1, 1, 6), 6, 1)
    assert r['labels'].tolist() == [0, 0, 0, 0, -1, 1] and r['totals'].tolist() == [2, 5, 2, 3] and r['peaks'].tolist() == [[0, 3], [5, 5]]
    r = restate(line, (1, 1, 6), 6, 1, min_size=2)
    assert r['labels'].tolist() == [0, 0, 0, 0, -1, -1] and r['totals'].tolist() == [1, 4, 2, 3]
    # a plateau 4 4 4 4: every point climbs one step down the index; one basin after doubling
    assert restate_basins(np.full(4, 4, np.int32), (1, 1, 4), 6)[1].tolist() == [0, 0, 0, 0]
    # the checkerboard and the serpentine as the issue describes them
    board = BY_NAME['checkerboard']
    assert expected('checkerboard', 6, 0)['totals'][0] == (board['height'] >= 1).sum() and expected('checkerboard', 26, 0)['totals'][0] == 1
    for conn in CONNECTIVITIES:
        assert expected('serpentine', conn, 0)['totals'][[0, 2]].tolist() == [1, 1] and expected('u-plateau', conn, 0)['totals'][0] == 1
        assert expected('u-plateau', conn, 0)['totals'][3] > 1 and expected('all-int32-max', conn, 0)['totals'][:3].tolist() == [1, 990, 1]
        assert expected('all-zero', conn, 0)['totals'].tolist() == [0, 0, 0, 0] and expected('single-member', conn, 2)['peaks'].tolist() == [[517, 3]]
    snake = BY_NAME['serpentine']
    assert restate_components(snake['height'] >= 1, snake['counts'], 6).max() == 0 and (snake['height'] >= 1).sum() > 1000
    assert restate_basins(snake['height'], snake['counts'], 6)[2] >= 5                     # a chain that needs its doubling rounds
    ridge = expected('slab-ridge', 26, 0)
    assert ridge['totals'][0] == 1 and ridge['peaks'].tolist() == [[(3 * 7 + 3) * 7 + 3, 4]]


def check_consequences(name, device):
    """(a) h >= the largest height, min_size 1: the labels of ops.grid_components of the same member set, numbering included, which
    is scipy.ndimage.label - 1; (b) every segment is connected; (c) the segments at h1 <= h2 nest; (d) no segment spans two
    components -- on what the LIBRARY returns, with yardsticks of their own."""
    c = BY_NAME[name]
    n = int(np.prod(c['counts']))
    member = c['height'] >= 1
    for conn in CONNECTIVITIES:
        comps = restate_components(member, c['counts'], conn)
        by_h = [run_ops(device, c['height'], c['counts'], conn, h)['labels'] for h in c['hs']]
        values = torch.from_numpy(np.where(member, 1.0, 0.0).astype(np.float32)).to(device)
        got = pk.ops.grid_components(values, c['counts'], 0.5, conn)[0].cpu().numpy()
        assert np.array_equal(by_h[-1], got) and np.array_equal(got, comps), (name, conn, 'a')
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
        if ndimage is not None and n:
            structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn])
            assert np.array_equal(by_h[-1], ndimage.label(member.reshape(c['counts']), structure)[0].reshape(-1).astype(np.int32) - 1), (name, conn)
        for labels in by_h:
            assert ((labels >= 0) == member).all()
            k = labels.max() + 1 if n else 0
            # (b): the components of "same segment" are as many as the segments
            parts = restate_components(member, c['counts'], conn, key=labels)
            assert (parts.max() + 1 if n else 0) == k, (name, conn, 'b')
            # (d): a segment lies in one component
            assert len({(s, q) for s, q in zip(labels[member].tolist(), comps[member].tolist())}) == k, (name, conn, 'd')
        for lo, hi in zip(by_h, by_h[1:]):                              # (c)
            assert len({(s, q) for s, q in zip(lo[member].tolist(), hi[member].tolist())}) == (lo.max() + 1 if n else 0), (name, conn, 'c')


def check_caps(device, L, loaded=True):
    """cap below, at and above K, and 0: the rows below min(cap, K) are the restatement's, the others untouched (run_raw's canaries).
    L: a plain handle that takes tensors of `device`; loaded: it is the library ops calls."""
    c = BY_NAME[CAP_CASE]
    want = expected(CAP_CASE, 6, 1)
    kept = int(want['totals'][0])
    assert kept > 4
    for cap in (0, 1, kept - 1, kept, kept + 3):
        got = run_raw(L, device, c['height'], c['counts'], 6, 1, 1, cap)
        same(got, want, 'cap %d' % cap, rows=min(cap, kept))
    if loaded:
        got = run_ops(device, c['height'], c['counts'], 6, 1, 1, cap=kept + 2)
        assert got['table'].shape == (kept + 2, 12) and got['peaks'].shape == (kept + 2, 2)
        assert np.array_equal(got['table'][:kept], want['table']) and np.array_equal(got['peaks'][:kept], want['peaks'])
    # foreign labels: a row number outside [0, min(cap, totals[0])) touches nothing, a row no member names reads (-1, 0)
    n = int(np.prod(c['counts']))
    hgt = tensor_of(c['height'], device)
    labels = torch.from_numpy(np.where(np.arange(n) % 3 == 0, 2 ** 31 - 1, np.where(np.arange(n) % 3 == 1, -7, 1)).astype(np.int32)).to(device)
    totals = torch.tensor([3, 0, 0, 0], dtype=I32, device=device)
    peaks = torch.full((5, 2), CANARY, dtype=I32, device=device)
    assert L.occ4d_watershed_peaks_i32(ptr(hgt), ptr(labels), n, ptr(totals), ptr(peaks), 4, None) == pk._lib.OK
    rows = peaks.cpu().numpy()
    members = np.flatnonzero((np.arange(n) % 3 == 2) & (c['height'] >= 1))
    top = c['height'][members].max()
    assert rows[0].tolist() == [-1, 0] and rows[2].tolist() == [-1, 0] and (rows[3:] == CANARY).all()
    assert rows[1].tolist() == [members[c['height'][members] == top][0], top]


def check_balls(device, twin_handle=None):
    """Two touching balls: two segments below the flip the RESTATEMENT gives, one from it on."""
    c = BALLS
    lo, hi = 0, int(c['height'].max())
    assert expected('two-balls', 26, lo)['totals'][0] == 2 and expected('two-balls', 26, hi)['totals'][0] == 1
    while hi - lo > 1:                                                  # (the segments nest in h: a bisection)
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if expected('two-balls', 26, mid)['totals'][0] == 2 else (lo, mid)
    flip = hi
    assert 20 < flip <= 40, flip                                        # where the prototype of the rules saw it
    for h, k in ((flip - 1, 2), (flip, 1)):
        want = expected('two-balls', 26, h)
        got = run_ops(device, c['height'], c['counts'], 26, h)
        assert got['totals'][0] == k
        same(got, want, 'two-balls h%d' % h)
        if twin_handle is not None:
            same(run_raw(twin_handle, 'cpu', c['height'], c['counts'], 26, h), got, 'two-balls twin')
    centre = (13 * 32 + 16) * 32 + 16                                   # the first ball's: the lower index of two equal depths
    assert got['peaks'].tolist() == [[centre, c['height'][centre]]] and c['height'][centre] == c['height'].max()


def check_argument_errors(device):
    c = BY_NAME['random-9x10x11']
    hgt = tensor_of(c['height'], device)
    for kw, text in ((dict(connectivity=8), 'connectivity = 8 must be 6, 18 or 26'), (dict(h=-1), 'h = -1 must be >= 0'),
                     (dict(min_size=0), 'min_size = 0 must be >= 1')):
        with pytest.raises(AssertionError, match=text):
            pk.ops.grid_watershed(hgt, c['counts'], **dict(dict(h=0), **kw))
    with pytest.raises(AssertionError, match='height must be'):
        pk.ops.grid_watershed(hgt[:-1], c['counts'], 0)
    with pytest.raises(AssertionError):
        pk.ops.grid_watershed(hgt.to(torch.float32), c['counts'], 0)
    with pytest.raises(AssertionError, match='cap = -1'):
        pk.ops.grid_watershed(hgt, c['counts'], 0, cap=-1)
    assert pk.ops.grid_watershed(hgt, c['counts'], INT32_MAX)[1][0] >= 1


# ---------------------------------------------------------------------------------------------------------------- end to end
def without(result):
    return {k: v for k, v in result.items() if k != 'segments'}


def split_of(result, device, option, counts=rc.COUNTS):
    """watershed.split on the output a call returned -> numpy (labels, table, peaks)."""
    out = torch.from_numpy(result['implicit_output']).to(device)
    level = 0.5 if option.level is None else option.level
    return [t.cpu().numpy() for t in pk.watershed.split(out, counts, level, option.h, option.select, option.weights, option.connectivity,
                                                        option.min_size)]


def check_result(result, device, option):
    seg = result['segments']
    assert sorted(seg) == ['labels', 'peaks', 'table'] and all(isinstance(v, np.ndarray) for v in seg.values())
    for got, want in zip((seg['labels'], seg['table'], seg['peaks']), split_of(result, device, option)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    # ... and the restatement of the whole product: the brute-force depth of the solid set, then the rules
    member = result['implicit_output'][:, 0] >= np.float32(0.5 if option.level is None else option.level)
    assert option.weights == (1, 1, 1) and option.select is None
    want = restate(depth2(member, rc.COUNTS), rc.COUNTS, option.connectivity, option.h, option.min_size)
    assert np.array_equal(seg['labels'], want['labels']) and np.array_equal(seg['table'], want['table']) and np.array_equal(seg['peaks'], want['peaks'])
    return want


def check_end_to_end(shared):
    option = pk.watershed.Segments(h=0)
    got = rc.infer(shared.device, shared.inputs, segments=option)
    want = check_result(got, shared.device, option)
    assert want['totals'][0] >= 1 and (got['segments']['labels'] >= 0).sum() == (shared.dense['implicit_output'][:, 0] >= 0.5).sum()
    rc.same_result(without(got), shared.dense)                          # implicit_output and the rest: unchanged
    option = pk.watershed.Segments(2, connectivity=6, min_size=3)
    got = rc.infer(shared.device, shared.inputs, segments=option, components=pk.components.Components(connectivity=6))
    check_result(got, shared.device, option)
    rc.same_result({k: v for k, v in without(got).items() if k != 'components'}, shared.dense)
    # a large h and min_size 1: the components of the same call
    option = pk.watershed.Segments(INT32_MAX, connectivity=6)
    got = rc.infer(shared.device, shared.inputs, segments=option, components=pk.components.Components(connectivity=6))
    assert np.array_equal(got['segments']['labels'], got['components']['labels']) and np.array_equal(got['segments']['table'], got['components']['table'])
    # under refine and in track_mode 'all': the segments of the array the call returns
    option = pk.watershed.Segments(1)
    got = rc.infer(shared.device, shared.inputs, refine=pk.inference.GridRefine(2, 0.46, 1), segments=option)
    check_result(got, shared.device, option)
    got = rc.infer(shared.device, shared.inputs, track_mode='all', segments=option)
    check_result(got, shared.device, option)
    rc.same_result(without(got), shared.dense_all)


def check_clip(shared):
    """evaluate_clip(segments=..., parts=[]) over two frames: one dict per frame, that of the perform_inference call."""
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = rc.clip_inputs(shared)
    option, parts = pk.watershed.Segments(1), []
    clip = pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True, segments=option, parts=parts)
    dense = pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True)
    assert len(clip) == len(dense) == len(parts) == 2
    for t in range(2):
        for got, want in zip(clip[t], dense[t]):
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        assert sorted(parts[t]) == ['labels', 'peaks', 'table'] and parts[t]['labels'].shape == (rc.N_QUERIES,)
        assert parts[t]['table'].shape[0] == parts[t]['peaks'].shape[0] == parts[t]['labels'].max() + 1
    with pytest.raises(ValueError, match='parts'):
        pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', segments=option)
    with pytest.raises(ValueError, match='segments must be a watershed.Segments'):
        pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', segments=1, parts=[])


def check_none_is_untouched(shared, monkeypatch):
    """segments=None: no new key and no entry point called; with segments still one host wait."""
    def forbidden(*a, **k):
        raise AssertionError('segments=None must not reach the watershed entry points')
    monkeypatch.setattr(pk.ops, 'grid_watershed', forbidden)
    L = pk._lib.lib()
    for name in SYMBOLS:
        monkeypatch.setattr(L, name, forbidden)
    res = rc.infer(shared.device, shared.inputs, segments=None)
    assert sorted(res) == sorted(shared.dense)
    rc.same_result(res, shared.dense)
    monkeypatch.undo()
    calls = rc.count_waits(monkeypatch)
    rc.infer(shared.device, shared.inputs, segments=pk.watershed.Segments(1))
    assert calls['wait'] == 1


def check_value_errors(shared):
    with pytest.raises(ValueError, match="segments needs point_sample_mode 'grid'"):
        rc.infer(shared.device, shared.inputs, segments=pk.watershed.Segments(1), point_sample_mode='random')
    with pytest.raises(ValueError, match='segments must be a watershed.Segments or None'):
        rc.infer(shared.device, shared.inputs, segments=4)


def check_compositions(device):
    """What works as it is on segments: boxes_and_centroids, expand_labels, Tracker.add_frame by hand."""
    c = BY_NAME['random-16x16x16']
    hgt = tensor_of(c['height'], device)
    labels, totals, table, peaks = pk.ops.grid_watershed(hgt, c['counts'], 1, 26)
    want = expected(c['name'], 26, 1)
    summary = pk.components.boxes_and_centroids(table, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert np.array_equal(summary['size'], want['table'][:, 0]) and (summary['klass'] == -1).all()
    assert np.array_equal(summary['box_min'], want['table'][:, 6:9] + 0.5) and np.array_equal(summary['box_max'], want['table'][:, 9:12] + 0.5)
    values = (hgt >= 1).to(torch.float32)
    nearest = pk.ops.grid_distance(values, c['counts'], 0.5, nearest=True)[1]
    region = pk.distance.expand_labels(labels, nearest).cpu().numpy()
    member = c['height'] >= 1
    assert np.array_equal(region[member], want['labels'][member]) and (region >= 0).all() and region.dtype == np.int32
    tracker = pk.components.Tracker()
    first = tracker.add_frame(labels, table).cpu().numpy()
    k = table.shape[0]
    assert first.shape == (k, 4) and first[:, 0].tolist() == list(range(k)) and (first[:, 1] == -1).all()
    # the next frame: the same field split with a larger h -- every segment continues one of the frame before, or is new
    labels2, _, table2, _ = pk.ops.grid_watershed(hgt, c['counts'], 2, 26)
    second = tracker.add_frame(labels2, table2).cpu().numpy()
    assert second.shape == (table2.shape[0], 4) and tracker.n_tracks() >= k
    again = tracker.add_frame(labels2, table2).cpu().numpy()            # an unchanged frame: every segment continues itself
    assert again[:, 1].tolist() == list(range(table2.shape[0])) and np.array_equal(again[:, 0], second[:, 0])
    assert np.array_equal(again[:, 3], table2.cpu().numpy()[:, 0])
