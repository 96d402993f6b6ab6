"""The case matrix of the line of sight through the solid set (include/ext/occ4d_sight.h, ops.grid_solid_bits / ops.grid_sight,
sight.py) and two RESTATEMENTS of the header's rules, written from the header and not from csrc/sight_math.hpp: a scalar one in
Python integers (the supercover walk with products, the SQUEEZE by enumerating the orders of T), and a vectorised numpy int64 one
with all queries in lockstep, which must first agree with the scalar one on every grid of at most 1000 points.
tests/test_sight_host.py runs the checks through the g++ twin, tests/test_gpu_sight.py on the device; everything is compared EQUAL,
there is no tolerance."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import raycast_cases as yc
import refine_cases as rc
import occlusions4d_amd as pk

SYMBOLS = ['occ4d_sight_bits_f32', 'occ4d_sight_grid_u32']
CANARY = -0x5a5a5a5b
I32 = torch.int32
FAR = 2 ** 20
FLAGS = (0,)                          # one variant of the walk kernel stayed (bits in global memory): `flags` must be 0


# ---------------------------------------------------------------------------------------------------------------- the restatements
def flat_of(counts, c):
    return (c[0] * counts[1] + c[1]) * counts[2] + c[2]


def inside(counts, c):
    return all(0 <= c[a] < counts[a] for a in range(3))


def walk_scalar(solid, counts, q, o):
    """THE WALK of the header from the query q to the origin o over solid (nx, ny, nz) bool -> -1: seen, else the blocker's flat
    index.  Python integers."""
    is_solid = lambda c: inside(counts, c) and bool(solid[tuple(c)])                 # a lattice point outside the grid is free
    d = [o[a] - q[a] for a in range(3)]
    s = [(x > 0) - (x < 0) for x in d]
    m = [abs(x) for x in d]
    c, j = list(q), [0, 0, 0]
    if not any(m):
        return -1
    for _ in range(sum(counts)):
        live = [a for a in range(3) if j[a] < m[a]]                                  # 1.
        T = [a for a in live if all((2 * j[a] + 1) * m[b] <= (2 * j[b] + 1) * m[a] for b in live)]      # 2., 3.: t_a <= t_b for all b
        if len(T) >= 2:                                                              # 4. SQUEEZE
            passes, cells = False, []
            for order in itertools.permutations(T):
                cur, between = list(c), []
                for a in order[:-1]:
                    cur[a] += s[a]
                    between.append(tuple(cur))
                cells += between
                passes = passes or not any(is_solid(x) for x in between)
            if not passes:
                return min(flat_of(counts, x) for x in cells if is_solid(x))
        for a in T:                                                                  # 5.
            c[a] += s[a]
            j[a] += 1
        if c == list(o):                                                             # 6.
            return -1
        if not inside(counts, c):                                                    # 7.
            return -1
        if solid[tuple(c)]:                                                          # 8.
            return flat_of(counts, c)
    raise AssertionError('the walk from %r to %r did not end within nx + ny + nz steps' % (q, o))


def blockers_scalar(solid, counts, origin):
    """(n,) int64: walk_scalar of every query towards one origin."""
    return np.array([walk_scalar(solid, counts, q, origin) for q in itertools.product(*(range(c) for c in counts))], np.int64).reshape(-1)


def blockers_lockstep(solid, counts, origin):
    """The same, all queries in lockstep on numpy int64 arrays."""
    counts_a = np.asarray(counts, np.int64)
    n = int(np.prod(counts))
    flat_solid = np.asarray(solid, bool).reshape(-1)
    BIG = np.int64(2 ** 62)

    def probe(cells):
        """cells (k, 3) -> (solid (k,) bool, flat (k,) int64 where inside)."""
        ok = ((cells >= 0) & (cells < counts_a)).all(1)
        flat = (cells[:, 0] * counts_a[1] + cells[:, 1]) * counts_a[2] + cells[:, 2]
        sol = np.zeros(len(cells), bool)
        sol[ok] = flat_solid[flat[ok]]
        return sol, flat

    q = np.stack(np.unravel_index(np.arange(n, dtype=np.int64), counts), 1).astype(np.int64)
    o = np.asarray(origin, np.int64)
    d = o[None, :] - q
    s, m = np.sign(d), np.abs(d)
    result = np.full(n, -1, np.int64)
    alive = np.flatnonzero(m.any(1))                                                 # (every m_a = 0: seen)
    c, j = q[alive].copy(), np.zeros((len(alive), 3), np.int64)
    s, m = s[alive], m[alive]
    for _ in range(sum(counts)):
        if not len(alive):
            break
        live = j < m
        k = 2 * j + 1
        in_t = live.copy()
        for a in range(3):
            for b in range(3):
                if a != b:                                                           # a is beaten by a live b with t_b < t_a
                    in_t[:, a] &= ~(live[:, b] & (k[:, b] * m[:, a] < k[:, a] * m[:, b]))
        size = in_t.sum(1)
        unit = np.eye(3, dtype=np.int64)
        single = [probe(c + s * unit[a]) for a in range(3)]
        pair = {(a, b): probe(c + s * (unit[a] + unit[b])) for a in range(3) for b in range(a + 1, 3)}
        low = np.full(len(alive), BIG)
        passes = size < 2
        for a in range(3):                                                           # the side cells of the axes of T
            sol, flat = single[a]
            low = np.where(in_t[:, a] & (size >= 2) & sol, np.minimum(low, flat), low)
            passes |= (size == 2) & in_t[:, a] & ~sol                                # |T| = 2: one free side cell
            for b in range(3):
                if b != a:                                                           # |T| = 3: the staircase a, then a + b
                    passes |= (size == 3) & ~sol & ~pair[(min(a, b), max(a, b))][0]
        for sol, flat in pair.values():
            low = np.where((size == 3) & sol, np.minimum(low, flat), low)
        blocked = ~passes
        c = c + s * in_t
        j = j + in_t
        arrived = (c == o[None, :]).all(1)
        sol, flat = probe(c)
        out = ~((c >= 0) & (c < counts_a)).all(1)
        value = np.where(blocked, low, np.where(arrived | out, -1, np.where(sol, flat, -2)))
        done = value != -2
        result[alive[done]] = value[done]
        keep = ~done
        alive, c, j, s, m = alive[keep], c[keep], j[keep], s[keep], m[keep]
    assert not len(alive), 'the lockstep walk did not end within nx + ny + nz steps'
    assert (result < BIG).all()
    return result


def restate(solid, counts, origins, framed=None, blocker=True):
    """The header's outputs of one call -> (seen (n,) int32, blocker (V, n) int32 or None): the lockstep walk per origin, then the
    rules of OUTPUTS."""
    n = int(np.prod(counts))
    V = len(origins)
    full = np.stack([blockers_lockstep(np.asarray(solid, bool).reshape(counts), counts, o) for o in origins]) if n else np.zeros((V, 0), np.int64)
    return outputs_of(full, framed, blocker)


def outputs_of(full, framed, blocker=True):
    """OUTPUTS from the blockers of every (origin, query) pair without a frustum."""
    V, n = full.shape
    fr = np.full(n, -1, np.int64) if framed is None else np.asarray(framed, np.int64)
    bit = ((fr[None, :] >> np.arange(V, dtype=np.int64)[:, None]) & 1) != 0
    seen = ((bit & (full < 0)).astype(np.int64) << np.arange(V, dtype=np.int64)[:, None]).sum(0).astype(np.int32)
    return seen, (np.where(bit, full, -1).astype(np.int32) if blocker else None)


def pack(member):
    """BITS of a member array -> (ceil(n / 32),) int32."""
    member = np.asarray(member, bool).reshape(-1)
    padded = np.zeros(-(-len(member) // 32) * 32, bool)
    padded[:len(member)] = member
    return np.packbits(padded, bitorder='little').view('<u4').astype(np.uint32).view(np.int32)


def member_of(values, level, mask=None, mask_level=0.0):
    """MEMBER in numpy float32: a NaN is no member."""
    with np.errstate(invalid='ignore'):
        m = np.asarray(values, np.float32) >= np.float32(level)
        if mask is not None:
            m &= np.asarray(mask, np.float32) >= np.float32(mask_level)
    return m


# ---------------------------------------------------------------------------------------------------------------- the case matrix
GRIDS = [(1, 1, 1), (1, 1, 70), (5, 1, 1), (3, 2, 5), (9, 10, 11), (17, 9, 33), (20, 17, 13), (33, 34, 35)]
GRID_IDS = ['%dx%dx%d' % g for g in GRIDS]
FIELDS = ['share-0', 'share-0.1', 'share-0.45', 'share-1', 'strided', 'nan', 'mask']
ORIGIN_COUNTS = (1, 3, 31)
FRAMINGS = ('null', 'random', 'zero')


def field_of(kind, counts):
    """-> dict(values (n,) float32 view -- a column of an (n, 3) array where the kind says so --, level, mask or None, mask_level,
    member (n,) bool: the member test restated)."""
    n = int(np.prod(counts))
    rng = np.random.default_rng([GRIDS.index(tuple(counts)), FIELDS.index(kind)])
    mask, mask_level = None, 0.0
    if kind.startswith('share-'):
        share = float(kind[6:])
        values = rng.random(n, dtype=np.float32)
        level = {0.0: 1.5, 1.0: -0.5}.get(share, 1.0 - share)
    elif kind == 'strided':
        values, level = rng.random((n, 3), dtype=np.float32)[:, 1], 0.7
    elif kind == 'nan':
        values, level = rng.random(n, dtype=np.float32), 0.4
        values[rng.random(n) < 0.3] = np.nan
    else:
        wide = rng.random((n, 4), dtype=np.float32)
        values, level, mask, mask_level = wide[:, 0], 0.2, wide[:, 2], 0.5
    return dict(values=values, level=level, mask=mask, mask_level=mask_level, member=member_of(values, level, mask, mask_level))


def origins_of(counts, V):
    """V lattice origins: one step outside the corner (ties of three axes), inside, outside a face, 2^20 cells away, then random
    ones round the grid."""
    nx, ny, nz = counts
    rng = np.random.default_rng([GRIDS.index(tuple(counts)), V])
    fixed = [(-1, -1, -1)] if V == 1 else [(int(rng.integers(nx)), int(rng.integers(ny)), int(rng.integers(nz))), (nx, ny // 2, -3), (FAR, -FAR, 500), (-1, -1, -1)]
    more = [tuple(int(rng.integers(-3, c + 3)) for c in counts) for _ in range(max(V - len(fixed), 0))]
    return np.array((fixed + more)[:V], np.int32)


def framings_of(counts, V):
    n = int(np.prod(counts))
    rng = np.random.default_rng([GRIDS.index(tuple(counts)), V, 7])
    return dict(null=None, random=rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32), zero=np.zeros(n, np.int32))


def origin_counts(counts):
    return [V for V in ORIGIN_COUNTS if V < 31 or int(np.prod(counts)) <= 1000]


@functools.lru_cache(maxsize=None)
def expected(counts, kind, V):
    """The blockers of every (origin, query) pair of a case, by the lockstep restatement: computed once, shared, never changed."""
    f = field_of(kind, counts)
    full = np.stack([blockers_lockstep(f['member'].reshape(counts), counts, o) for o in origins_of(counts, V)])
    full.setflags(write=False)
    return full


# ---------------------------------------------------------------------------------------------------------------- running a call
def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def on(device, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def column_on(device, view):
    """A numpy column view -> the same view of its base array on the device (the stride survives)."""
    if view is None:
        return None
    if view.base is None or view.base.ndim != 2:
        return torch.from_numpy(np.array(view)).to(device)
    col = (view.__array_interface__['data'][0] - view.base.__array_interface__['data'][0]) // 4
    return torch.from_numpy(np.array(view.base)).to(device)[:, col]


def run_ops(device, f, counts, origins, framed=None, blocker=True, flags=0):
    """ops.grid_solid_bits + ops.grid_sight on the loaded library -> numpy (bits, seen, blocker or None)."""
    values, mask = column_on(device, f['values']), column_on(device, f['mask'])
    assert values.numel() <= 1 or values.stride(0) == f['values'].strides[0] // 4
    bits = pk.ops.grid_solid_bits(values, f['level'], mask, f['mask_level'])
    seen, block = pk.ops.grid_sight(bits, counts, origins, on(device, framed), blocker, flags)
    assert bits.dtype == seen.dtype == I32 and seen.device.type == torch.device(device).type and (block is None) == (not blocker)
    return bits.cpu().numpy(), seen.cpu().numpy(), None if block is None else block.cpu().numpy()


def run_raw(L, device, f, counts, origins, framed=None, blocker=True, flags=0):
    """The two entry points on the plain library handle `L` with tensors of `device`, every buffer with a canary word behind it ->
    numpy (bits, seen, blocker or None); asserts that nothing else was written."""
    nx, ny, nz = counts
    n, V = nx * ny * nz, len(origins)
    words = (n + 31) // 32
    values, mask = column_on(device, f['values']), column_on(device, f['mask'])
    full = lambda *shape: torch.full(shape, CANARY, dtype=I32, device=device)
    bits, seen, block = full(words + 1), full(n + 1), full(V * n + 1) if blocker else None
    ld = lambda t: 1 if t is None or t.numel() <= 1 else t.stride(0)
    assert L.occ4d_sight_bits_f32(ptr(values), ld(values), f['level'], ptr(mask), ld(mask), f['mask_level'], n, ptr(bits), None) == pk._lib.OK
    org = np.ascontiguousarray(origins, np.int32)
    assert L.occ4d_sight_grid_u32(ptr(bits), nx, ny, nz, org.ctypes.data_as(ctypes.c_void_p), V, ptr(on(device, framed)), ptr(seen),
                                  ptr(block), flags, None) == pk._lib.OK, L.occ4d_last_error()
    bits, seen = bits.cpu().numpy(), seen.cpu().numpy()
    assert bits[words] == CANARY and seen[n] == CANARY
    if blocker:
        block = block.cpu().numpy()
        assert block[V * n] == CANARY
        block = block[:V * n].reshape(V, n)
    return bits[:words], seen[:n], block


def same(got, want, what):
    for g, w, key in zip(got, want, ('bits', 'seen', 'blocker')):
        assert (g is None) == (w is None), (what, key)
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, key)


# ---------------------------------------------------------------------------------------------------------------- the checks
def check_restatements_agree():
    """The lockstep restatement against the scalar one on every grid of at most 1000 points, every field, every origin of the
    matrix; and at 7 x 6 x 5 at 40 % solid towards every grid point and a ring of outside ones."""
    walks = 0
    for counts in GRIDS:
        if int(np.prod(counts)) > 1000:
            continue
        for kind in FIELDS:
            solid = field_of(kind, counts)['member'].reshape(counts)
            for V in origin_counts(counts):
                full = expected(counts, kind, V)
                for v, o in enumerate(origins_of(counts, V).tolist()):
                    assert np.array_equal(full[v], blockers_scalar(solid, counts, o)), (counts, kind, o)
                    walks += full.shape[1]
    counts = (7, 6, 5)
    solid = np.random.default_rng(40).random(counts) < 0.4
    for o in itertools.product(range(-1, 8, 2), range(-1, 7, 3), range(-2, 7, 2)):
        assert np.array_equal(blockers_lockstep(solid, counts, o), blockers_scalar(solid, counts, o)), o
    assert walks > 20000


def scene(counts, cells):
    solid = np.zeros(counts, bool)
    for c in cells:
        solid[tuple(c)] = True
    return solid


def by_hand():
    """(counts, solid cells, origin, {query: -1 or the blocker's flat index}): cases worked on paper from the header."""
    cases = []
    # a cell on an axis line: the cells behind it are hidden with that blocker, the cell itself and the cells in front are seen
    hit = flat_of((3, 3, 7), (1, 1, 3))
    cases.append(((3, 3, 7), [(1, 1, 3)], (1, 1, 0), {(1, 1, 0): -1, (1, 1, 1): -1, (1, 1, 2): -1, (1, 1, 3): -1, (1, 1, 4): hit,
                                                    (1, 1, 5): hit, (1, 1, 6): hit, (0, 1, 2): -1, (0, 1, 6): hit}))
    # the 2 x 2 diagonal: one side cell solid -- seen; both -- hidden by the lower flat index, (0, 1, 0) = 1 against (1, 0, 0) = 2
    cases.append(((2, 2, 1), [(1, 0, 0)], (1, 1, 0), {(0, 0, 0): -1}))
    cases.append(((2, 2, 1), [(0, 1, 0)], (1, 1, 0), {(0, 0, 0): -1}))
    cases.append(((2, 2, 1), [(1, 0, 0), (0, 1, 0)], (1, 1, 0), {(0, 0, 0): 1}))
    cases.append(((2, 2, 1), [(1, 0, 0), (0, 1, 0)], (0, 0, 0), {(1, 1, 0): 1, (1, 0, 0): -1, (0, 1, 0): -1}))
    # the three-axis tie (0, 0, 0) -> (1, 1, 1): X 4, Y 2, Z 1, XY 6, XZ 5, YZ 3.  Each staircase as the only free one: seen
    between = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]
    for first, then in (((1, 0, 0), (1, 1, 0)), ((1, 0, 0), (1, 0, 1)), ((0, 1, 0), (1, 1, 0)), ((0, 1, 0), (0, 1, 1)),
                        ((0, 0, 1), (1, 0, 1)), ((0, 0, 1), (0, 1, 1))):
        cases.append(((2, 2, 2), [c for c in between if c not in (first, then)], (1, 1, 1), {(0, 0, 0): -1}))
    cases.append(((2, 2, 2), between, (1, 1, 1), {(0, 0, 0): 1}))                       # none free: the lowest, Z
    cases.append(((2, 2, 2), between[3:], (1, 1, 1), {(0, 0, 0): 3}))                   # every first step free, no second: YZ
    cases.append(((2, 2, 2), between[:3], (1, 1, 1), {(0, 0, 0): 1}))
    # q == o, on a solid cell; o solid: never tested
    cases.append(((3, 2, 5), [(1, 1, 2)], (1, 1, 2), {(1, 1, 2): -1}))
    cases.append(((1, 1, 4), [(0, 0, 3)], (0, 0, 3), {(0, 0, 0): -1, (0, 0, 2): -1}))
    cases.append(((1, 1, 4), [(0, 0, 3), (0, 0, 1)], (0, 0, 3), {(0, 0, 0): 1, (0, 0, 1): -1, (0, 0, 2): -1}))
    # o one step outside a face, an edge, a corner
    cases.append(((3, 3, 3), [(0, 1, 1)], (-1, 1, 1), {(2, 1, 1): flat_of((3, 3, 3), (0, 1, 1)), (1, 1, 1): flat_of((3, 3, 3), (0, 1, 1)),
                                                     (0, 1, 1): -1, (0, 0, 1): -1, (2, 0, 1): flat_of((3, 3, 3), (0, 1, 1))}))
    cases.append(((3, 3, 3), [], (-1, -1, 1), {(1, 1, 1): -1, (0, 0, 1): -1}))
    cases.append(((3, 3, 3), [(0, 0, 1)], (-1, -1, 1), {(1, 1, 1): 1, (2, 2, 1): 1, (0, 0, 1): -1}))
    cases.append(((3, 3, 3), [(0, 1, 1), (1, 0, 1)], (-1, -1, 1), {(1, 1, 1): flat_of((3, 3, 3), (0, 1, 1)), (0, 0, 1): -1}))
    cases.append(((3, 3, 3), [], (-1, -1, -1), {(0, 0, 0): -1, (2, 2, 2): -1}))
    cases.append(((3, 3, 3), [(0, 0, 0)], (-1, -1, -1), {(1, 1, 1): 0, (2, 2, 2): 0, (0, 0, 0): -1}))
    # o at (+-2^20, ...): along an axis the far origin is an axis line
    cases.append(((1, 1, 5), [(0, 0, 3)], (0, 0, FAR), {(0, 0, 0): 3, (0, 0, 2): 3, (0, 0, 3): -1, (0, 0, 4): -1}))
    cases.append(((5, 1, 1), [(1, 0, 0)], (-FAR, 0, 0), {(4, 0, 0): 1, (2, 0, 0): 1, (1, 0, 0): -1, (0, 0, 0): -1}))
    # ... and off the axis by one cell in 2^20: the walk leaves the 1 x 1 x 5 line through the far face only
    cases.append(((1, 1, 5), [(0, 0, 3)], (1, -1, FAR), {(0, 0, 0): 3, (0, 0, 4): -1}))
    cases.append(((2, 2, 2), [], (FAR, -FAR, FAR), {(0, 0, 0): -1, (1, 1, 1): -1}))
    return cases


def check_by_hand(device=None, flags=FLAGS):
    """The cases worked by hand on both restatements; with a device also on the loaded library."""
    for counts, cells, origin, wanted in by_hand():
        solid = scene(counts, cells)
        for q, want in wanted.items():
            assert walk_scalar(solid, counts, q, origin) == want, (counts, cells, origin, q)
        lock = blockers_lockstep(solid, counts, origin)
        got = [lock]
        if device is not None:
            f = dict(values=solid.reshape(-1).astype(np.float32), level=0.5, mask=None, mask_level=0.0)
            for fl in flags:
                bits, seen, block = run_ops(device, f, counts, [origin], None, True, fl)
                assert np.array_equal(bits, pack(solid)) and np.array_equal(seen, (block[0] < 0).astype(np.int32))
                got.append(block[0])
        for q, want in wanted.items():
            assert all(g[flat_of(counts, q)] == want for g in got), (counts, cells, origin, q, [g[flat_of(counts, q)] for g in got])
        assert all(np.array_equal(g, lock) for g in got)


def check_grid(counts, device, twin_handle=None):
    """Every cell of the matrix on one grid: fields x V x framed x blocker (x every value of FLAGS) through ops, twice with equal
    bits, EQUAL to the restatement; with `twin_handle` (a plain handle of the g++ twin beside the HIP library) also
    bit-equal to the twin on host arrays.  -> the number of calls compared."""
    calls = 0
    for kind in FIELDS:
        f = field_of(kind, counts)
        for V in origin_counts(counts):
            origins, full = origins_of(counts, V), expected(counts, kind, V)
            for framing, framed in framings_of(counts, V).items():
                for blocker in (True, False):
                    want = (pack(f['member']),) + outputs_of(full, framed, blocker)
                    what = '%s %s V%d %s blocker=%r' % (counts, kind, V, framing, blocker)
                    for flags in FLAGS:
                        got = run_ops(device, f, counts, origins, framed, blocker, flags)
                        same(got, want, what + ' flags %d' % flags)
                        same(run_ops(device, f, counts, origins, framed, blocker, flags), got, what + ' again')
                        calls += 2
                    if twin_handle is not None:
                        same(run_raw(twin_handle, 'cpu', f, counts, origins, framed, blocker), got, what + ' twin')
                    # the consequences that hold for every call
                    seen, block = got[1], got[2]
                    fr = np.full(len(seen), -1, np.int32) if framed is None else framed
                    assert not (seen & ~fr).any() and not (seen >> V).any(), what
                    if blocker and block.size:
                        assert f['member'][block[block >= 0]].all(), what               # every blocker is a solid cell
                        bit = ((fr[None, :] >> np.arange(V)[:, None]) & 1) != 0
                        assert np.array_equal(block < 0, ~bit | (((seen[None, :] >> np.arange(V)[:, None]) & 1) != 0)), what
    return calls


def check_raw_canaries(device, L):
    """The raw entry points write their n (V n, ceil(n / 32)) words and nothing behind them; n == 0 touches no pointer."""
    for counts in ((3, 2, 5), (9, 10, 11)):
        f = field_of('mask', counts)
        origins, full = origins_of(counts, 3), expected(counts, 'mask', 3)
        for flags in FLAGS:
            same(run_raw(L, device, f, counts, origins, None, True, flags), (pack(f['member']),) + outputs_of(full, None), (counts, flags))
    org = np.zeros((1, 3), np.int32)
    assert L.occ4d_sight_bits_f32(None, 1, 0.5, None, 0, 0.0, 0, None, None) == pk._lib.OK
    assert L.occ4d_sight_grid_u32(None, 0, 4, 4, None, 1, None, None, None, 0, None) == pk._lib.OK
    assert L.occ4d_sight_grid_u32(None, 4, 0, 0, org.ctypes.data_as(ctypes.c_void_p), 31, None, None, None, 0, None) == pk._lib.OK


def all_pairs(device, solid, counts, flags=0):
    """seen[o, q] for every pair of grid points, from the library: the grid points as origins, 31 at a time."""
    n = int(np.prod(counts))
    cells = np.stack(np.unravel_index(np.arange(n), counts), 1).astype(np.int32)
    f = dict(values=solid.reshape(-1).astype(np.float32), level=0.5, mask=None, mask_level=0.0)
    rows = []
    for start in range(0, n, 31):
        chunk = cells[start:start + 31]
        seen, block = run_ops(device, f, counts, chunk, None, True, flags)[1:]
        assert np.array_equal(((seen[None, :] >> np.arange(len(chunk))[:, None]) & 1) != 0, block < 0)
        rows.append(block < 0)
    return np.concatenate(rows)


def free_components(solid):
    """The 6-connected components of the free cells -> (nx, ny, nz) int, 0 on solid cells."""
    try:
        from scipy import ndimage
        return ndimage.label(~solid)[0]
    except ImportError:
        label = np.zeros(solid.shape, np.int64)
        k = 0
        for start in zip(*np.nonzero(~solid)):
            if label[start]:
                continue
            k += 1
            label[start] = k
            queue = [start]
            while queue:
                c = queue.pop()
                for a in range(3):
                    for step in (-1, 1):
                        d = list(c)
                        d[a] += step
                        d = tuple(d)
                        if all(0 <= d[i] < solid.shape[i] for i in range(3)) and not solid[d] and not label[d]:
                            label[d] = k
                            queue.append(d)
        return label


def check_consequences(device):
    """On what the LIBRARY returns: seen is symmetric between grid points; a face-connected plane, an edge-connected staircase and a
    corner-connected plane hide everything across them; two free cells that see each other share a 6-connected free component."""
    counts = (7, 6, 5)
    n = 7 * 6 * 5
    for share, seed in ((0.15, 1), (0.4, 2), (0.45, 3)):
        solid = np.random.default_rng(seed).random(counts) < share
        seen = all_pairs(device, solid, counts, FLAGS[seed % len(FLAGS)])
        assert seen.shape == (n, n) and np.array_equal(seen, seen.T) and seen.diagonal().all(), share
        comp = free_components(solid).reshape(-1)
        free = comp > 0
        pairs = seen & free[:, None] & free[None, :]
        assert pairs.sum() > n and (comp[:, None] == comp[None, :])[pairs].all(), share
    ix, iy, iz = np.indices(counts)
    for name, side in (('face', ix - 3), ('staircase', ix + iy - 5), ('corner', ix + iy + iz - 8)):
        solid = side == 0
        seen = all_pairs(device, solid, counts)
        s = side.reshape(-1)
        across = (s[:, None] < 0) & (s[None, :] > 0)
        assert across.sum() > 500 and not seen[across].any() and not seen.T[across].any(), name
        assert np.array_equal(seen, seen.T)
    # ... and without the wall every pair sees each other
    assert all_pairs(device, np.zeros(counts, bool), counts).all()


def check_argument_errors(device):
    f = field_of('share-0.45', (9, 10, 11))
    values = on(device, f['values'])
    bits = pk.ops.grid_solid_bits(values, 0.5)
    assert not pk.ops.grid_solid_bits(values, float('nan')).any()                        # a NaN level: no member
    grid = lambda **k: pk.ops.grid_sight(**dict(dict(bits=bits, counts=(9, 10, 11), origins=[(0, 0, 0)]), **k))
    for kw, text in ((dict(origins=np.zeros((0, 3), np.int32)), r'V = 0 must be in \[1, 31\]'),
                     (dict(origins=np.zeros((32, 3), np.int32)), 'V = 32 must be in'),
                     (dict(origins=[(0, FAR + 1, 0)]), r'origin 0 = \(0, 1048577, 0\) has a coordinate outside \[-1048576, 1048576\]'),
                     (dict(origins=[(0, 0, 0), (0, 0, -FAR - 1)]), r'origin 1 = \(0, 0, -1048577\)'),
                     (dict(flags=1), 'flags = 1 must be 0'), (dict(flags=-1), 'flags = -1 must be 0'),
                     (dict(counts=(513, 1, 1), bits=torch.zeros(17, dtype=I32, device=device)), 'nx = 513, ny = 1, nz = 1 must be <= 512'),
                     (dict(bits=bits[:-1]), 'bits must be'), (dict(origins=[(0, 0)]), 'origins must be'),
                     (dict(framed=torch.zeros(5, dtype=I32, device=device)), 'framed must be'),
                     (dict(origins=[(2 ** 31, 0, 0)]), 'origins must fit int32')):
        with pytest.raises(AssertionError, match=text):
            grid(**kw)
    with pytest.raises(AssertionError):
        pk.ops.grid_sight(bits.to(torch.float32), (9, 10, 11), [(0, 0, 0)])
    with pytest.raises(AssertionError, match='mask must be'):
        pk.ops.grid_solid_bits(values, 0.5, mask=values[:-1])
    assert grid(origins=[(FAR, -FAR, FAR)])[0].shape == (990,) and grid(flags=0)[1] is None
    seen, block = pk.ops.grid_sight(torch.zeros(0, dtype=I32, device=device), (0, 3, 3), [(0, 0, 0)], blocker=True)
    assert seen.shape == (0,) and block.shape == (1, 0)


# ---------------------------------------------------------------------------------------------------------------- the module
def check_look(device):
    """sight.look on a dense output with select and channel against the restatement."""
    rng = np.random.default_rng(5)
    counts = (9, 10, 11)
    out_np = rng.random((990, 3)).astype(np.float32)
    out = torch.from_numpy(out_np).to(device)
    origins = np.array([(4, -2, 5), (9, 10, 11), (3, 3, 3)], np.int64)
    framed = rng.integers(0, 8, size=990).astype(np.int32)
    member = member_of(out_np[:, 1], 0.3, out_np[:, 2], 0.2)
    for fr in (None, framed):
        seen, block = pk.sight.look(out, counts, origins, 0.3, select=(2, 0.2), framed=on(device, fr), blocker=True, channel=1)
        want = restate(member, counts, origins.tolist(), fr)
        assert np.array_equal(seen.cpu().numpy(), want[0]) and np.array_equal(block.cpu().numpy(), want[1])
    seen, block = pk.sight.look(out, counts, origins[:1], 0.6)
    assert block is None and np.array_equal(seen.cpu().numpy(), restate(member_of(out_np[:, 0], 0.6), counts, origins[:1].tolist())[0])
    for kw, text in ((dict(level=float('nan')), 'level is NaN'), (dict(origins_ijk=np.zeros((0, 3), np.int32)), 'V = 0'),
                     (dict(origins_ijk=np.zeros((32, 3), np.int32)), 'V = 32'), (dict(origins_ijk=[(0, 0, FAR + 1)]), 'beyond 2\\^20 cells'),
                     (dict(origins_ijk=[(0.5, 0, 0)]), 'integers'), (dict(select=5), 'select = 5 must be')):
        with pytest.raises(ValueError, match=text):
            pk.sight.look(out, counts, **dict(dict(origins_ijk=origins, level=0.5), **kw))


def check_codes_and_by_label(device):
    rng = np.random.default_rng(9)
    n, V, k = 500, 3, 6
    framed = rng.integers(0, 2 ** V, size=n).astype(np.int32)
    seen = (rng.integers(0, 2 ** V, size=n) & framed).astype(np.int32)
    VIS, OCC, OUT = pk.projection.VISIBLE, pk.projection.OCCLUDED, pk.projection.OUTSIDE
    assert (VIS, OCC, OUT) == (0, 1, 2)
    for fr in (framed, None):
        for view in (None, 0, 2):
            s_bit = (seen != 0) if view is None else ((seen >> view) & 1) != 0
            f_bit = np.ones(n, bool) if fr is None else (fr != 0) if view is None else ((fr >> view) & 1) != 0
            want = np.where(s_bit & f_bit, VIS, np.where(f_bit, OCC, OUT)).astype(np.int32)
            got = pk.sight.codes(on(device, seen), on(device, fr), view)
            assert got.dtype == I32 and np.array_equal(got.cpu().numpy(), want)
            host = pk.sight.codes(seen, fr, view)
            assert isinstance(host, np.ndarray) and host.dtype == np.int32 and np.array_equal(host, want)
    with pytest.raises(ValueError, match='view = 31'):
        pk.sight.codes(seen, framed, 31)
    labels = rng.integers(-1, k + 2, size=n).astype(np.int32)                          # -1 (air) and numbers >= k are left out
    for fr in (framed, None):
        code = pk.sight.codes(seen, fr)
        want = np.array([[((labels == i) & (code == c)).sum() for c in (VIS, OCC, OUT)] for i in range(k)], np.int64)
        got = pk.sight.by_label(on(device, labels), k, on(device, seen), on(device, fr))
        assert got.dtype == torch.int64 and got.shape == (k, 3) and got.device.type == torch.device(device).type
        assert np.array_equal(got.cpu().numpy(), want)
    assert pk.sight.by_label(on(device, labels), 0, on(device, seen)).shape == (0, 3)
    assert 'never observed' in ' '.join(pk.sight.by_label.__doc__.split())


def check_grid_origin():
    mins, spacings = (-1.0, 0.5, 2.0), (0.25, 0.5, 1.0)
    pts = np.array([[-1.0, 0.5, 2.0], [-0.76, 0.99, 2.999], [-1.0001, 0.4999, 1.0], [5.0, -7.0, 100.5]])
    got = pk.sight.grid_origin(pts, mins, spacings)
    assert got.dtype == np.int32 and got.tolist() == [[0, 0, 0], [0, 0, 0], [-1, -1, -1], [24, -15, 98]]
    counts = (30, 30, 30)                                                               # geodesic.grid_index's convention where both answer
    inside_pts = np.array([[0.3, 3.3, 9.9], [6.4, 15.4, 31.9]])
    ijk = pk.sight.grid_origin(inside_pts, mins, spacings).astype(np.int64)
    assert np.array_equal((ijk[:, 0] * 30 + ijk[:, 1]) * 30 + ijk[:, 2], pk.geodesic.grid_index(inside_pts, mins, spacings, counts))
    assert pk.sight.grid_origin([[-1.0 + 0.25 * FAR, 0.5, 2.0]], mins, spacings).tolist() == [[FAR, 0, 0]]
    for bad in ([[-1.0 + 0.25 * (FAR + 1), 0.5, 2.0]], [[np.nan, 0, 0]], [[0, np.inf, 0]], [[0, 0, -1e30]]):
        with pytest.raises(ValueError, match='beyond 2\\^20 cells'):
            pk.sight.grid_origin(bad, mins, spacings)
    with pytest.raises(ValueError, match=r'must be \(V, 3\)'):
        pk.sight.grid_origin([0.0, 0.0, 0.0], mins, spacings)


# ---------------------------------------------------------------------------------------------------------------- end to end
def without(result):
    return {k: v for k, v in result.items() if k != 'sight'}


def world_origins(shared):
    """Three sensor positions round the fixture's grid: inside it, beside it and far above."""
    mins, spacings = yc.frame_of(shared)
    mins, spacings = np.asarray(mins, np.float64), np.asarray(spacings, np.float64)
    cells = np.array([[6.5, 3.25, 4.75], [-2.5, 15.5, 3.5], [7.5, 7.25, 400.5]])      # (off the cell boundaries)
    return mins + cells * spacings, [[6, 3, 4], [-3, 15, 3], [7, 7, 400]]


def check_result(shared, result, option, origins_ijk, output=None):
    """result['sight'] EQUAL to sight.look on the call's own implicit_output and to the restatement; framed EQUAL to the OUTSIDE
    rule on the call's own points_query."""
    device = shared.device
    got = result['sight']
    keys = ['seen'] + (['framed'] if option.cameras is not None else []) + (['blocker'] if option.blocker else [])
    assert sorted(got) == sorted(keys) and all(isinstance(v, np.ndarray) and v.dtype == np.int32 for v in got.values())
    out = result['implicit_output'] if output is None else output
    level = 0.5 if option.level is None else option.level
    framed = None
    if option.cameras is not None:
        cam_RT, cam_K, H, W = option.cameras
        V = len(origins_ijk)
        code = pk.projection.visibility(on(device, result['points_query'][:, :3]), torch.zeros((V, H, W), device=device), cam_RT, cam_K, 0.0)
        framed = ((code.cpu().numpy() != pk.projection.OUTSIDE).astype(np.int64) << np.arange(V)[:, None]).sum(0).astype(np.int32)
        assert np.array_equal(got['framed'], framed)
    seen, block = pk.sight.look(on(device, out), rc.COUNTS, np.asarray(origins_ijk), level, option.select, on(device, framed), option.blocker)
    assert np.array_equal(got['seen'], seen.cpu().numpy()) and got['seen'].shape == (rc.N_QUERIES,)
    member = member_of(out[:, 0], level) if option.select is None else member_of(out[:, 0], level, out[:, option.select[0]], option.select[1])
    want = restate(member, rc.COUNTS, origins_ijk, framed, option.blocker)
    assert np.array_equal(got['seen'], want[0])
    if option.blocker:
        assert np.array_equal(got['blocker'], block.cpu().numpy()) and np.array_equal(got['blocker'], want[1])
        assert got['blocker'].shape == (len(origins_ijk), rc.N_QUERIES)
    return got


def check_end_to_end(shared, monkeypatch):
    points, ijk = world_origins(shared)
    mins, spacings = yc.frame_of(shared)
    assert pk.sight.grid_origin(points, mins, spacings).tolist() == ijk
    option = pk.sight.Sight(origins=points, blocker=True)
    calls = rc.count_waits(monkeypatch)
    res = rc.infer(shared.device, shared.inputs, sight=option)
    assert calls['wait'] == 1                                                           # exactly one host wait
    monkeypatch.undo()
    got = check_result(shared, res, option, ijk)
    solid = shared.dense['implicit_output'][:, 0] >= np.float32(0.5)
    assert 0 < solid.sum() < rc.N_QUERIES and (got['blocker'] >= 0).any() and (got['seen'] != 0).any()      # the fixture's condition
    rc.same_result(without(res), shared.dense)                                          # implicit_output and the rest: unchanged
    # cameras: the ray-cast fixture's; the origins are the camera centres, framed is the OUTSIDE rule
    cam_RT, cam_K = yc.fixture_cameras(shared)
    option = pk.sight.Sight(cameras=(cam_RT, cam_K, *yc.IMAGE), select=(1, 0.1))
    centres = np.linalg.inv(pk.projection.invert_cameras(cam_RT, cam_K)[2])[:, :3, 3]
    cam_ijk = pk.sight.grid_origin(centres, mins, spacings).tolist()
    assert np.array_equal(option.origins, centres) and option.prepare(pk.products.Grid((rc.COUNTS, mins, spacings), 0.5, False, 13, shared.device))[1].tolist() == cam_ijk
    calls = rc.count_waits(monkeypatch)
    res = rc.infer(shared.device, shared.inputs, sight=option, components=pk.components.Components())
    assert calls['wait'] == 1
    monkeypatch.undo()
    got = check_result(shared, res, option, cam_ijk)
    assert 0 < (got['framed'] != 0).sum() and not (got['seen'] & ~got['framed']).any()
    rc.same_result({k: v for k, v in without(res).items() if k != 'components'}, shared.dense)
    # the question the feature exists for, on the call's own components
    k = res['components']['table'].shape[0]
    share = pk.sight.by_label(on(shared.device, res['components']['labels']), k, on(shared.device, got['seen']), on(shared.device, got['framed']))
    assert np.array_equal(share.cpu().numpy().sum(1), res['components']['table'][:, 0])
    # under refine and in track_mode 'all': the sight of the array the call returns
    option = pk.sight.Sight(origins=points[:2], level=0.48, blocker=True)
    res = rc.infer(shared.device, shared.inputs, refine=pk.inference.GridRefine(2, 0.46, 1), sight=option)
    check_result(shared, res, option, ijk[:2])
    res = rc.infer(shared.device, shared.inputs, track_mode='all', sight=option)
    check_result(shared, res, option, ijk[:2])
    rc.same_result(without(res), shared.dense_all)


def check_clip(shared):
    """evaluate_clip(sight=..., sights=[]) over two frames: one dict per output frame, that of the perform_inference call."""
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = rc.clip_inputs(shared)
    points, ijk = world_origins(shared)
    option, sights = pk.sight.Sight(origins=points, blocker=True), []
    clip = pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True, sight=option, sights=sights)
    dense = pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True)
    assert len(clip) == len(dense) == len(sights) == 2
    for t in range(2):
        for got, want in zip(clip[t], dense[t]):
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        assert sorted(sights[t]) == ['blocker', 'seen'] and sights[t]['seen'].shape == (rc.N_QUERIES,) and sights[t]['blocker'].shape == (3, rc.N_QUERIES)
    with pytest.raises(ValueError, match='sights'):
        pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', sight=option)
    with pytest.raises(ValueError, match='sight must be a sight.Sight'):
        pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', sight=1, sights=[])


def check_none_is_untouched(shared, monkeypatch):
    """sight=None: no new key and no entry point called."""
    def forbidden(*a, **k):
        raise AssertionError('sight=None must not reach the sight entry points')
    for name in ('grid_solid_bits', 'grid_sight'):
        monkeypatch.setattr(pk.ops, name, forbidden)
    L = pk._lib.lib()
    for name in SYMBOLS:
        monkeypatch.setattr(L, name, forbidden)
    res = rc.infer(shared.device, shared.inputs, sight=None)
    assert sorted(res) == sorted(shared.dense)
    rc.same_result(res, shared.dense)


def check_value_errors(shared):
    points, _ = world_origins(shared)
    with pytest.raises(ValueError, match="sight needs point_sample_mode 'grid'"):
        rc.infer(shared.device, shared.inputs, sight=pk.sight.Sight(origins=points), point_sample_mode='random')
    with pytest.raises(ValueError, match='sight must be a sight.Sight or None'):
        rc.infer(shared.device, shared.inputs, sight=4)
    mins, spacings = yc.frame_of(shared)
    too_far = np.asarray(mins, np.float64) + np.array([[0.5, 0.5, FAR + 1.5]]) * np.asarray(spacings, np.float64)
    with pytest.raises(ValueError, match='beyond 2\\^20 cells'):                        # in prepare(), before the encode
        rc.infer(shared.device, shared.inputs, sight=pk.sight.Sight(origins=too_far))
