"""Shared by tests/test_boxes_host.py (g++ twin) and tests/test_gpu_boxes.py (HIP): the oriented boxes of include/ext/occ4d_boxes.h
(ops.grid_box_extents / boxes_choose, components.yaw_directions / Boxes / oriented_boxes / tracks, perform_inference(boxes=...)).
RESTATEMENT: EXTENTS, RANGE and CHOICE written again from the header in numpy int64 (sorted points and reduceat for the extents, an
argmin over masked areas for the choice), sharing no code with csrc/boxes_math.hpp.  Every comparison is EQUAL -- integers, no
tolerance --, every library call is made twice with equal bits.  The one float comparison is components.oriented_boxes on a row
worked by hand, whose values are exact in binary."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import raycast_cases as yc
import refine_cases as rc
import occlusions4d_amd as pk

SYMBOLS = ['occ4d_boxes_extents_i32', 'occ4d_boxes_choose_i32']
OPS = ['grid_box_extents', 'boxes_choose']
CONSTANTS = dict(MAX_AXIS=2048, MAX_DIRS=256, MAX_COEF=32768, COLS=8, TILE=8, GATHER_SLOTS=8, GATHER_PROBES=4)
CANARY = -0x5a5a5a5b
I32 = torch.int32
IMAX, IMIN = 2 ** 31 - 1, -2 ** 31
MAX_COEF = 32768
FOREIGN = lambda K: [-1, -7, K, K + 5, IMAX, IMIN]
BAD_COEFS = [32769, -32769, IMAX, IMIN]
EMPTY_EXTENT, EMPTY_ZR = [IMAX, IMIN, IMAX, IMIN], [IMAX, IMIN, 0]


# ---------------------------------------------------------------------------------------------------------------- the restatement
def dead_rows(dirs):
    return (np.abs(np.asarray(dirs, np.int64)) > MAX_COEF).any(axis=1)


def restate_extents(labels, counts, K, dirs):
    """-> (extent (K, A, 4), zr (K, 3)) int64, from the header's EXTENTS and RANGE."""
    d = np.asarray(dirs, np.int64)
    A = d.shape[0]
    extent = np.tile(np.array(EMPTY_EXTENT, np.int64), (K, A, 1))
    zr = np.tile(np.array(EMPTY_ZR, np.int64), (K, 1))
    lab = np.asarray(labels, np.int64).reshape(counts)
    ix, iy, iz = np.nonzero((lab >= 0) & (lab < K))
    if len(ix) == 0:
        return extent, zr
    k = lab[ix, iy, iz]
    order = np.argsort(k, kind='stable')
    k, ix, iy, iz = k[order], ix[order], iy[order], iz[order]
    present, starts = np.unique(k, return_index=True)
    zr[present, 0], zr[present, 1] = np.minimum.reduceat(iz, starts), np.maximum.reduceat(iz, starts)
    zr[present, 2] = np.diff(np.append(starts, len(k)))
    live = ~dead_rows(d)
    u = ix[:, None] * d[None, live, 0] + iy[:, None] * d[None, live, 1]                 # (points, live rows)
    v = ix[:, None] * d[None, live, 2] + iy[:, None] * d[None, live, 3]
    rows = np.stack([np.minimum.reduceat(u, starts, axis=0), np.maximum.reduceat(u, starts, axis=0),
                     np.minimum.reduceat(v, starts, axis=0), np.maximum.reduceat(v, starts, axis=0)], axis=2)
    extent[np.ix_(present, np.nonzero(live)[0])] = rows
    return extent, zr


def areas(extent, dirs):
    """-> (qualifies (K, A) bool, area (K, A) int64) of CHOICE."""
    e, d = np.asarray(extent, np.int64), np.asarray(dirs, np.int64)
    du, dv = e[:, :, 1] - e[:, :, 0], e[:, :, 3] - e[:, :, 2]
    ok = ~dead_rows(d)[None, :] & (du >= 0) & (du < 2 ** 30) & (dv >= 0) & (dv < 2 ** 30)
    cell = np.where(dead_rows(d)[:, None], 0, np.abs(d))
    area = np.where(ok, (du + cell[None, :, 0] + cell[None, :, 1]) * (dv + cell[None, :, 2] + cell[None, :, 3]), np.iinfo(np.int64).max)
    return ok, area


def restate_choose(extent, zr, dirs):
    """-> box (K, 8) int64, from the header's CHOICE."""
    e, z = np.asarray(extent, np.int64), np.asarray(zr, np.int64)
    K = z.shape[0]
    ok, area = areas(e, dirs)
    box = np.zeros((K, 8), np.int64)
    for k in range(K):
        if z[k, 2] <= 0:
            box[k, 0] = -1
        elif not ok[k].any():
            box[k] = [-1, 0, 0, 0, 0, z[k, 0], z[k, 1], z[k, 2]]
        else:
            best = int(np.argmin(area[k]))                                                  # the first minimum: THE LOWEST a
            box[k] = [best, *e[k, best], z[k, 0], z[k, 1], z[k, 2]]
    return box


# ---------------------------------------------------------------------------------------------------------------- cases
GRIDS = [(1, 1, 1), (1, 1, 5), (5, 1, 1), (3, 2, 5), (7, 9, 4), (20, 19, 3)]
GRID_IDS = ['%dx%dx%d' % g for g in GRIDS]
A_VALUES = (1, 2, 63, 64, 65, 90, 256)
LABEL_KINDS = ['random', 'foreign', 'k-below', 'two-runs', 'shares']


def labels_of(kind, counts, rng):
    """-> (labels (n,) int32, K)."""
    nx, ny, nz = counts
    n = nx * ny * nz
    ix, iy, iz = np.indices(counts)
    if kind == 'random':
        K = 5
        lab = np.where(rng.random(n) < 0.4, -1, rng.integers(0, K, n))
    elif kind == 'foreign':
        K = 4
        lab = rng.integers(0, K, n)
        strange = rng.random(n) < 0.5
        lab[strange] = rng.choice(FOREIGN(K), int(strange.sum()))
    elif kind == 'k-below':                                                                # K below the largest label present
        K = 3
        lab = rng.integers(-1, 9, n)
        lab[0] = 8
    elif kind == 'two-runs':                                                               # an object in separate runs of one column
        K = 3
        lab = np.where(iz % 2 == 0, (ix + iy) % 2, np.where(iz % 4 == 1, -1, 2)).reshape(-1)
    else:                                                                                  # 'shares': one object that spans every
        tile = pk._lib.BOXES_CONSTANTS['TILE']                                             # workgroup's share, the others confined to one
        share = (ix // tile) * ((ny + tile - 1) // tile) + iy // tile
        K = int(share.max()) + 2
        lab = np.where((ix + 2 * iy + iz) % 3 == 0, 0, np.where((ix + iy) % 2 == 0, share + 1, -1)).reshape(-1)
    return lab.astype(np.int64).astype(np.int32), K                                        # (INT32 extremes wrap to themselves)


def dirs_of(A, rng, dead_every=5):
    """A rows of coefficients in [-2^15, 2^15], negative ones included, the edge values among them, a DEAD row interleaved every
    `dead_every` rows: one coefficient of the four replaced by a value outside the range."""
    d = rng.integers(-MAX_COEF, MAX_COEF + 1, (A, 4)).astype(np.int64)
    d[rng.random((A, 4)) < 0.1] = MAX_COEF
    d[rng.random((A, 4)) < 0.1] = -MAX_COEF
    if dead_every:
        for i, a in enumerate(range(dead_every - 1, A, dead_every)):
            d[a, i % 4] = BAD_COEFS[(i // 4) % 4]
    return d.astype(np.int32)


def on(device, a, dtype=I32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(device)


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def run_ops(device, labels, counts, K, dirs):
    """The two ops -> (extent, zr, box) as numpy."""
    lab, d = on(device, labels), on(device, dirs)
    extent, zr = pk.ops.grid_box_extents(lab, counts, K, d)
    box = pk.ops.boxes_choose(extent, zr, d)
    return extent.cpu().numpy(), zr.cpu().numpy(), box.cpu().numpy()


def run_raw(L, device, labels, counts, K, dirs, rows_behind=2):
    """The two entry points of the library handle L on buffers of exactly the documented sizes inside canary words: in front,
    behind, and `rows_behind` whole rows >= K -> (extent, zr, box) as numpy."""
    A, pad = len(dirs), 8
    lab, d = on(device, labels), on(device, dirs)
    sizes = dict(extent=A * 4, zr=3, box=8)
    buf = {k: torch.full((pad + (K + rows_behind) * w + pad,), CANARY, dtype=I32, device=device) for k, w in sizes.items()}
    view = {k: buf[k][pad:pad + K * w] for k, w in sizes.items()}
    nx, ny, nz = counts
    assert L.occ4d_boxes_extents_i32(p(lab), nx, ny, nz, K, p(d), A, p(view['extent']), p(view['zr']), None) == pk._lib.OK, L.occ4d_last_error()
    assert L.occ4d_boxes_choose_i32(p(view['extent']), p(view['zr']), p(d), K, A, p(view['box']), None) == pk._lib.OK, L.occ4d_last_error()
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()
    for k, w in sizes.items():
        whole = buf[k].cpu().numpy()
        assert (whole[:pad] == CANARY).all() and (whole[pad + K * w:] == CANARY).all(), 'canary of %s' % k
    return (view['extent'].cpu().numpy().reshape(K, A, 4), view['zr'].cpu().numpy().reshape(K, 3), view['box'].cpu().numpy().reshape(K, 8))


def same(got, want, what):
    for name, g, w in zip(('extent', 'zr', 'box'), got, want):
        assert g.shape == w.shape and np.array_equal(np.asarray(g, np.int64), np.asarray(w, np.int64)), (what, name)


def check_case(device, labels, counts, K, dirs, twin_handle=None, what=''):
    """One case: the ops twice, the raw entry points inside canaries, all EQUAL to the restatement; with `twin_handle` the device's
    library also bit for bit against the g++ twin's raw call on host copies."""
    extent, zr = restate_extents(labels, counts, K, dirs)
    want = (extent, zr, restate_choose(extent, zr, dirs))
    first, second = run_ops(device, labels, counts, K, dirs), run_ops(device, labels, counts, K, dirs)
    assert all(a.dtype == np.int32 for a in first)
    same(first, want, what)
    same(second, first, what + ' twice')
    same(run_raw(pk._lib.lib(), device, labels, counts, K, dirs), first, what + ' raw')
    if twin_handle is not None:
        same(run_raw(twin_handle, 'cpu', labels, counts, K, dirs), first, what + ' twin')
    return want


def check_grid(counts, device, twin_handle=None):
    """Every kind of labels x every A on one grid -> the number of cases."""
    rng = np.random.default_rng(sum(c * 31 ** i for i, c in enumerate(counts)))
    cases = 0
    for kind in LABEL_KINDS:
        labels, K = labels_of(kind, counts, rng)
        for A in A_VALUES:
            want = check_case(device, labels, counts, K, dirs_of(A, rng), twin_handle, '%s A=%d' % (kind, A))
            dead = dead_rows(dirs_of(A, np.random.default_rng(0)))
            assert (A < 5) == (not dead.any())                                             # the DEAD rows are there from A = 5 on
            cases += 1
        if kind == 'shares' and counts == (20, 19, 3):
            assert K == 3 * 3 + 1 and want[1][0].tolist() == [0, 2, (np.asarray(labels) == 0).sum()]  # object 0 in all nine shares
            assert (want[1][1:, 2] > 0).all()
    return cases


def check_columns(device, twin_handle=None):
    """Every column its own label: more objects in one workgroup's share than its gather table has slots."""
    slots = pk._lib.BOXES_CONSTANTS['GATHER_SLOTS']
    side = max(12, int(math.isqrt(slots)) + 1)
    counts, K = (side, side, 2), side * side
    assert K > slots and pk._lib.BOXES_CONSTANTS['TILE'] ** 2 > slots
    labels = np.repeat(np.arange(K, dtype=np.int32), 2)
    rng = np.random.default_rng(12)
    for A in (3, 90):
        want = check_case(device, labels, counts, K, dirs_of(A, rng), twin_handle, 'columns A=%d' % A)
        assert (want[1] == [0, 1, 2]).all()
    labels = labels.reshape(counts).copy()
    labels[:, :, 1] = labels[::-1, ::-1, 0]                                               # ... and every label in two far columns
    check_case(device, labels.reshape(-1), counts, K, dirs_of(65, rng), twin_handle, 'columns twice')


def check_int32_edge(device, twin_handle=None):
    """Coefficients of +-2^15 on the longest axes: |u|, |v| reach 2^15 * 2047 and twice that, the int32 edge the header names."""
    rows = np.array([[MAX_COEF, MAX_COEF, -MAX_COEF, -MAX_COEF], [-MAX_COEF, MAX_COEF, MAX_COEF, -MAX_COEF],
                     [MAX_COEF, -MAX_COEF, MAX_COEF, MAX_COEF], [MAX_COEF + 1, 0, 0, 1]], np.int32)
    rng = np.random.default_rng(2048)
    for counts in ((2048, 1, 1), (1, 2048, 1)):
        labels = np.where(rng.random(2048) < 0.2, -1, rng.integers(0, 2, 2048)).astype(np.int32)
        labels[[0, -1]] = 0
        want = check_case(device, labels, counts, 2, rows, twin_handle, 'edge %s' % (counts,))
        assert np.abs(want[0][0, :3]).max() == MAX_COEF * 2047 and want[0][0, 3].tolist() == EMPTY_EXTENT
    diagonal = (np.arange(2048 * 2) * 0).astype(np.int32)                                  # all of (2048, 2, 1): ix = 2047 and iy = 1
    want = check_case(device, diagonal, (2048, 2, 1), 1, rows, twin_handle, 'edge sum')
    assert want[0][0, 0].tolist() == [0, MAX_COEF * 2048, -MAX_COEF * 2048, 0]


def check_tall(device, twin_handle=None):
    """Columns longer than the 64 labels a wave loads at once: runs that cross the boundary between two loads, a last load of 3."""
    counts, rng = (2, 3, 131), np.random.default_rng(131)
    labels = np.repeat(rng.integers(-1, 4, 2 * 3 * 131 // 6 + 1), 6)[:2 * 3 * 131].astype(np.int32)       # runs of six across every border
    for A in (2, 65):
        check_case(device, labels, counts, 3, dirs_of(A, rng), twin_handle, 'tall A=%d' % A)
    want = check_case(device, np.zeros(131, np.int32), (1, 1, 131), 1, dirs_of(1, rng), twin_handle, 'tall one run')
    assert want[1].tolist() == [[0, 130, 131]]


def choose(device, extent, zr, dirs):
    """ops.boxes_choose twice on hand-made rows -> box as a list, EQUAL to the restatement."""
    e, z, d = np.asarray(extent, np.int64).reshape(len(zr), len(dirs), 4), np.asarray(zr, np.int64), np.asarray(dirs, np.int64)
    got = [pk.ops.boxes_choose(on(device, e), on(device, z), on(device, d)).cpu().numpy() for _ in range(2)]
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], restate_choose(e, z, d))
    return got[0].tolist()


def check_choice_by_hand(device):
    S = 2 ** 14
    unit = [S, 0, 0, S]
    # ties go to the lowest a: three identical rows; then a smaller area in the middle; then the same area from other widths
    assert choose(device, [[0, S, 0, S]] * 3, [[2, 3, 5]], [unit] * 3) == [[0, 0, S, 0, S, 2, 3, 5]]
    assert choose(device, [[0, S, 0, S], [0, S, 0, 0], [0, S, 0, 0]], [[2, 3, 5]], [unit] * 3) == [[1, 0, S, 0, 0, 2, 3, 5]]
    assert choose(device, [[0, 3 * S, 0, 0], [0, S, 0, S], [0, 0, 0, 3 * S]], [[0, 0, 9]], [unit] * 3) == [[0, 0, 3 * S, 0, 0, 0, 0, 9]]
    # |ax| + |ay| counts: the same extents, a direction of shorter coefficients wins although it stands later
    assert choose(device, [[0, 0, 0, 0]] * 2, [[0, 0, 1]], [unit, [S // 2, 0, 0, -S]])[0][0] == 1
    # a row without points, one with a negative count; every direction DEAD; 65 directions, the best one in the second pass of a lane
    assert choose(device, [[0, S, 0, S]] * 2, [[1, 2, 0], [1, 2, -4]], [unit]) == [[-1, 0, 0, 0, 0, 0, 0, 0]] * 2
    dead = [[S, 0, 0, 32769], [IMIN, 0, 0, S]]
    assert choose(device, [[0, S, 0, S]] * 2, [[4, 6, 7]], dead) == [[-1, 0, 0, 0, 0, 4, 6, 7]]
    many = [[0, 9 * S, 0, 9 * S]] * 65
    many[64] = [5, 6, 7, 8]
    assert choose(device, many, [[0, 0, 3]], [unit] * 65) == [[64, 5, 6, 7, 8, 0, 0, 3]]
    # foreign extents: max - min >= 2^30 is skipped, 2^30 - 1 is not; min > max is skipped; the extremes of int32 are
    wide = [[0, 2 ** 30, 0, 1], [0, 2 ** 30 - 1, 0, 1], [3, 2, 0, 0], [IMIN, IMAX, 0, 0], [0, 0, IMAX, IMIN]]
    assert choose(device, wide, [[0, 0, 1]], [unit] * 5) == [[1, 0, 2 ** 30 - 1, 0, 1, 0, 0, 1]]
    assert choose(device, [wide[0], wide[2], wide[3], wide[4]], [[7, 8, 2]], [unit] * 4) == [[-1, 0, 0, 0, 0, 7, 8, 2]]
    assert choose(device, [[-2 ** 29, 2 ** 29 - 1, -2 ** 29, 2 ** 29 - 1]], [[0, 0, IMAX]], [[-MAX_COEF, MAX_COEF, MAX_COEF, -MAX_COEF]])[0][0] == 0
    # a one-point object in a table that contains 0 degrees picks direction 0; empty extents of an object that has points: a* = -1
    table = pk.components.yaw_directions((1, 1, 1))['table']
    labels = np.full(7 * 9 * 4, -1, np.int32)
    labels[(3 * 9 + 5) * 4 + 2] = 1
    extent, zr, box = run_ops(device, labels, (7, 9, 4), 3, table)
    assert box.tolist() == [[-1] + [0] * 7, [0, 3 * S, 3 * S, 5 * S, 5 * S, 2, 2, 1], [-1] + [0] * 7]
    assert choose(device, [EMPTY_EXTENT] * 2, [[0, 1, 2]], [unit] * 2) == [[-1, 0, 0, 0, 0, 0, 1, 2]]


RECTANGLE_YAWS = (7, 17, 30, 45, 60, 73, 120, 163)


def rectangle_labels(deg, length=30, width=12, centre=(47.3, 50.1), counts=(96, 96, 2)):
    ix, iy = np.meshgrid(np.arange(counts[0]), np.arange(counts[1]), indexing='ij')
    th = math.radians(deg)
    dx, dy = ix - centre[0], iy - centre[1]
    inside = (np.abs(dx * math.cos(th) + dy * math.sin(th)) <= length / 2) & (np.abs(-dx * math.sin(th) + dy * math.cos(th)) <= width / 2)
    return np.repeat(np.where(inside, 0, -1).astype(np.int32).reshape(-1), counts[2])


def check_rectangles(device, twin_handle=None):
    """A 30 x 12-cell rectangle at eight yaws on 96 x 96 x 2: the library equals the restatement, whose a* lies within one direction
    of the yaw mod 90 and whose area is at most that of direction 0."""
    table = pk.components.yaw_directions((1, 1, 1))['table']
    assert table.shape == (90, 4)
    for deg in RECTANGLE_YAWS:
        extent, zr, box = check_case(device, rectangle_labels(deg), (96, 96, 2), 1, table, twin_handle, 'rectangle %d' % deg)
        best = int(box[0, 0])
        assert min((best - deg) % 90, (deg - best) % 90) <= 1, (deg, best)
        ok, area = areas(extent, table)
        assert ok.all() and area[0, best] <= area[0, 0] and area[0, best] == area[0].min()


def check_consequences(device):
    """What follows from the rules, on what the library returns: direction (1, 0, 0, 1) gives the component table's box columns,
    zr its z columns and its size."""
    rng = np.random.default_rng(5)
    for counts in ((7, 9, 4), (20, 19, 3), (3, 2, 5)):
        n = counts[0] * counts[1] * counts[2]
        field = torch.from_numpy((rng.random(n) < 0.35).astype(np.float32)).to(device)
        labels, _, table = pk.ops.grid_components(field, counts, 0.5, 6, 1)
        K = int(table.shape[0])
        assert K >= 2
        dirs = on(device, np.array([[1, 0, 0, 1], [0, 1, 1, 0]], np.int32))
        extent, zr = pk.ops.grid_box_extents(labels, counts, K, dirs)
        t, e, z = table.cpu().numpy(), extent.cpu().numpy(), zr.cpu().numpy()
        assert np.array_equal(e[:, 0], t[:, [6, 9, 7, 10]]) and np.array_equal(e[:, 1], t[:, [7, 10, 6, 9]])
        assert np.array_equal(z, t[:, [8, 11, 0]])
        # fewer rows than objects: the objects >= K are foreign, the rows below K as before
        fewer = pk.ops.grid_box_extents(labels, counts, K - 1, dirs)
        assert np.array_equal(fewer[0].cpu().numpy(), e[:K - 1]) and np.array_equal(fewer[1].cpu().numpy(), z[:K - 1])
    # K == 0 and an empty grid
    none = on(device, np.zeros((0,), np.int32))
    extent, zr = pk.ops.grid_box_extents(none, (0, 3, 2), 2, dirs)
    assert extent.cpu().tolist() == [[EMPTY_EXTENT] * 2] * 2 and zr.cpu().tolist() == [EMPTY_ZR] * 2
    assert pk.ops.boxes_choose(extent, zr, dirs).cpu().tolist() == [[-1] + [0] * 7] * 2
    extent, zr = pk.ops.grid_box_extents(on(device, np.zeros(6, np.int32)), (1, 3, 2), 0, dirs)
    assert extent.shape == (0, 2, 4) and zr.shape == (0, 3) and pk.ops.boxes_choose(extent, zr, dirs).shape == (0, 8)


def check_argument_errors(device):
    lab, dirs = on(device, np.zeros(30, np.int32)), on(device, np.array([[1, 0, 0, 1]], np.int32))
    with pytest.raises(AssertionError, match='labels must be \\(30,\\)'):
        pk.ops.grid_box_extents(lab[:29], (3, 2, 5), 1, dirs)
    with pytest.raises(AssertionError, match='dirs must be \\(A, 4\\)'):
        pk.ops.grid_box_extents(lab, (3, 2, 5), 1, dirs[:, :3])
    with pytest.raises(AssertionError, match='K = -1 must be >= 0'):
        pk.ops.grid_box_extents(lab, (3, 2, 5), -1, dirs, out=(lab, lab))
    with pytest.raises(AssertionError, match='A = 0 must be in \\[1, 256\\]'):
        pk.ops.grid_box_extents(lab, (3, 2, 5), 1, dirs[:0])
    with pytest.raises(AssertionError, match='A = 257 must be in \\[1, 256\\]'):
        pk.ops.grid_box_extents(lab, (3, 2, 5), 1, dirs.expand(257, 4))
    with pytest.raises(AssertionError, match='must be <= 2048'):
        pk.ops.grid_box_extents(lab[:0], (2049, 0, 1), 1, dirs)
    extent, zr = pk.ops.grid_box_extents(lab, (3, 2, 5), 2, dirs)
    with pytest.raises(AssertionError, match='extent and zr must be contiguous'):
        pk.ops.boxes_choose(extent[:1], zr, dirs)
    with pytest.raises(AssertionError, match='must be torch.int32'):
        pk.ops.boxes_choose(extent.long(), zr, dirs)
    out = pk.ops.grid_box_extents(lab, (3, 2, 5), 2, dirs, out=(torch.zeros(9, dtype=I32, device=device), torch.zeros(6, dtype=I32, device=device)))
    assert out[0].shape == (2, 1, 4) and np.array_equal(out[0].cpu().numpy(), extent.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------- the host side
def check_yaw_directions():
    S = 2 ** 14
    for spacings in ((1, 1, 1), (1.0, 0.99, 1.0), (0.5, 0.625, 3.0)):
        got = pk.components.yaw_directions(spacings)
        assert list(got) == ['table', 'yaw', 'unit'] and got['table'].shape == (90, 4) and got['table'].dtype == np.int32
        assert got['yaw'].dtype == np.float64 and got['unit'] == max(spacings[:2]) / S
        m = max(spacings[0], spacings[1])
        for a in range(90):
            th = math.radians(a * 90.0 / 90)
            assert abs(got['yaw'][a] - th) < 1e-15
            want = [S * spacings[0] / m * math.cos(th), S * spacings[1] / m * math.sin(th), -S * spacings[0] / m * math.sin(th),
                    S * spacings[1] / m * math.cos(th)]
            assert got['table'][a].tolist() == [int(np.rint(w)) for w in want], (spacings, a)
        assert not dead_rows(got['table']).any()
    got = pk.components.yaw_directions((1, 1, 1), n=4, span_deg=180.0)
    assert got['table'].tolist() == [[S, 0, 0, S], [11585, 11585, -11585, 11585], [0, S, -S, 0], [-11585, 11585, -11585, -11585]]
    for bad in (dict(n=0), dict(n=257), dict(spacings=(0.0, 1.0, 1.0)), dict(spacings=(1.0, float('nan'), 1.0))):
        with pytest.raises(ValueError, match='yaw_directions'):
            pk.components.yaw_directions(**{'spacings': (1, 1, 1), **bad})


def check_oriented_boxes():
    """Rows worked by hand; every value is exact in binary, so the comparison is EQUAL."""
    S = 2 ** 14
    dirs = pk.components.yaw_directions((1, 1, 1), n=2)['table']                         # 0 and 45 degrees
    box = np.array([[0, 2 * S, 5 * S, 1 * S, 2 * S, 3, 4, 10],                           # 4 x 2 x 2 cells at 0 degrees
                    [0, 1 * S, 2 * S, 2 * S, 5 * S, 0, 0, 8],                            # 2 x 4 x 1: the length lies across
                    [-1, 0, 0, 0, 0, 1, 2, 5], [2, 0, 0, 0, 0, 1, 2, 5]], np.int32)      # no direction; a direction out of range
    got = pk.components.oriented_boxes(box, dirs, (10.0, 20.0, 30.0), (1.0, 1.0, 0.5))
    assert list(got) == ['centre', 'size', 'yaw', 'points', 'fill']
    assert got['centre'][:2].tolist() == [[14.0, 22.0, 32.0], [12.0, 24.0, 30.25]]
    assert got['size'][:2].tolist() == [[4.0, 2.0, 1.0], [4.0, 2.0, 0.5]]
    assert got['yaw'][:2].tolist() == [0.0, -math.pi / 2] and got['fill'][:2].tolist() == [10 / 16, 8 / 8]
    assert got['points'].tolist() == [10, 8, 5, 5] and got['points'].dtype == np.int64
    for name in ('centre', 'size', 'yaw', 'fill'):
        assert np.isnan(got[name][2:]).all(), name
    # 45 degrees on a grid with sy = 0.5: a point of the lattice, length >= width, yaw in [-pi/2, pi/2)
    dirs = pk.components.yaw_directions((1.0, 0.5, 1.0), n=2)['table']
    got = pk.components.oriented_boxes(np.array([[1, 0, 0, 0, 4 * 11585, 0, 0, 3]], np.int32), dirs, (0, 0, 0), (1.0, 0.5, 1.0))
    assert got['size'][0, 0] >= got['size'][0, 1] and -math.pi / 2 <= got['yaw'][0] < math.pi / 2
    assert abs(got['yaw'][0] + math.pi / 4) < 1e-4                                         # the length lies across 45 degrees
    empty = pk.components.oriented_boxes(np.zeros((0, 8), np.int32), dirs, (0, 0, 0), (1, 1, 1))
    assert empty['centre'].shape == (0, 3) and empty['yaw'].shape == (0,)


def check_option():
    B = pk.components.Boxes
    option = B()
    assert (option.keyword, option.of, option.into, option.n, option.extents, B.reads_grid, B.clip_list) == \
        ('boxes', 'components', 'components', 90, False, False, None)
    assert B(of='segments', n=7, extents=True).into == 'segments' and 'segments' in repr(B(of='segments'))
    for kw in (dict(of='tracker'), dict(of=None), dict(n=0), dict(n=257), dict(n=2.5), dict(n=True)):
        with pytest.raises(ValueError, match='Boxes: '):
            B(**kw)
    B.check(option, ['components', 'boxes'])
    B.check(option, ['components', 'boxes'], 'random')                                     # reads no grid itself: components says so
    with pytest.raises(ValueError, match='boxes needs components='):
        B.check(option, ['segments', 'boxes'])
    with pytest.raises(ValueError, match='boxes needs segments='):
        B.check(B(of='segments'), ['components', 'boxes'])
    option.of = 'clearance'                                                                # check looks at the instance
    with pytest.raises(ValueError, match="of = 'clearance' must be 'components' or 'segments'"):
        B.check(option, ['components', 'clearance', 'boxes'])
    with pytest.raises(ValueError, match='boxes must be a components.Boxes or None'):
        B.check(0.5, ['components'])


def check_signatures():
    """boxes stands directly in front of next_view in both signatures."""
    names = list(inspect.signature(pk.inference.perform_inference).parameters)
    assert names[-6:] == ['boxes', 'next_view', 'sight', 'segments', 'tracker', 'clearance']
    names = list(inspect.signature(pk.evaluation.evaluate_clip).parameters)
    assert names[-9:] == ['boxes', 'next_view', 'next_views', 'sight', 'sights', 'segments', 'parts', 'route', 'routes']
    for fn in (pk.inference.perform_inference, pk.evaluation.evaluate_clip):
        assert inspect.signature(fn).parameters['boxes'].default is None and 'boxes' in fn.__doc__
    assert 'Boxes' in pk.products.__doc__


def check_tracks_by_hand():
    """components.tracks: obox_* only when every frame has box and dirs; without them the result is what it was."""
    S = 2 ** 14
    dirs = np.array([[S, 0, 0, S]], np.int32)
    table = np.array([[4, 0, -1, 6, 8, 2, 1, 2, 0, 2, 2, 1]], np.int64)
    box = np.array([[0, 1 * S, 2 * S, 2 * S, 2 * S, 0, 1, 4]], np.int32)
    link = np.array([[0, -1, -1, 0]], np.int32)
    plain = [dict(labels=None, table=table, link=link)] * 2
    full = [dict(labels=None, table=table, link=link, box=box, dirs=dirs)] * 2
    before, after = pk.components.tracks(plain, (0, 0, 0), (1, 1, 1)), pk.components.tracks(full, (0, 0, 0), (1, 1, 1))
    assert list(before[0]) == ['frames', 'components', 'size', 'centroid', 'box_min', 'box_max']
    assert list(after[0]) == list(before[0]) + ['obox_centre', 'obox_size', 'obox_yaw']
    for k in before[0]:
        assert np.array_equal(before[0][k], after[0][k])
    assert after[0]['obox_centre'].tolist() == [[2.0, 2.5, 1.0]] * 2 and after[0]['obox_size'].tolist() == [[2.0, 1.0, 2.0]] * 2
    assert after[0]['obox_yaw'].tolist() == [0.0, 0.0]
    assert list(pk.components.tracks([full[0], plain[0]], (0, 0, 0), (1, 1, 1))[0]) == list(before[0])


# ---------------------------------------------------------------------------------------------------------------- end to end
def without(result):
    return {k: v for k, v in result.items() if k not in ('components', 'segments')}


def check_joined(shared, got, option):
    """The dict the boxes joined: box, dirs[, extent] EQUAL to the stand-alone pieces on its own labels and to the restatement."""
    device = shared.device
    mins, spacings = yc.frame_of(shared)
    table = pk.components.yaw_directions(spacings, option.n)['table']
    K = len(got['table'])
    assert K >= 2 and np.array_equal(got['dirs'], table) and got['dirs'].dtype == np.int32
    assert got['box'].shape == (K, 8) and got['box'].dtype == np.int32 and ('extent' in got) == option.extents
    extent, zr = pk.ops.grid_box_extents(on(device, got['labels']), rc.COUNTS, K, on(device, table))
    box = pk.ops.boxes_choose(extent, zr, on(device, table))
    want_extent, want_zr = restate_extents(got['labels'], rc.COUNTS, K, table)
    assert np.array_equal(got['box'], box.cpu().numpy()) and np.array_equal(got['box'], restate_choose(want_extent, want_zr, table))
    if option.extents:
        assert np.array_equal(got['extent'], extent.cpu().numpy()) and np.array_equal(got['extent'], want_extent)
    assert np.array_equal(got['box'][:, 7], got['table'][:, 0]) and (got['box'][:, 0] >= 0).all()
    world = pk.components.oriented_boxes(got['box'], got['dirs'], mins, spacings)
    summary = pk.components.boxes_and_centroids(got['table'], mins, spacings)
    assert (world['size'][:, 0] >= world['size'][:, 1]).all() and (world['fill'] > 0).all() and (world['fill'] <= 1 + 1e-9).all()
    assert np.allclose(world['size'][:, 2], summary['box_max'][:, 2] - summary['box_min'][:, 2] + spacings[2], rtol=1e-12, atol=0)
    assert np.array_equal(world['points'], summary['size'])


def check_end_to_end(shared, monkeypatch):
    comp = pk.components.Components()
    option = pk.components.Boxes(extents=True)
    calls = rc.count_waits(monkeypatch)
    res = rc.infer(shared.device, shared.inputs, components=comp, boxes=option)
    assert calls['wait'] == 1                                                              # exactly one host wait
    monkeypatch.undo()
    assert list(res['components']) == ['labels', 'table', 'box', 'dirs', 'extent']
    check_joined(shared, res['components'], option)
    # boxes=None: every other key and array as they were
    alone = rc.infer(shared.device, shared.inputs, components=comp, boxes=None)
    assert sorted(alone) == sorted(res) and list(alone['components']) == ['labels', 'table']
    for k in alone['components']:
        assert np.array_equal(alone['components'][k], res['components'][k])
    rc.same_result(without(alone), shared.dense)
    rc.same_result(without(res), shared.dense)
    # of='segments'; both products at once, the boxes on the segments; under refine and in track_mode 'all'
    seg = pk.watershed.Segments(h=1)
    option = pk.components.Boxes(of='segments', n=7)
    res = rc.infer(shared.device, shared.inputs, components=comp, segments=seg, boxes=option)
    assert list(res['segments']) == ['labels', 'table', 'peaks', 'box', 'dirs'] and list(res['components']) == ['labels', 'table']
    check_joined(shared, res['segments'], option)
    option = pk.components.Boxes(n=64)
    res = rc.infer(shared.device, shared.inputs, refine=pk.inference.GridRefine(2, 0.46, 1), components=comp, boxes=option)
    check_joined(shared, res['components'], option)
    res = rc.infer(shared.device, shared.inputs, track_mode='all', components=comp, tracker=pk.components.Tracker(), boxes=option)
    assert list(res['components']) == ['labels', 'table', 'link', 'box', 'dirs']
    check_joined(shared, res['components'], option)
    rc.same_result(without(res), shared.dense_all)


def check_clip(shared):
    """evaluate_clip(components=..., objects=[], tracker=..., boxes=...): every dict gains box and dirs, components.tracks the three
    obox_* arrays; the tuples of the clip as without."""
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = rc.clip_inputs(shared)
    run = lambda **kw: pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True, **kw)
    option, objects = pk.components.Boxes(), []
    clip = run(components=pk.components.Components(), objects=objects, tracker=pk.components.Tracker(), boxes=option)
    dense = run()
    assert len(clip) == len(dense) == len(objects) == 2
    for t in range(2):
        for got, want in zip(clip[t], dense[t]):
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        assert list(objects[t]) == ['labels', 'table', 'link', 'box', 'dirs']
        check_joined(shared, objects[t], option)
    mins, spacings = yc.frame_of(shared)
    tracks = pk.components.tracks(objects, mins, spacings)
    plain = pk.components.tracks([{k: v for k, v in o.items() if k not in ('box', 'dirs')} for o in objects], mins, spacings)
    assert sorted(tracks) == sorted(plain) and len(tracks) >= 2
    for track, row in tracks.items():
        T = len(row['frames'])
        assert list(row) == list(plain[track]) + ['obox_centre', 'obox_size', 'obox_yaw']
        assert row['obox_centre'].shape == row['obox_size'].shape == (T, 3) and row['obox_yaw'].shape == (T,)
        for t, k, centre in zip(row['frames'], row['components'], row['obox_centre']):
            world = pk.components.oriented_boxes(objects[t]['box'], objects[t]['dirs'], mins, spacings)
            assert np.array_equal(centre, world['centre'][k])
    parts = []
    run(segments=pk.watershed.Segments(h=1), parts=parts, boxes=pk.components.Boxes(of='segments'))
    assert [list(o) for o in parts] == [['labels', 'table', 'peaks', 'box', 'dirs']] * 2
    with pytest.raises(ValueError, match='boxes needs components='):
        run(boxes=option)
    with pytest.raises(ValueError, match='boxes must be a components.Boxes'):
        run(components=pk.components.Components(), objects=[], boxes=[option])          # no list for boxes, as for tracker


def check_none_is_untouched(shared, monkeypatch):
    """boxes=None: no new key and no entry point called."""
    def forbidden(*a, **k):
        raise AssertionError('boxes=None must not reach the boxes entry points')
    for name in OPS:
        monkeypatch.setattr(pk.ops, name, forbidden)
    monkeypatch.setattr(pk.components, 'yaw_directions', forbidden)
    L = pk._lib.lib()
    for name in SYMBOLS:
        monkeypatch.setattr(L, name, forbidden)
    res = rc.infer(shared.device, shared.inputs, boxes=None)
    assert sorted(res) == sorted(shared.dense)
    rc.same_result(res, shared.dense)
    res = rc.infer(shared.device, shared.inputs, components=pk.components.Components())
    assert list(res['components']) == ['labels', 'table']


def check_value_errors(shared):
    comp, option = pk.components.Components(), pk.components.Boxes()
    with pytest.raises(ValueError, match='boxes must be a components.Boxes or None'):
        rc.infer(shared.device, shared.inputs, components=comp, boxes=comp)
    with pytest.raises(ValueError, match='boxes needs components=<a components.Components>'):
        rc.infer(shared.device, shared.inputs, boxes=option)
    with pytest.raises(ValueError, match='boxes needs segments=<a watershed.Segments>'):
        rc.infer(shared.device, shared.inputs, components=comp, boxes=pk.components.Boxes(of='segments'))
    with pytest.raises(ValueError, match="of = 'sight' must be 'components' or 'segments'"):
        pk.components.Boxes(of='sight')
    option.of = 'sight'
    with pytest.raises(ValueError, match="of = 'sight' must be 'components' or 'segments'"):
        rc.infer(shared.device, shared.inputs, components=comp, boxes=option)
    with pytest.raises(ValueError, match="components needs point_sample_mode 'grid'"):
        rc.infer(shared.device, shared.inputs, components=comp, boxes=pk.components.Boxes(), point_sample_mode='random')
