"""Shared by tests/test_layers_host.py (through the g++ twin) and tests/test_gpu_layers.py (on the device): the numpy restatement of
the rules of include/ext/occ4d_layers.h -- vectorised over the pixels, a loop over EVERY sample, no shortcut --, the case matrix of
the entry point, the consequences of the rules checked on what the library returns (the table recomputed from the per-pixel
arrays, the prefix property, the permutation of the objects, five slabs worked by hand, cameras that see nothing, the argument
contract) and the end-to-end comparisons of perform_inference(layers=...) on the refine fixture.
Everything is an integer and is compared EQUAL; the one float, a layer's depth, is compared bit for bit with the sample's own d_i.
The ray helpers are those of tests/raycast_cases.py."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import raycast_cases as yc
import refine_cases as rc
import occlusions4d_amd as pk
from raycast_cases import rays, grid_coords, cameras, march_of, look_at, MINS, SPACINGS

F32, I32 = np.float32, np.int32
IMAX = 2 ** 31 - 1
SYMBOLS = ['occ4d_layers_march_i32']
CONSTANTS = dict(MAX=8, COLS=7, AMODAL=0, VISIBLE=1, NEAR=2, XMIN=3, XMAX=4, YMIN=5, YMAX=6, GATHER_SLOTS=32, GATHER_PROBES=4)
GATHER_SLOTS = CONSTANTS['GATHER_SLOTS']          # the objects one workgroup's LDS table holds (csrc/layers.hip)
COLS = CONSTANTS['COLS']
FILL = np.array([0, 0, IMAX, IMAX, -1, IMAX, -1], I32)
PIXEL_ARRAYS = ('label', 'first', 'samples', 'point')
ARRAYS = PIXEL_ARRAYS + ('count', 'table', 'status')
CANARY = -0x5a5a5a5b

GRIDS = [(2, 2, 2), (3, 2, 5), (12, 7, 9), (17, 9, 33)]
GRID_IDS = ['%dx%dx%d' % g for g in GRIDS]
IMAGES = [(1, 1), (5, 7), (16, 16), (20, 33)]         # (H, W): ragged tiles, wave borders
VIEW_COUNTS = [0, 1, 3]
PLACEMENTS = yc.PLACEMENTS
STEP_COUNTS = [1, 2, 64]
LAYER_COUNTS = [1, 2, 4, 8]
LABEL_KINDS = ['none', 'one', 'slabs', 'blobs', 'random', 'foreign', 'k0', 'many']
OUTPUT_SETS = [ARRAYS, ('table',)] + [(name,) for name in ARRAYS]


# ---------------------------------------------------------------------------------------------------------------- restatement
def restate(labels, K, counts, mins, spacings, k_inv, rt_inv, H, W, near, step, n_steps, L):
    """The rules of the header, every sample walked -> dict(label, first, samples, point (V, H, W, L), count (V, H, W), table
    (V, K, 7), status (2,)), all int32."""
    labels = np.asarray(labels, I32)
    k_inv, rt_inv = np.asarray(k_inv, F32).reshape(-1, 4, 4), np.asarray(rt_inv, F32).reshape(-1, 4, 4)
    V = k_inv.shape[0]
    near, step = F32(near), F32(step)
    nx, ny, nz = counts
    top = np.asarray(counts, F32) - F32(1)
    P0, direction = rays(k_inv, rt_inv, H, W)
    P0, direction = P0.reshape(-1, 3), direction.reshape(-1, 3)
    R = P0.shape[0]
    label, first, point = (np.full((R, L), -1, I32) for _ in range(3))
    samples, count = np.zeros((R, L), I32), np.zeros(R, I32)
    with np.errstate(all='ignore'):
        for i in range(n_steps):
            d = near + F32(i) * step
            g = grid_coords(P0 + d * direction, mins, spacings)
            idx = np.flatnonzero(((F32(0) <= g) & (g <= top)).all(axis=1))
            r = np.minimum(np.floor(g[idx] + F32(0.5)).astype(np.int64), np.asarray(counts, np.int64) - 1)
            flat = (r[:, 0] * ny + r[:, 1]) * nz + r[:, 2]
            o = labels[flat].astype(np.int64)
            keep = (o >= 0) & (o < K)
            idx, o, flat = idx[keep], o[keep], flat[keep]
            match = label[idx] == o[:, None]
            samples[idx] += match
            new = ~match.any(axis=1)
            stored = np.minimum(count[idx], L)
            opens = new & (stored < L)
            rows, j = idx[opens], stored[opens]
            label[rows, j], first[rows, j], samples[rows, j], point[rows, j] = o[opens], i, 1, flat[opens]
            count[rows] += 1
            count[idx[new & ~opens]] = L + 1
    shape = (V, H, W, L)
    out = dict(label=label.reshape(shape), first=first.reshape(shape), samples=samples.reshape(shape), point=point.reshape(shape),
               count=count.reshape(V, H, W))
    out['table'] = table_of(out['label'], out['first'], K)
    out['status'] = np.array([(count == L + 1).sum(), (count >= 1).sum()], I32)
    return out


def table_of(label, first, K):
    """TABLE of the header from the per-pixel arrays and the pixel indices."""
    V, H, W, L = label.shape
    table = np.tile(FILL, (V, K, 1)).astype(I32)
    v, py, px, j = np.nonzero(label >= 0)
    k = label[v, py, px, j]
    np.add.at(table[:, :, 0], (v, k), 1)
    np.add.at(table[:, :, 1], (v, k), (j == 0).astype(I32))
    np.minimum.at(table[:, :, 2], (v, k), first[v, py, px, j])
    np.minimum.at(table[:, :, 3], (v, k), px.astype(I32))
    np.maximum.at(table[:, :, 4], (v, k), px.astype(I32))
    np.minimum.at(table[:, :, 5], (v, k), py.astype(I32))
    np.maximum.at(table[:, :, 6], (v, k), py.astype(I32))
    return table


# ---------------------------------------------------------------------------------------------------------------- inputs
def labels_of(kind, counts, L, rng):
    """(labels (n,) int32, K) of one kind on the grid."""
    nx, ny, nz = counts
    n = nx * ny * nz
    ix = np.broadcast_to(np.arange(nx)[:, None, None], counts)
    if kind == 'none':
        return np.full(n, -1, I32), 3
    if kind == 'one':
        return np.zeros(n, I32), 1
    if kind == 'slabs':                                   # slabs along x, one more than the layers kept where the grid has room
        m = min(nx, L + 1)
        return (ix * m // nx).astype(I32).reshape(-1), m
    if kind == 'blobs':                                   # a few balls in grid units, air between them
        K = 5
        lab = np.full(counts, -1, I32)
        pts = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing='ij'), axis=-1).astype(np.float64)
        for k in range(K):
            centre = rng.uniform(0, 1, size=3) * (np.array(counts) - 1)
            lab[np.linalg.norm((pts - centre) / np.maximum(np.array(counts) / 4.0, 1.0), axis=-1) <= 1.0] = k
        return lab.reshape(-1), K
    if kind == 'random':                                  # every sample changes owner: overflow everywhere
        K = 40
        return rng.integers(-1, K, size=n).astype(I32), K
    if kind == 'foreign':                                 # values < -1 and >= K mixed in: they count as -1
        K = 4
        lab = rng.integers(-1, K, size=n).astype(I32)
        bad = rng.uniform(size=n) < 0.4
        lab[bad] = rng.choice(np.array([-2, -7, K, K + 5, IMAX, -IMAX - 1], np.int64), size=int(bad.sum())).astype(I32)
        return lab, K
    if kind == 'k0':
        return rng.integers(-1, 6, size=n).astype(I32), 0
    if kind == 'many':                                    # every point an object of its own: more objects than gather slots
        return rng.permutation(n).astype(I32), n
    raise ValueError(kind)


def on(device, a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(device)


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def sizes_of(V, H, W, L, K):
    pixels = V * H * W
    return dict(label=pixels * L, first=pixels * L, samples=pixels * L, point=pixels * L, count=pixels, table=V * K * COLS, status=2)


def shapes_of(V, H, W, L, K):
    return dict(label=(V, H, W, L), first=(V, H, W, L), samples=(V, H, W, L), point=(V, H, W, L), count=(V, H, W), table=(V, K, COLS),
                status=(2,))


def run_raw(lib, device, labels, K, counts, mins, spacings, k_inv, rt_inv, H, W, near, step, n_steps, L, want=ARRAYS, pad=5):
    """The entry point of the library handle `lib` as it is: every array of `want` of exactly its documented size inside canary
    words, the others null -> dict of numpy arrays."""
    V = len(k_inv)
    sizes, shapes = sizes_of(V, H, W, L, K), shapes_of(V, H, W, L, K)
    buf = {k: torch.full((pad + sizes[k] + pad,), CANARY, dtype=torch.int32, device=device) for k in want}
    view = {k: buf[k][pad:pad + sizes[k]] for k in want}
    lab, k_t, rt_t = on(device, labels), on(device, np.asarray(k_inv, F32), torch.float32), on(device, np.asarray(rt_inv, F32), torch.float32)
    status = lib.occ4d_layers_march_i32(p(lab), *counts, K, mins[0], spacings[0], mins[1], spacings[1], mins[2], spacings[2], p(k_t),
                                        p(rt_t), V, H, W, float(near), float(step), n_steps, L, *(p(view.get(k)) for k in ARRAYS), None)
    assert status == pk._lib.OK, lib.occ4d_last_error()
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()
    out = {}
    for k in want:
        whole = buf[k].cpu().numpy()
        assert (whole[:pad] == CANARY).all() and (whole[pad + sizes[k]:] == CANARY).all(), 'canary of %s' % k
        out[k] = whole[pad:pad + sizes[k]].reshape(shapes[k])
    return out


def run_ops(device, labels, K, counts, mins, spacings, k_inv, rt_inv, H, W, near, step, n_steps, L, want=ARRAYS):
    to = lambda a: on(device, np.asarray(a, F32), torch.float32)
    out = pk.ops.grid_layers(on(device, labels), K, counts, mins, spacings, to(rt_inv), to(k_inv), H, W, float(near), float(step), n_steps,
                             L, want=want)
    assert sorted(out) == sorted(want) and all(t.dtype == torch.int32 for t in out.values())
    return {k: t.cpu().numpy() for k, t in out.items()}


def same(got, want, what, names=None):
    for name in (sorted(got) if names is None else names):
        g, w = got[name], want[name]
        assert g.dtype == I32 and g.shape == w.shape and np.array_equal(g, w), (what, name)


# ---------------------------------------------------------------------------------------------------------------- the matrix
def check_cell(device, counts, image, placements, n_steps, L, kind, want_set, rng, twin_handle=None):
    """One cell: ops.grid_layers twice, the raw entry point inside canaries with the arrays of `want_set` alone, all EQUAL to the
    restatement; with `twin_handle` also the g++ twin's raw call on host copies.  -> the restatement."""
    what = (counts, image, placements, n_steps, L, kind, want_set)
    H, W = image
    V = len(placements)
    labels, K = labels_of(kind, counts, L, rng)
    if V:
        cam_RT, cam_K = cameras(placements, counts, H, W)
        rt_inv, k_inv = yc.inverses(cam_RT, cam_K)
    else:
        rt_inv, k_inv = np.zeros((0, 4, 4), F32), np.zeros((0, 4, 4), F32)
    near, step = march_of(counts, n_steps)
    args = (labels, K, counts, MINS, SPACINGS, k_inv, rt_inv, H, W, near, step, n_steps, L)
    want = restate(*args)
    first, second = run_ops(device, *args), run_ops(device, *args)
    same(first, want, what)
    same(second, first, (what, 'twice'))
    if V:                                                 # (with no view the entry point is a no-op that writes nothing)
        same(run_raw(pk._lib.lib(), device, *args, want=want_set), want, (what, 'raw'))
        if twin_handle is not None:
            same(run_raw(twin_handle, 'cpu', *args, want=want_set), want, (what, 'twin'))
            same(run_raw(twin_handle, 'cpu', *args), want, (what, 'twin all'))
    return want


def matrix_cells(counts):
    """The cells of one grid: every image x every view count, the other factors cycled so that each of their values occurs; then
    every label kind and every L once more with all five placements at once."""
    cells, k = [], 0
    for image in IMAGES:
        for V in VIEW_COUNTS:
            placements = [PLACEMENTS[(k + j) % len(PLACEMENTS)] for j in range(V)]
            cells.append((image, placements, STEP_COUNTS[k % 3] if image != (20, 33) else 64, LAYER_COUNTS[k % 4],
                          LABEL_KINDS[(k * 3) % len(LABEL_KINDS)], OUTPUT_SETS[k % len(OUTPUT_SETS)]))
            k += 1
    for i, kind in enumerate(LABEL_KINDS):
        cells.append(((5, 7) if i % 2 else (16, 16), PLACEMENTS, 64 if i % 4 else 2, LAYER_COUNTS[i % 4], kind, OUTPUT_SETS[(i + 3) % len(OUTPUT_SETS)]))
    for i, L in enumerate(LAYER_COUNTS):
        cells.append(((5, 7), ['outside', 'inside', 'side'], 64, L, ('random', 'slabs', 'blobs', 'many')[i], OUTPUT_SETS[i]))
    cells.append(((5, 7), ['outside', 'inside'], 1, 4, 'one', ARRAYS))
    return cells


def check_matrix(counts, device, twin_handle=None):
    rng = np.random.default_rng(9000 + counts[0] * 10000 + counts[1] * 100 + counts[2])
    exact = overflowed = 0
    cells = matrix_cells(counts)
    for cell in cells:
        want = check_cell(device, counts, *cell, rng, twin_handle)
        # both branches of the CONTRACT, on the restatement's own output
        if want['status'][1] > 0:
            exact += int(want['status'][0] == 0)
            overflowed += int(want['status'][0] > 0)
    assert exact > 0 and overflowed > 0, (counts, exact, overflowed)
    return len(cells)


def check_more_objects_than_slots(device, twin_handle=None):
    """Every point an object of its own on the largest grid: one 16 x 16 tile meets more objects than the LDS gather table has
    slots (GATHER_SLOTS), so contributions go to the table directly; and K > GATHER_SLOTS objects that do fit, in slabs."""
    counts, (H, W) = (17, 9, 33), (16, 16)
    rng = np.random.default_rng(77)
    for L in (1, 8):
        want = check_cell(device, counts, (H, W), ['outside', 'inside'], 64, L, 'many', ARRAYS, rng, twin_handle)
        met = np.unique(want['label'][0][want['label'][0] >= 0]).size                      # the objects of view 0's one tile
        assert met > GATHER_SLOTS and pk._lib.LAYERS_CONSTANTS['GATHER_SLOTS'] == GATHER_SLOTS, met
    # labels that collide in the table: k and k + GATHER_SLOTS probe the same slots
    nx, ny, nz = counts
    labels = ((np.arange(nx * ny * nz) // (ny * nz)) * GATHER_SLOTS).astype(I32)             # slab ix -> object 32 ix
    K = nx * GATHER_SLOTS
    cam_RT, cam_K = cameras(['outside', 'side'], counts, H, W)
    rt_inv, k_inv = yc.inverses(cam_RT, cam_K)
    near, step = march_of(counts, 64)
    args = (labels, K, counts, MINS, SPACINGS, k_inv, rt_inv, H, W, near, step, 64, 8)
    want = restate(*args)
    assert np.unique(want['label'][want['label'] >= 0]).size > CONSTANTS['GATHER_PROBES']
    same(run_ops(device, *args), want, 'colliding labels')
    if twin_handle is not None:
        same(run_raw(twin_handle, 'cpu', *args), want, 'colliding labels, twin')


# ---------------------------------------------------------------------------------------------------------------- consequences
def x_camera(counts, H, W, f=40.0, back=1.0):
    """A camera on the -x side of the grid in raycast's frame that looks along +x through the grid's centre, the principal point at
    the centre pixel -> (cam_RT (1, 3, 4), cam_K (1, 3, 3), eye)."""
    lo, hi = yc.hull(counts)
    centre = 0.5 * (lo + hi)
    eye = np.array([lo[0] - back, centre[1], centre[2]])
    Rm = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])                      # camera z = world x
    cam_RT = np.concatenate([Rm, (-Rm @ eye)[:, None]], axis=1).astype(F32)[None]
    cam_K = np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]], F32)[None]
    return cam_RT, cam_K, eye


def x_slabs(counts, m, thick):
    """m slabs of `thick` points along x from ix = 0 on, -1 behind them."""
    ix = np.broadcast_to(np.arange(counts[0])[:, None, None], counts)
    return np.where(ix < m * thick, ix // thick, -1).astype(I32).reshape(-1)


def layers_of(device, labels, K, counts, cam_RT, cam_K, H, W, L, **kw):
    out = pk.projection.object_layers(on(device, labels), K, counts, MINS, SPACINGS, cam_RT, cam_K, H, W, max_layers=L, **kw)
    assert list(out) == ['label', 'first', 'samples', 'point', 'count', 'table', 'status', 'march']
    return {k: t.cpu().numpy() for k, t in out.items()}


def check_slabs_on_the_central_ray(device):
    """Slabs stacked along the view axis with exactly L - 1, L and L + 1 objects on the central ray: count there is L - 1, L and
    L + 1 (the overflow mark), the labels in the order of entry."""
    counts, (H, W) = (12, 7, 9), (11, 9)
    cam_RT, cam_K, _ = x_camera(counts, H, W)
    for L in LAYER_COUNTS:
        for m in (L - 1, L, L + 1):
            got = layers_of(device, x_slabs(counts, m, 1), max(m, 1), counts, cam_RT, cam_K, H, W, L)
            assert got['count'][0, 5, 4] == m, (L, m)
            kept = min(m, L)
            assert got['label'][0, 5, 4].tolist() == list(range(kept)) + [-1] * (L - kept), (L, m)
            assert (got['status'][0] > 0) == (m > L) and (got['first'][0, 5, 4, :kept] >= 0).all()
            assert (np.diff(got['first'][0, 5, 4, :kept]) > 0).all()


def check_table_from_pixels(device):
    """(1) With status[0] == 0 every column of the table is what numpy makes of label, first and the pixel indices, and the visible
    pixels of all objects are the pixels with any object."""
    rng = np.random.default_rng(31)
    counts, (H, W) = (17, 9, 33), (20, 33)
    cam_RT, cam_K = cameras(['outside', 'side', 'inside'], counts, H, W)
    seen = 0
    for kind, L in (('blobs', 8), ('slabs', 4), ('one', 1)):
        labels, K = labels_of(kind, counts, L - 1, rng)
        got = layers_of(device, labels, K, counts, cam_RT, cam_K, H, W, L)
        assert got['status'][0] == 0 and got['status'][1] > 0, kind
        assert np.array_equal(got['table'], table_of(got['label'], got['first'], K)), kind
        assert got['table'][:, :, 1].sum() == got['status'][1] == (got['count'] >= 1).sum()
        assert ((got['samples'] > 0) == (got['label'] >= 0)).all() and ((got['point'] >= 0) == (got['label'] >= 0)).all()
        assert np.array_equal(labels[got['point'][got['label'] >= 0]], got['label'][got['label'] >= 0])
        rate = pk.projection.occlusion_rate(got['table'])
        assert rate.dtype == F32 and np.array_equal(np.isnan(rate), got['table'][:, :, 0] == 0)
        assert ((rate[~np.isnan(rate)] >= 0) & (rate[~np.isnan(rate)] <= 1)).all()
        seen += int((got['count'] >= 2).sum())
    assert seen > 0


def check_prefix(device):
    """(2) For L' < L the layers of the L' call are the first L' of the L call in all four arrays, count' = min(count, L' + 1)."""
    rng = np.random.default_rng(32)
    counts, (H, W) = (17, 9, 33), (20, 33)
    cam_RT, cam_K = cameras(['outside', 'inside', 'side'], counts, H, W)
    for kind in ('random', 'blobs', 'slabs'):
        labels, K = labels_of(kind, counts, 8, rng)
        full = layers_of(device, labels, K, counts, cam_RT, cam_K, H, W, 8)
        assert (full['count'] >= 2).any(), kind
        for Lp in (4, 1):
            part = layers_of(device, labels, K, counts, cam_RT, cam_K, H, W, Lp)
            for name in PIXEL_ARRAYS:
                assert np.array_equal(part[name], full[name][..., :Lp]), (kind, Lp, name)
            assert np.array_equal(part['count'], np.minimum(full['count'], Lp + 1)), (kind, Lp)


def check_permutation(device):
    """(3) Relabelling the objects by a permutation permutes label's values and the table's rows; nothing else changes."""
    rng = np.random.default_rng(33)
    counts, (H, W) = (12, 7, 9), (16, 16)
    cam_RT, cam_K = cameras(['outside', 'side'], counts, H, W)
    for kind, L in (('random', 4), ('blobs', 8)):
        labels, K = labels_of(kind, counts, L, rng)
        perm = rng.permutation(K).astype(I32)
        relabelled = np.where(labels >= 0, perm[np.maximum(labels, 0)], labels).astype(I32)
        a = layers_of(device, labels, K, counts, cam_RT, cam_K, H, W, L)
        b = layers_of(device, relabelled, K, counts, cam_RT, cam_K, H, W, L)
        assert np.array_equal(b['label'], np.where(a['label'] >= 0, perm[np.maximum(a['label'], 0)], -1)), kind
        assert np.array_equal(b['table'][:, perm], a['table']), kind
        for name in ('first', 'samples', 'point', 'count', 'status'):
            assert np.array_equal(a[name], b[name]), (kind, name)
        assert same_float_bits(a['march'], b['march'])


def same_float_bits(a, b):
    return a.dtype == b.dtype == F32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_by_hand(device):
    """(4) Five two-point-thick slabs along x of the 12 x 7 x 9 grid, seen from the -x side along +x, 9 x 11 pixels, step = half the
    least spacing.  At the centre pixel count == 5 and the labels are 0 .. 4 in order; each layer's depth near + first * step lies in
    [D, D + step), D the analytic entry depth of the slab's cell union clipped to the grid's hull (a slack of 1e-5 for the float32
    rounding of a depth of a few units).  The objects behind slab 0 are never in front: VISIBLE == 0 < AMODAL."""
    counts, (H, W) = (12, 7, 9), (11, 9)
    cam_RT, cam_K, eye = x_camera(counts, H, W)
    step = 0.5 * min(SPACINGS)
    got = layers_of(device, x_slabs(counts, 5, 2), 5, counts, cam_RT, cam_K, H, W, 8, near=step, step=step)
    assert got['status'].tolist() == [0, int((got['count'] >= 1).sum())]
    assert got['count'][0, 5, 4] == 5 and got['label'][0, 5, 4].tolist() == [0, 1, 2, 3, 4, -1, -1, -1]
    depth = pk.projection.layer_depth(got['first'], got['march'])
    assert depth.dtype == F32 and np.array_equal(np.isnan(depth), got['first'] < 0)
    near32, step32 = got['march']
    assert near32 == F32(step) and step32 == F32(step)
    lo, hi = yc.hull(counts)
    for j in range(5):
        i = int(got['first'][0, 5, 4, j])
        assert depth[0, 5, 4, j].view(np.uint32) == (near32 + F32(i) * step32).view(np.uint32)         # d_i bit for bit
        D = max(MINS[0] + 2 * j * SPACINGS[0], lo[0]) - eye[0]
        assert D - 1e-5 <= float(depth[0, 5, 4, j]) < D + step + 1e-5, (j, i, D, float(depth[0, 5, 4, j]))
    table = got['table'][0]
    assert table[0, 1] == table[0, 0] > 0 and (table[1:, 1] == 0).all() and (table[1:, 0] > 0).all()
    rate = pk.projection.occlusion_rate(got['table'])[0]
    assert rate[0] == 0 and (rate[1:] == 1).all()
    # the masks and the pairs, numpy and torch
    label = got['label']
    for k in range(5):
        amodal, visible = pk.projection.amodal_mask(label, k), pk.projection.visible_mask(label, k)
        assert amodal.sum() == table[k, 0] and visible.sum() == table[k, 1] and not (visible & ~amodal).any()
        ys, xs = np.nonzero(amodal[0])
        assert table[k, 3:].tolist() == [xs.min(), xs.max(), ys.min(), ys.max()]
        t = torch.from_numpy(label)
        assert np.array_equal(pk.projection.amodal_mask(t, k).numpy(), amodal) and np.array_equal(pk.projection.visible_mask(t, k).numpy(), visible)
    pairs = pk.projection.occlusion_pairs(label, got['count'])
    assert pairs.dtype == np.int64 and pairs[:, :3].tolist() == [[0, 0, k] for k in range(1, 5)]
    assert pairs[:, 3].tolist() == [int(table[k, 0]) for k in range(1, 5)]
    assert np.array_equal(pk.projection.occlusion_pairs(torch.from_numpy(label)).numpy(), pairs)
    assert np.array_equal(pk.projection.layer_depth(torch.from_numpy(got['first']), torch.from_numpy(got['march'])).numpy().view(np.uint32),
                          depth.view(np.uint32))


def check_nothing_seen(device):
    """(5) Cameras that miss the grid or look away: all -1 / 0, the table at its fill values, status [0, 0]."""
    counts, (H, W) = (12, 7, 9), (20, 33)
    cam_RT, cam_K = cameras(['miss', 'behind'], counts, H, W)
    rt_inv, k_inv = yc.inverses(cam_RT, cam_K)
    near, step = march_of(counts, 64)
    got = run_ops(device, np.zeros(12 * 7 * 9, I32), 2, counts, MINS, SPACINGS, k_inv, rt_inv, H, W, near, step, 64, 4)
    for name in ('label', 'first', 'point'):
        assert (got[name] == -1).all(), name
    assert (got['samples'] == 0).all() and (got['count'] == 0).all() and got['status'].tolist() == [0, 0]
    assert np.array_equal(got['table'], np.tile(FILL, (2, 2, 1)))


def check_argument_errors(device):
    """(6) Each OCC4D_EINVAL with its message through ops.grid_layers (AssertionError with the library's text); the no-op cases."""
    counts, n = (3, 2, 5), 30
    z = lambda *s: torch.zeros(*s, device=device)
    lab = torch.zeros(n, dtype=torch.int32, device=device)
    call = lambda **k: pk.ops.grid_layers(**dict(dict(labels=lab, k=2, counts=counts, mins=MINS, spacings=SPACINGS, rt_inv=z(1, 16),
                                                      k_inv=z(1, 16), height=4, width=4, near=0.1, step=0.1, n_steps=4, max_layers=2), **k))
    for kw, text in ((dict(counts=(30, 1, 1)), 'occ4d_layers_march_i32: nx = 30, ny = 1, nz = 1 must be >= 2'),
                     (dict(step=0.0), 'step = 0 must be finite and > 0'), (dict(step=float('nan')), 'step = nan'),
                     (dict(near=float('inf')), 'near = inf must be finite'), (dict(n_steps=0), 'n_steps = 0 must be in 1 .. 65536'),
                     (dict(n_steps=65537), 'n_steps = 65537'), (dict(k=-1), 'K = -1 must be >= 0'),
                     (dict(max_layers=0), 'L = 0 must be in 1 .. 8'), (dict(max_layers=9), 'L = 9 must be in 1 .. 8'),
                     (dict(height=32769), 'H = 32769, W = 4 in 0 .. 32768')):
        with pytest.raises(AssertionError, match=text):
            call(**kw)
    for kw in (dict(rt_inv=z(0, 16), k_inv=z(0, 16)), dict(height=0), dict(width=0)):
        out = call(**kw)
        assert out['label'].numel() == 0 and out['count'].numel() == 0 and out['status'].tolist() == [0, 0]
        assert np.array_equal(out['table'].cpu().numpy(), np.tile(FILL, (out['table'].shape[0], 2, 1)))
    # the no-ops touch no pointer: nulls everywhere, and all outputs null with real inputs
    lib = pk._lib.lib()
    assert lib.occ4d_layers_march_i32(None, 3, 2, 5, 2, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, None, None, 0, 4, 4, 0.1, 0.1, 4, 2, *([None] * 7), None) == pk._lib.OK
    assert lib.occ4d_layers_march_i32(None, 3, 2, 5, 2, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, None, None, 3, 0, 4, 0.1, 0.1, 4, 2, *([None] * 7), None) == pk._lib.OK
    assert lib.occ4d_layers_march_i32(None, 3, 2, 5, 2, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, None, None, 3, 4, 4, 0.1, 0.1, 4, 2, *([None] * 7), None) == pk._lib.OK
    with pytest.raises(AssertionError, match="want = "):
        call(want=('depth',))


# ---------------------------------------------------------------------------------------------------------------- the option
def check_option():
    P = pk.projection
    cam_RT, cam_K = cameras(['outside', 'side'], (3, 2, 5), 4, 6)
    option = P.ObjectLayers(cam_RT, cam_K, 4, 6)
    assert (option.keyword, option.of, option.into, option.max_layers, option.step, option.arrays, P.ObjectLayers.reads_grid,
            P.ObjectLayers.clip_list) == ('layers', 'components', None, 4, None, ('label', 'first', 'count'), True,
                                          ('layer_images', 'one dict of layer images'))
    assert issubclass(P.ObjectLayers, pk.products.GridProduct) and 'segments' in repr(P.ObjectLayers(cam_RT, cam_K, 4, 6, of='segments'))
    assert P.ObjectLayers(cam_RT, cam_K, 4, 6, arrays=('count', 'samples')).arrays == ('samples', 'count')
    for kw in (dict(of='tracker'), dict(of=None), dict(max_layers=0), dict(max_layers=9), dict(max_layers=2.5), dict(max_layers=True),
               dict(arrays=('depth',)), dict(arrays=('table',))):
        with pytest.raises(ValueError, match='ObjectLayers: '):
            P.ObjectLayers(cam_RT, cam_K, 4, 6, **kw)
    P.ObjectLayers.check(option, ['components', 'layers'])
    with pytest.raises(ValueError, match="layers needs point_sample_mode 'grid'"):
        P.ObjectLayers.check(option, ['components', 'layers'], 'random')
    with pytest.raises(ValueError, match='layers needs components='):
        P.ObjectLayers.check(option, ['segments', 'layers'])
    with pytest.raises(ValueError, match='layers needs segments='):
        P.ObjectLayers.check(P.ObjectLayers(cam_RT, cam_K, 4, 6, of='segments'), ['components', 'layers'])
    option.of = 'clearance'                                                                # check looks at the instance
    with pytest.raises(ValueError, match="of = 'clearance' must be 'components' or 'segments'"):
        P.ObjectLayers.check(option, ['components', 'clearance', 'layers'])
    with pytest.raises(ValueError, match='layers must be a projection.ObjectLayers or None'):
        P.ObjectLayers.check(0.5, ['components'])


def check_signatures():
    """layers stands directly in front of boxes in perform_inference, layers and layer_images in evaluate_clip."""
    names = list(inspect.signature(pk.inference.perform_inference).parameters)
    assert names[-7:] == ['layers', 'boxes', 'next_view', 'sight', 'segments', 'tracker', 'clearance']
    names = list(inspect.signature(pk.evaluation.evaluate_clip).parameters)
    assert names[-11:] == ['layers', 'layer_images', 'boxes', 'next_view', 'next_views', 'sight', 'sights', 'segments', 'parts', 'route', 'routes']
    for fn in (pk.inference.perform_inference, pk.evaluation.evaluate_clip):
        assert inspect.signature(fn).parameters['layers'].default is None and 'layers' in fn.__doc__
    assert inspect.signature(pk.evaluation.evaluate_clip).parameters['layer_images'].default is None
    assert 'ObjectLayers' in pk.products.__doc__


# ---------------------------------------------------------------------------------------------------------------- end to end
IMAGE = yc.IMAGE


def fixture_option(shared, **kw):
    return pk.projection.ObjectLayers(*yc.fixture_cameras(shared), *IMAGE, **kw)


def without(result):
    return {k: v for k, v in result.items() if k not in ('components', 'segments', 'layers')}


def check_product(shared, got, option, of):
    """result['layers'] EQUAL to object_layers on the returned labels of the `of` product, and to the restatement."""
    device = shared.device
    mins, spacings = yc.frame_of(shared)
    layers, labels, K = got['layers'], got[of]['labels'], len(got[of]['table'])
    assert list(layers) == list(option.arrays) + ['table', 'status', 'march'] and all(isinstance(a, np.ndarray) for a in layers.values())
    assert K >= 2 and layers['table'].shape == (2, K, COLS) and layers['table'].dtype == I32 and layers['march'].dtype == F32
    alone = pk.projection.object_layers(on(device, labels), K, rc.COUNTS, mins, spacings, *yc.fixture_cameras(shared), *IMAGE,
                                        max_layers=option.max_layers, step=option.step)
    for name, a in layers.items():
        assert np.array_equal(a, alone[name].cpu().numpy()), name
    near, step, n_steps = pk.projection.march_range(rc.COUNTS, mins, spacings, option.rt64, step=option.step)
    assert same_float_bits(layers['march'], np.array([near, step], F32))
    want = restate(labels, K, rc.COUNTS, mins, spacings, option.k_inv, option.rt_inv, *IMAGE, near, step, n_steps, option.max_layers)
    same(layers, want, of, names=list(option.arrays) + ['table', 'status'])
    assert want['status'][1] > 0
    return want


def check_end_to_end(shared, monkeypatch):
    comp = pk.components.Components()
    option = fixture_option(shared, arrays=PIXEL_ARRAYS + ('count',), max_layers=8)
    calls = rc.count_waits(monkeypatch)
    res = rc.infer(shared.device, shared.inputs, components=comp, layers=option)
    assert calls['wait'] == 1                                                              # exactly one host wait
    monkeypatch.undo()
    check_product(shared, res, option, 'components')
    # every other key of the result is bit-equal with and without layers=
    alone = rc.infer(shared.device, shared.inputs, components=comp, layers=None)
    assert sorted(list(alone) + ['layers']) == sorted(res) and list(alone['components']) == list(res['components']) == ['labels', 'table']
    for k in alone['components']:
        assert np.array_equal(alone['components'][k], res['components'][k])
    rc.same_result(without(alone), shared.dense)
    rc.same_result(without(res), shared.dense)
    # of='segments' beside components; the default arrays; one layer: overflow is reported
    seg = pk.watershed.Segments(h=1)
    option = fixture_option(shared, of='segments', max_layers=1)
    res = rc.infer(shared.device, shared.inputs, components=comp, segments=seg, boxes=pk.components.Boxes(), layers=option)
    assert list(res['layers']) == ['label', 'first', 'count', 'table', 'status', 'march']
    assert list(res['components']) == ['labels', 'table', 'box', 'dirs']
    check_product(shared, res, option, 'segments')
    # under refine and in track_mode 'all': the labels are those of the expanded / merged array
    option = fixture_option(shared, step=0.05)
    res = rc.infer(shared.device, shared.inputs, refine=pk.inference.GridRefine(2, 0.46, 1), components=comp, layers=option)
    check_product(shared, res, option, 'components')
    res = rc.infer(shared.device, shared.inputs, track_mode='all', components=comp, layers=option)
    check_product(shared, res, option, 'components')
    rc.same_result(without(res), shared.dense_all)


def check_clip(shared):
    """evaluate_clip(components=..., objects=[], layers=..., layer_images=[]): one dict per output frame, that of the
    perform_inference call; the tuples of the clip as without."""
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = rc.clip_inputs(shared)
    run = lambda **kw: pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True, **kw)
    option, objects, images = fixture_option(shared), [], []
    clip = run(components=pk.components.Components(), objects=objects, layers=option, layer_images=images)
    dense = run()
    assert len(clip) == len(dense) == len(objects) == len(images) == 2
    for t in range(2):
        for got, want in zip(clip[t], dense[t]):
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        assert list(images[t]) == ['label', 'first', 'count', 'table', 'status', 'march']
        check_product(shared, dict(layers=images[t], components=objects[t]), option, 'components')
    with pytest.raises(ValueError, match='layer_images'):
        run(components=pk.components.Components(), objects=[], layers=option)
    with pytest.raises(ValueError, match='layers needs components='):
        run(layers=option, layer_images=[])


def check_none_is_untouched(shared, monkeypatch):
    """layers=None: no new key, one host wait, and neither the op nor the entry point is reached."""
    def forbidden(*a, **k):
        raise AssertionError('layers=None must not reach the layers entry point')
    monkeypatch.setattr(pk.ops, 'grid_layers', forbidden)
    L = pk._lib.lib()
    for name in SYMBOLS:
        monkeypatch.setattr(L, name, forbidden)
    calls = rc.count_waits(monkeypatch)
    res = rc.infer(shared.device, shared.inputs, layers=None)
    assert calls == dict(wait=1)
    assert sorted(res) == sorted(shared.dense)
    rc.same_result(res, shared.dense)
    res = rc.infer(shared.device, shared.inputs, components=pk.components.Components())
    assert list(res['components']) == ['labels', 'table'] and 'layers' not in res


def check_value_errors(shared):
    comp, option = pk.components.Components(), fixture_option(shared)
    with pytest.raises(ValueError, match='layers must be a projection.ObjectLayers or None'):
        rc.infer(shared.device, shared.inputs, components=comp, layers=comp)
    with pytest.raises(ValueError, match='layers needs components=<a components.Components>'):
        rc.infer(shared.device, shared.inputs, layers=option)
    with pytest.raises(ValueError, match='layers needs segments=<a watershed.Segments>'):
        rc.infer(shared.device, shared.inputs, components=comp, layers=fixture_option(shared, of='segments'))
    with pytest.raises(ValueError, match="needs point_sample_mode 'grid'"):
        rc.infer(shared.device, shared.inputs, components=comp, layers=option, point_sample_mode='random')
    with pytest.raises(ValueError, match='n_steps'):
        rc.infer(shared.device, shared.inputs, components=comp, layers=fixture_option(shared, step=1e-7))
