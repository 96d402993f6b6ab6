"""Shared by tests/test_sweep_host.py (through the g++ twin) and tests/test_gpu_sweep.py (on the device): the numpy float32
restatement of the sweep rules (include/ext/occ4d_sweep.h) in the stated operation order, written from the header -- vectorised over
the rays, looped over the samples, every sample walked --, the case matrix of the entry point, the placements, the hand-built owner
cells, the two checks that do not use the restatement (the analytic range and incidence on a linear field, the replay of points on
its level plane) and the end-to-end comparisons of perform_inference(sweep=...) on the refine fixture.
Everything but the two independent checks is compared EQUAL: the non-NaN floats bit for bit, the NaN positions as positions.

The ray directions go through libm's fmaf, one scalar at a time (as tests/raycast_cases.py does for its rays); the grid coordinate,
the cell, the lerp and the trilinear value are that module's restatements of the ray cast's rules, which the sweep takes over."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import raycast_cases as yc
import refine_cases as rc
import occlusions4d_amd as pk
from track_cases import same_bits, same_result

F32, I32 = np.float32, np.int32
GRIDS = yc.GRIDS                                         # (2, 2, 2), (3, 2, 5), (17, 9, 33)
SHAPES = [(1, 1), (1, 63), (1, 65), (8, 8), (9, 17), (7, 40)]      # (B, A): below and above a wave and a workgroup, ragged ends
VIEW_COUNTS = [0, 1, 3]
STEP_COUNTS = [1, 2, 64]
CHANNEL_COUNTS = [0, 1, 3]
SEM_COUNTS = [0, 1, 5]
LABEL_KINDS = ['null', 'in_range', 'mixed']             # mixed: also < 0 and >= K
FIELDS = ['air', 'solid', 'blob', 'nans']
PLACEMENTS = ['outside', 'free', 'solid', 'on_point']
NAMES = ('range', 'point', 'cell', 'owner', 'cos', 'sem', 'inst', 'features')
OUTPUT_SETS = [NAMES] + [(name,) for name in NAMES]
D, PAD, SENTINEL = yc.D, yc.PAD, yc.SENTINEL
LEVEL, MINS, SPACINGS = yc.LEVEL, yc.MINS, yc.SPACINGS
K_OBJECTS = 4
BG, FBG = -1.5, -2.5
SYMBOLS = ['occ4d_sweep_rays_f32']
CONSTANTS = dict(MAX_STEPS=65536, MAX_CHANNELS=32)

_fmaf = yc._fmaf


# ---------------------------------------------------------------------------------------------------------------- restatement
def ray_directions(pose, dirs, R, per_view):
    """(P0, dir), both (V * R, 3) float32: RAYS of the header, the fused chain through libm's fmaf."""
    pose = np.asarray(pose, F32).reshape(-1, 12)
    dirs = np.asarray(dirs, F32).reshape(-1, 3)
    V = pose.shape[0]
    P0, direction = np.zeros((V * R, 3), F32), np.zeros((V * R, 3), F32)
    fma = lambda x, y, z: F32(_fmaf(float(x), float(y), float(z)))
    with np.errstate(all='ignore'):
        for v in range(V):
            Rm = pose[v].reshape(3, 4)
            for r in range(R):
                d = dirs[v * R + r if per_view else r]
                P0[v * R + r] = Rm[:, 3]
                for a in range(3):
                    direction[v * R + r, a] = fma(Rm[a, 2], d[2], fma(Rm[a, 1], d[1], F32(Rm[a, 0]) * F32(d[0])))
    return P0, direction


def march(field, counts, mins, spacings, level, P0, direction, near, step, n_steps):
    """SAMPLES, IN, VALUE and HIT of the ray cast's header for rays (P0, dir) -> (hit (n,) bool, range (n,) float32)."""
    level, near, step = F32(level), F32(near), F32(step)
    top = np.asarray(counts, F32) - F32(1)
    n = P0.shape[0]
    rng_, hit = np.zeros(n, F32), np.zeros(n, bool)
    prev_in, prev_v = np.zeros(n, bool), np.zeros(n, F32)
    with np.errstate(all='ignore'):
        for i in range(n_steps):                                      # every sample is walked; rays that have hit are masked
            live = ~hit
            d = near + F32(i) * step
            g = yc.grid_coords(P0 + d * direction, mins, spacings)
            inside = ((F32(0) <= g) & (g <= top)).all(axis=1)
            v = np.zeros(n, F32)
            c, w = yc.cells_of(g[inside], counts)
            v[inside] = yc.trilinear(field, counts, c, w)
            now = live & inside & (v >= level)
            refine = now & prev_in & (prev_v < level) & (i >= 1)
            t = (level - prev_v) / (v - prev_v)
            t = np.where((t >= F32(0)) & (t <= F32(1)), t, F32(0.5)).astype(F32)
            d0 = near + F32(i - 1) * step
            rng_[now] = np.where(refine, d0 + t * (d - d0), d).astype(F32)[now]
            hit |= now
            prev_in = np.where(live, inside, prev_in)
            prev_v = np.where(live, v, prev_v).astype(F32)
    return hit, rng_


def restate(field, counts, mins, spacings, level, pose, dirs, shape, per_view, near, step, n_steps, attrs=None, cols=(), sem=None,
            labels=None, K=0, background=0.0, feature_background=None):
    """dict(range, point, cell, owner, cos, features[, sem][, inst], hit) of the header, (V, R) each unless shaped otherwise."""
    field = np.asarray(field, F32)
    pose = np.asarray(pose, F32).reshape(-1, 12)
    V, R = pose.shape[0], shape[0] * shape[1]
    nx, ny, nz = counts
    top = np.asarray(counts, F32) - F32(1)
    sp = np.asarray(spacings, F32)
    P0, direction = ray_directions(pose, dirs, R, per_view)
    hit, rng_ = march(field, counts, mins, spacings, level, P0, direction, near, step, n_steps)
    n = V * R
    lerp = yc.lerp
    with np.errstate(all='ignore'):
        point = (P0 + rng_[:, None] * direction).astype(F32)
        g = np.fmin(np.fmax(yc.grid_coords(point, mins, spacings), F32(0)), top)
        c, w = yc.cells_of(g, counts)
        flat = (c[:, 0] * ny + c[:, 1]) * nz + c[:, 2]
        wx, wy, wz = w[:, 0], w[:, 1], w[:, 2]
        f = [field[flat + ((j >> 2) * ny + ((j >> 1) & 1)) * nz + (j & 1)] for j in range(8)]       # index x * 4 + y * 2 + z
        gx = lerp(lerp(f[4] - f[0], f[5] - f[1], wz), lerp(f[6] - f[2], f[7] - f[3], wz), wy) / sp[0]
        gy = lerp(lerp(f[2] - f[0], f[3] - f[1], wz), lerp(f[6] - f[4], f[7] - f[5], wz), wx) / sp[1]
        gz = lerp(lerp(f[1] - f[0], f[3] - f[2], wy), lerp(f[5] - f[4], f[7] - f[6], wy), wx) / sp[2]
        dx, dy, dz = direction[:, 0], direction[:, 1], direction[:, 2]
        nd = gx * dx + gy * dy + gz * dz
        nn = gx * gx + gy * gy + gz * gz
        dd = dx * dx + dy * dy + dz * dz
        den = np.sqrt(nn * dd)
        cos = np.where(den > F32(0), np.fmin(np.abs(nd) / den, F32(1)), F32(0)).astype(F32)
        best, k = np.full(n, -np.inf, F32), np.zeros(n, np.int64)
        for j in range(8):
            take = f[j] > best
            best, k = np.where(take, f[j], best), np.where(take, j, k)
        owner = flat + ((k >> 2) * ny + ((k >> 1) & 1)) * nz + (k & 1)
        fbg = background if feature_background is None else feature_background
        feat = np.full((n, len(cols)), fbg, F32)
        for j, col in enumerate(cols):
            feat[hit, j] = yc.trilinear(np.ascontiguousarray(attrs[:, col]), counts, c[hit], w[hit])
    out = dict(hit=hit.reshape(V, R),
               range=np.where(hit, rng_, F32(background)).astype(F32).reshape(V, R),
               point=np.where(hit[:, None], point, F32(background)).astype(F32).reshape(V, R, 3),
               cell=np.where(hit, flat, -1).astype(I32).reshape(V, R), owner=np.where(hit, owner, -1).astype(I32).reshape(V, R),
               cos=np.where(hit, cos, F32(0)).astype(F32).reshape(V, R), features=feat.reshape(V, R, len(cols)))
    if sem is not None and sem[1] > 0:
        block = np.asarray(attrs, F32)[owner, sem[0]:sem[0] + sem[1]]
        m, s = block[:, 0].copy(), np.zeros(n, np.int64)
        for j in range(1, sem[1]):
            take = block[:, j] > m
            m, s = np.where(take, block[:, j], m), np.where(take, j, s)
        out['sem'] = np.where(hit, s, -1).astype(I32).reshape(V, R)
    if labels is not None:
        lab = np.asarray(labels, np.int64)[owner]
        out['inst'] = np.where(hit & (lab >= 0) & (lab < K), lab, -1).astype(I32).reshape(V, R)
    return out


def same(got, want, tag=None, names=None):
    """got: name -> numpy array for the outputs that were asked for."""
    for name in (got if names is None else names):
        a, b = got[name], want[name]
        if b.dtype == F32:
            assert same_bits(a, b), (name, tag)
        else:
            assert a.dtype == I32 and a.shape == b.shape and np.array_equal(a, b), (name, tag)


# ---------------------------------------------------------------------------------------------------------------- inputs
def rotation(rng):
    """A proper rotation (3, 3) float64."""
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def facing(origin, target):
    """The rotation (3, 3) float64 whose sensor x axis points from origin to target, z as far up as that allows."""
    x = np.asarray(target, np.float64) - np.asarray(origin, np.float64)
    x /= np.linalg.norm(x)
    y = np.cross([0.0, 0.0, 1.0], x)
    y /= np.linalg.norm(y)
    return np.stack([x, y, np.cross(x, y)], axis=1)


def pose_of(origin, Rm=None):
    """(12,) float32 [Rm | t]."""
    Rm = np.eye(3) if Rm is None else Rm
    return np.concatenate([Rm, np.asarray(origin, np.float64)[:, None]], axis=1).reshape(12).astype(F32)


def blob(counts, rng, mins=MINS, spacings=SPACINGS):
    """A smooth field: high round a random centre inside the grid, low far from it, plus a little noise."""
    lo, hi = yc.hull(counts, mins, spacings)
    axes = [np.linspace(l, h, c) for l, h, c in zip(lo, hi, counts)]
    X, Y, Z = np.meshgrid(*axes, indexing='ij')
    u = rng.uniform(0.25, 0.75, size=3)
    r = np.sqrt(sum(((A - (l + t * (h - l))) / max(h - l, 1e-9)) ** 2 for A, l, h, t in zip((X, Y, Z), lo, hi, u)))
    peak, slope = (1.25, 0.8) if min(counts) < 3 else (0.95, 1.1)          # (a grid of one cell has no point near its centre)
    return (peak - slope * r + rng.uniform(-0.02, 0.02, size=r.shape)).astype(F32).reshape(-1)


def field_of(kind, counts, rng):
    n = counts[0] * counts[1] * counts[2]
    if kind == 'air':
        return yc.fields('all_below', n, rng)
    if kind == 'solid':
        return yc.fields('all_above', n, rng)
    if kind == 'nans':
        return yc.fields('pool', n, rng)                 # the level and its neighbours, zeros, NaN, infinities, finite values
    return blob(counts, rng)


def origin_of(placement, counts, field, rng, mins=MINS, spacings=SPACINGS):
    """The sensor origin (3,) float64 of one placement round / in the grid."""
    lo, hi = yc.hull(counts, mins, spacings)
    centre, ext = 0.5 * (lo + hi), hi - lo
    if placement == 'outside':
        return centre + np.array([-0.9, -0.7, 0.6]) * float(np.linalg.norm(ext))
    vol = np.asarray(field, F32).reshape(counts)
    finite = np.where(np.isnan(vol), -np.inf, vol)
    idx = np.unravel_index(int(np.argmin(finite) if placement == 'free' else np.argmax(finite)), counts)
    at = np.array([m + (i + 0.5) * s for m, i, s in zip(mins, idx, spacings)])
    if placement == 'on_point':
        idx = tuple(int(rng.integers(0, c)) for c in counts)
        return np.array([F32(F32(i) + F32(0.5)) * F32(s) + F32(m) for m, i, s in zip(mins, idx, spacings)], np.float64)
    # free: just off the lowest point; solid: from the highest point a step towards the middle, so that rays of every direction
    # stay in the grid for their first sample
    return at + (0.01 * ext if placement == 'free' else 0.15 * (centre - at))


def placed(placement, counts, field, rng):
    """The pose (12,) float32 of one placement: from outside the sensor faces the grid, elsewhere it is turned at random."""
    origin = origin_of(placement, counts, field, rng)
    if placement == 'outside':
        lo, hi = yc.hull(counts)
        return pose_of(origin, facing(origin, 0.5 * (lo + hi)))
    return pose_of(origin, rotation(rng))


def bundle(shape, rng, V=1, per_view=False):
    """A lidar table (B * A, 3) -- or V of them, each spread differently -- of unit vectors that is AIMED: one beam lies within a
    degree of elevation 0 and one azimuth within a degree of 0, so a sensor that faces the grid has rays through its middle, also
    with one beam and however small the grid is; the other beams and azimuths go round and past it."""
    B, A = shape
    tables = []
    for _ in range(V if per_view else 1):
        delta, m = rng.uniform(3.0, 10.0), int(rng.integers(0, B))                  # beam m is the one at elevation ~0
        el0, az0 = rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0) - (A // 2) * 360.0 / A
        tables.append(pk.sweep.lidar_directions(B, A, el0 + m * delta, el0 - (B - 1 - m) * delta, (az0, az0 + 360.0)))
    return np.concatenate(tables).reshape(-1, 3)


def march_of(counts, n_steps):
    return yc.march_of(counts, n_steps)


def labels_of(kind, n, rng):
    if kind == 'null':
        return None
    if kind == 'in_range':
        return rng.integers(0, K_OBJECTS, size=n).astype(I32)
    labels = rng.integers(0, K_OBJECTS, size=n).astype(I32)
    foreign = rng.uniform(size=n) < 0.3                                 # about a third of the points: < 0 or >= K
    labels[foreign] = rng.choice(np.array([-3, -1, K_OBJECTS, K_OBJECTS + 2, 2 ** 31 - 1, -2 ** 31], np.int64), size=int(foreign.sum())).astype(I32)
    return labels


def raw_call(device, field_view, ld, counts, mins, spacings, level, pose, dirs, shape, per_view, near, step, n_steps, attrs_view=None,
             ld_attr=0, d=0, cols=(), sem=None, labels=None, K=0, background=0.0, feature_background=0.0, want=NAMES, guard=3):
    """The entry point as it is, each output null unless `want` names it, sentinel guards round every output -> name -> numpy."""
    L, p = pk._lib.lib(), pk.ops._ptr
    pose = np.asarray(pose, F32).reshape(-1, 12)
    V, (B, A), C = pose.shape[0], shape, len(cols)
    R = B * A
    rays = V * R
    dev = lambda a, dt=F32: torch.from_numpy(np.ascontiguousarray(a, dt)).to(device)
    sem_first, n_sem = (0, 0) if sem is None else sem
    specs = dict(range=((V, R), F32, SENTINEL), point=((V, R, 3), F32, SENTINEL), cell=((V, R), I32, -7), owner=((V, R), I32, -7),
                 cos=((V, R), F32, SENTINEL), sem=((V, R), I32, -7), inst=((V, R), I32, -7), features=((V, R, C), F32, SENTINEL))
    bufs = {name: torch.full((int(np.prod(s)) + 2 * guard,), fill, dtype=torch.float32 if dt == F32 else torch.int32, device=device)
            for name, (s, dt, fill) in specs.items()}
    pose_t, dirs_t = dev(pose), dev(np.asarray(dirs, F32).reshape(-1, 3))
    lab_t = None if labels is None else dev(labels, I32)
    arr = (ctypes.c_int32 * C)(*cols) if C else None
    status = L.occ4d_sweep_rays_f32(
        p(field_view), ld, *counts, mins[0], spacings[0], mins[1], spacings[1], mins[2], spacings[2], float(level), p(pose_t), p(dirs_t),
        V, B, A, int(per_view), float(near), float(step), n_steps, p(attrs_view), ld_attr, d, arr, C, sem_first, n_sem, p(lab_t), K,
        float(background), float(feature_background), *(p(bufs[name][guard:]) if name in want else None for name in NAMES),
        pk.ops._stream())
    assert status == pk._lib.OK, L.occ4d_last_error()
    written = set(want) - ({'sem'} if n_sem == 0 else set()) - ({'inst'} if labels is None else set()) - ({'features'} if C == 0 else set())
    out = {}
    for name, (s, dt, fill) in specs.items():
        a = bufs[name].cpu().numpy()
        assert (a[:guard] == fill).all() and (a[len(a) - guard:] == fill).all(), name
        if name not in written:
            assert (a == fill).all(), name                          # an output that is not asked for is not touched
        elif name in want:
            out[name] = a[guard:len(a) - guard].reshape(s)
    if 'features' in want and C == 0:
        out['features'] = np.zeros((V, R, 0), F32)
    return out


# ---------------------------------------------------------------------------------------------------------------- the matrix
def check_cell(device, counts, shape, placements, per_view, n_steps, C, n_sem, label_kind, strided, kind, want, rng):
    """One cell: the raw entry point inside canaries when strided or when not all outputs are asked for, ops.sweep_rays otherwise.
    -> the restatement."""
    tag = (counts, shape, placements, per_view, n_steps, C, n_sem, label_kind, strided, kind, want)
    n = counts[0] * counts[1] * counts[2]
    V = len(placements)
    field = field_of(kind, counts, rng)
    attrs, cols = yc.attributes(n, rng), yc.columns(C, rng)
    sem = (D - n_sem, n_sem) if n_sem else None
    labels = labels_of(label_kind, n, rng)
    pose = np.stack([placed(pl, counts, field, rng) for pl in placements]) if V else np.zeros((0, 12), F32)
    dirs = bundle(shape, rng, V, per_view) if (V or not per_view) else np.zeros((0, 3), F32)
    near, step = march_of(counts, n_steps)
    expect = restate(field, counts, MINS, SPACINGS, LEVEL, pose, dirs, shape, per_view, near, step, n_steps, attrs, cols, sem, labels,
                     K_OBJECTS, BG, FBG)
    field_buf, field_view = yc.padded(device, field[:, None], strided)
    attr_buf, attr_view = yc.padded(device, attrs, strided)
    need_attrs = C or n_sem
    if strided or tuple(want) != NAMES:
        got = raw_call(device, field_view, field_buf.stride(0), counts, MINS, SPACINGS, LEVEL, pose, dirs, shape, per_view, near, step,
                       n_steps, attr_view if need_attrs else None, attr_buf.stride(0) if need_attrs else 0, D if need_attrs else 0, cols,
                       sem, labels, K_OBJECTS, BG, FBG, want)
    else:
        to = lambda a, dt=F32: torch.from_numpy(np.ascontiguousarray(a, dt)).to(device)
        got = pk.ops.sweep_rays(field_view[:, 0], counts, MINS, SPACINGS, float(LEVEL), to(pose), to(dirs), shape, float(near), float(step),
                                n_steps, per_view=per_view, attrs=attr_view if need_attrs else None, channels=cols, sem=sem,
                                labels=None if labels is None else to(labels, I32), k=K_OBJECTS, background=BG, feature_background=FBG)
        assert got['range'].shape == (V, shape[0] * shape[1]) and got['features'].shape == (V, shape[0] * shape[1], C), tag
        assert ('sem' in got) == bool(n_sem) and ('inst' in got) == (labels is not None), tag
        got = {name: t.cpu().numpy() for name, t in got.items()}
    assert set(got) == {name for name in want if name in expect}, tag
    same(got, expect, tag)
    for a in got.values():                                 # no sentinel from the padding in any output
        assert not (a == SENTINEL).any(), tag
    assert (field_buf.cpu().numpy()[:, 1:] == SENTINEL).all() and (attr_buf.cpu().numpy()[:, D:] == SENTINEL).all(), tag
    if kind == 'air':
        assert not expect['hit'].any(), tag
    return expect


def matrix_cells(counts):
    """The cells of one grid: every shape x every view count, the other factors cycled so that each of their values occurs."""
    cells, k = [], 0
    for shape in SHAPES:
        for V in VIEW_COUNTS:
            placements = [PLACEMENTS[(k + j) % len(PLACEMENTS)] for j in range(V)]
            cells.append((shape, placements, k % 2 == 1, STEP_COUNTS[(k + 1) % 3] if shape != (7, 40) else 64, CHANNEL_COUNTS[k % 3],
                          SEM_COUNTS[(k // 2) % 3], LABEL_KINDS[(k // 3) % 3], (k // 2) % 2 == 1, FIELDS[(k + 2) % 4],
                          OUTPUT_SETS[0]))
            k += 1
    # every output alone, and the remaining combinations on the blob with all placements at once
    for j, want in enumerate(OUTPUT_SETS[1:]):
        cells.append(((9, 17), ['outside', 'solid', 'free'], j % 2 == 0, 64, 3, 5, 'mixed', True, 'blob', want))
    for j, kind in enumerate(FIELDS):
        cells.append(((8, 8), PLACEMENTS, j % 2 == 1, 64, CHANNEL_COUNTS[j % 3], SEM_COUNTS[(j + 1) % 3], LABEL_KINDS[(j + 2) % 3], False,
                      kind, OUTPUT_SETS[0]))
    cells.append(((1, 65), ['outside', 'on_point'], False, 64, 1, 1, 'in_range', False, 'blob', OUTPUT_SETS[0]))
    return cells


# chosen on the CPU so that the RESTATEMENT alone satisfies check_matrix's coverage condition
SEEDS = {(2, 2, 2): 9100, (3, 2, 5): 9100, (17, 9, 33): 9100}


def seed_of(counts):
    return SEEDS[tuple(counts)]


def check_matrix(counts, device):
    """The cells of one grid, which hold every value of every factor, and the coverage condition ON THE RESTATEMENT: EVERY blob cell
    with labels and a view has a return (with labels all in range: inst >= 0 at every one); over the blob cells there are hits and
    misses and, at the hits, inst >= 0 and inst == -1.  The seeds are chosen so that the restatement alone satisfies it."""
    rng = np.random.default_rng(seed_of(counts))
    cells = matrix_cells(counts)
    assert {c[0] for c in cells} == set(SHAPES) and {len(c[1]) for c in cells} >= set(VIEW_COUNTS)
    assert {p for c in cells for p in c[1]} == set(PLACEMENTS) and {c[2] for c in cells} == {False, True}
    assert {c[3] for c in cells} == set(STEP_COUNTS) and {c[4] for c in cells} == set(CHANNEL_COUNTS)
    assert {c[5] for c in cells} == set(SEM_COUNTS) and {c[6] for c in cells} == set(LABEL_KINDS)
    assert {c[7] for c in cells} == {False, True} and {c[8] for c in cells} == set(FIELDS) and {c[9] for c in cells} == set(OUTPUT_SETS)
    hits = misses = with_inst = without_inst = 0
    for cell in cells:
        expect = check_cell(device, counts, *cell, rng)
        if cell[8] == 'blob' and len(cell[1]):
            hit = expect['hit']
            hits, misses = hits + int(hit.sum()), misses + int((~hit).sum())
            if 'inst' in expect:
                assert hit.any(), (counts, cell)
                if cell[6] == 'in_range':
                    assert (expect['inst'][hit] >= 0).all(), (counts, cell)
                with_inst += int((expect['inst'][hit] >= 0).sum())
                without_inst += int((expect['inst'][hit] < 0).sum())
    assert hits > 0 and misses > 0 and with_inst > 0 and without_inst > 0, (counts, hits, misses, with_inst, without_inst)
    return len(cells)


# ---------------------------------------------------------------------------------------------------------------- placements
EXACT_MINS, EXACT_SPACINGS = yc.EXACT_MINS, yc.EXACT_SPACINGS


def call(device, field, counts, mins, spacings, level, pose, dirs, shape, near, step, n_steps, **kw):
    to = lambda a, dt=F32: torch.from_numpy(np.ascontiguousarray(a, dt)).to(device)
    if kw.get('labels') is not None:
        kw['labels'] = to(kw['labels'], I32)
    if kw.get('attrs') is not None:
        kw['attrs'] = to(kw['attrs'])
    got = pk.ops.sweep_rays(to(field), counts, mins, spacings, float(level), to(np.asarray(pose, F32).reshape(-1, 12)), to(dirs), shape,
                            float(near), float(step), n_steps, **kw)
    return {name: t.cpu().numpy() for name, t in got.items()}


def check_placements(device):
    """What each placement is there for, on the blob of the large grid: from outside the bundle hits and misses; inside free space
    it hits beyond the first sample; inside the solid the first sample is solid and range == near on every ray; on a grid point the
    results equal the restatement (the matrix) and a zero step count of in-grid samples is no error."""
    counts, shape = (17, 9, 33), (9, 17)
    rng = np.random.default_rng(12)
    field = blob(counts, rng)
    dirs = bundle(shape, rng)
    near, step = march_of(counts, 64)
    seen = {}
    for placement in PLACEMENTS:
        pose = placed(placement, counts, field, rng)[None]
        expect = restate(field, counts, MINS, SPACINGS, LEVEL, pose, dirs, shape, False, near, step, 64, background=BG)
        got = call(device, field, counts, MINS, SPACINGS, LEVEL, pose, dirs, shape, near, step, 64, background=BG)
        same(got, expect, placement)
        seen[placement] = expect
    assert seen['outside']['hit'].any() and not seen['outside']['hit'].all()
    assert seen['free']['hit'].any() and (seen['free']['range'][seen['free']['hit']] > near).all()
    assert seen['solid']['hit'].all() and (seen['solid']['range'] == near).all()
    # near = 0: the first sample is the origin itself
    pose = pose_of(origin_of('solid', counts, field, rng))[None]
    got = call(device, field, counts, MINS, SPACINGS, LEVEL, pose, dirs, shape, 0.0, step, 4, background=BG)
    assert (got['range'] == 0.0).all() and (got['point'] == pose[0].reshape(3, 4)[:, 3]).all() and len(np.unique(got['cell'])) == 1


def check_axis_rays_through_grid_points(device):
    """The frame whose points are exact floats (point i of an axis at i / 4), the identity pose ON grid point (0, 0, 0), rays along
    +x, +y, +z with step 0.25: every sample lies on a grid point and takes that point's own value; the hit cell is limited to n - 2
    at g = n - 1.  Compared with the restatement, and the range with the first solid point of the line by hand."""
    rng = np.random.default_rng(13)
    dirs = np.eye(3, dtype=F32)
    for counts in GRIDS:
        n = counts[0] * counts[1] * counts[2]
        field = yc.fields('pool', n, rng)
        pose = pose_of((0.0, 0.0, 0.0))[None]
        n_steps = max(counts) + 3
        expect = restate(field, counts, EXACT_MINS, EXACT_SPACINGS, LEVEL, pose, dirs, (1, 3), False, 0.0, 0.25, n_steps, background=BG)
        got = call(device, field, counts, EXACT_MINS, EXACT_SPACINGS, LEVEL, pose, dirs, (1, 3), 0.0, 0.25, n_steps, background=BG)
        same(got, expect, counts)
        vol = field.reshape(counts)
        for a in range(3):
            line = np.moveaxis(vol, a, 0)[:, 0, 0]
            solid = np.flatnonzero(line >= LEVEL)               # (a NaN is not solid)
            if solid.size == 0:
                assert got['cell'][0, a] == -1
            elif solid[0] == 0 or not line[solid[0] - 1] < LEVEL:   # no refinement: the sample on the point itself
                assert got['range'][0, a] == F32(0.25) * F32(solid[0]), (counts, a)
            assert got['cell'].max() <= (counts[0] - 2) * counts[1] * counts[2] + (counts[1] - 2) * counts[2] + counts[2] - 2


def check_zero_and_nan_directions(device):
    """A zero direction: every sample is the origin, a hit at near iff the origin's own sample is solid, point == the origin, cos 0
    (den is 0).  A NaN direction: no sample is in the grid, no hit.  Neither reads outside the field (the canaries of the raw call)."""
    counts = (5, 5, 5)
    rng = np.random.default_rng(14)
    vol = rng.uniform(-0.3, 0.2, size=counts).astype(F32)
    vol[2, 2, 2] = 0.9                                      # the one solid point, inside: the 'solid' origin lies on it
    field = vol.reshape(-1)
    dirs = np.array([[0, 0, 0], [np.nan, 0, 1], [0, np.nan, 0], [np.inf, 1, 0], [1, 0, 0], [-0.0, 0.0, 0.0]], F32)
    near, step = march_of(counts, 64)
    for placement in ('solid', 'free', 'outside'):
        pose = pose_of(origin_of(placement, counts, field, rng))[None]
        expect = restate(field, counts, MINS, SPACINGS, LEVEL, pose, dirs, (1, 6), False, near, step, 64, background=BG)
        buf, view = yc.padded(device, field[:, None], True)
        got = raw_call(device, view, buf.stride(0), counts, MINS, SPACINGS, LEVEL, pose, dirs, (1, 6), False, near, step, 64,
                       background=BG, want=('range', 'point', 'cell', 'owner', 'cos'))
        same(got, expect, placement)
        for r in (0, 5):
            assert bool(got['cell'][0, r] >= 0) == (placement == 'solid'), placement
            assert got['cos'][0, r] == 0.0
        if placement == 'solid':
            assert got['range'][0, 0] == near and (got['point'][0, 0] == pose[0].reshape(3, 4)[:, 3]).all()
        assert (got['cell'][0, 1:4] == -1).all(), placement


# ---------------------------------------------------------------------------------------------------------------- owner
def one_cell(device, corners, labels=None, attrs=None, sem=None, at=(0.5, 0.5, 0.5)):
    """A 2 x 2 x 2 grid in the exact frame with the given corner values (index x * 4 + y * 2 + z), a ray along +x from x = -1 whose
    samples (step 0.125) enter the cell at (0, at_y, at_z) cell units -> the outputs of that one ray."""
    field = np.asarray(corners, F32)
    origin = (-1.0, 0.25 * at[1], 0.25 * at[2])
    return call(device, field, (2, 2, 2), EXACT_MINS, EXACT_SPACINGS, LEVEL, pose_of(origin)[None], np.array([[1, 0, 0]], F32), (1, 1),
                0.0, 0.125, 16, labels=labels, k=8, attrs=attrs, sem=sem, background=BG)


def check_owner(device):
    """Hand-built cells: the greatest corner wins, ties go to the first in the order (0,0,0), (0,0,1), ..., all corners equal give
    corner 0; sem and inst are the argmax / the label gathered at owner."""
    labels = np.arange(8, dtype=I32)[::-1].copy()
    attrs = np.random.default_rng(15).uniform(-1, 1, size=(8, 6)).astype(F32)
    attrs[3, 2] = attrs[3, 4] = 5.0                                                    # a tie between classes: the first wins
    for corners, owner in (
            ([0.9, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7], 0),
            ([0.5, 0.6, 0.7, 0.95, 0.6, 0.5, 0.5, 0.5], 3),
            ([0.5, 0.8, 0.5, 0.8, 0.8, 0.5, 0.5, 0.8], 1),                                  # a three-way tie: corner (0, 0, 1)
            ([0.1, 0.1, 0.1, 0.1, 0.9, 0.9, 0.9, 0.9], 4),                                  # a face: its first corner
            ([0.6] * 8, 0)):                                                                # all equal: corner 0
        got = one_cell(device, corners, labels, attrs, (1, 5))
        tag = (corners, owner, got)
        assert got['cell'][0, 0] == 0 and got['owner'][0, 0] == owner, tag
        assert got['inst'][0, 0] == labels[owner] and got['sem'][0, 0] == int(np.argmax(attrs[owner, 1:6])), tag
    got = one_cell(device, [0.5, 0.5, 0.5, 0.95, 0.5, 0.5, 0.5, 0.5], labels, attrs, (1, 5))
    assert got['owner'][0, 0] == 3 and got['sem'][0, 0] == 1                              # columns 2 and 4 tie: class 2 - 1 = 1
    got = one_cell(device, [np.nan] * 8, labels)                                            # no sample is >= level: no hit at all
    assert got['cell'][0, 0] == -1 and got['owner'][0, 0] == -1 and got['inst'][0, 0] == -1


def check_owner_of_a_skipped_cell(device):
    """A NaN corner poisons every sample of its cell, so a hit cell with NaN corners is one the samples stepped over: a 6 x 2 x 2
    grid in the exact frame, a ray along +x with two samples, at x = 0.1 (cell 0, all 0) and x = 1.1 (cell 4, all 0.92 = 2 level):
    t = 0.5, the hit position x = 0.6 lies in cell 2, whose eight corners no sample has read.  A NaN never wins, all NaN (or
    -inf) give corner 0, and cos is 0 where the gradient is NaN."""
    counts = (6, 2, 2)
    nan, inf = np.nan, np.inf
    pose, dirs = pose_of((-0.9, 0.125, 0.125))[None], np.array([[1, 0, 0]], F32)
    labels = np.arange(24, dtype=I32)
    for corners, corner in (([nan] * 8, 0), ([nan, 0.7, nan, 0.7, 0.9, nan, 0.9, 0.2], 4), ([nan] * 7 + [-inf], 0),
                            ([nan, -inf, 0.1, nan, nan, 0.1, nan, nan], 2), ([inf, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, inf], 0),
                            ([nan, nan, nan, nan, nan, nan, nan, -5.0], 7)):
        vol = np.zeros(counts, F32)
        vol[4:] = F32(2) * LEVEL
        vol[2:4] = np.asarray(corners, F32).reshape(2, 2, 2)
        field = vol.reshape(-1)
        expect = restate(field, counts, EXACT_MINS, EXACT_SPACINGS, LEVEL, pose, dirs, (1, 1), False, 1.0, 1.0, 2, labels=labels, K=24,
                         background=BG)
        got = call(device, field, counts, EXACT_MINS, EXACT_SPACINGS, LEVEL, pose, dirs, (1, 1), 1.0, 1.0, 2, labels=labels, k=24,
                   background=BG)
        same(got, expect, corners)
        want = 8 + (corner >> 2) * 4 + ((corner >> 1) & 1) * 2 + (corner & 1)
        assert got['range'][0, 0] == 1.5 and got['cell'][0, 0] == 8 and got['owner'][0, 0] == want == got['inst'][0, 0], (corners, got)
        if np.isnan(corners).any():
            assert got['cos'][0, 0] == 0.0


def check_slab(device):
    """A slab one cell thick (the points ix == 4 of a 9 x 5 x 5 grid): every ray that hits it has a slab point as owner, whichever
    side it comes from, while the hit cell's low corner is a slab point only from the far side; sem and inst equal the argmax and
    the labels gathered at owner in numpy."""
    counts = (9, 5, 5)
    n = 9 * 5 * 5
    rng = np.random.default_rng(16)
    vol = np.zeros(counts, F32)
    vol[4] = 1.0
    field = vol.reshape(-1)
    attrs = rng.uniform(-1, 1, size=(n, D)).astype(F32)
    labels = rng.integers(-2, 6, size=n).astype(I32)
    lo, hi = yc.hull(counts)
    centre, ext = 0.5 * (lo + hi), hi - lo
    dirs = pk.sweep.lidar_directions(8, 8, 12.0, -12.0, (-15.0, 15.0))
    near, step = march_of(counts, 64)
    for side in (-1.0, 1.0):
        Rm = np.diag([-side, -side, 1.0])                                                  # x forward = towards the slab
        pose = pose_of(centre + np.array([side * 0.9 * ext[0], 0.0, 0.0]), Rm)[None]
        got = call(device, field, counts, MINS, SPACINGS, LEVEL, pose, dirs, (8, 8), near, step / 4, 256, attrs=attrs, sem=(1, 5),
                   labels=labels, k=4, background=BG)
        expect = restate(field, counts, MINS, SPACINGS, LEVEL, pose, dirs, (8, 8), False, near, step / 4, 256, attrs, (), (1, 5), labels,
                         4, BG)
        same(got, expect, side)
        hit = got['cell'] >= 0
        assert hit.sum() > 20
        own = got['owner'][hit].astype(np.int64)
        assert (own // 25 == 4).all(), side                                                # a slab point
        assert ((got['cell'][hit] // 25 == 4).all()) == (side > 0)
        assert np.array_equal(got['sem'][hit], np.argmax(attrs[own, 1:6], axis=1).astype(I32))
        lab = labels[own]
        assert np.array_equal(got['inst'][hit], np.where((lab >= 0) & (lab < 4), lab, -1).astype(I32))
        assert (got['inst'][hit] >= 0).any() and (got['inst'][hit] < 0).any()


# ---------------------------------------------------------------------------------------------------------------- independent checks
# Worst absolute differences seen on the g++ twin (printed by the two checks below), and the tolerances taken from them: 4 x.
ANALYTIC_RANGE_WORST, ANALYTIC_RANGE_TOL = 5.46e-7, 2.184e-6
ANALYTIC_COS_WORST, ANALYTIC_COS_TOL = 4.16e-7, 1.664e-6
REPLAY_WORST, REPLAY_TOL = 4.77e-7, 1.908e-6


def linear_case():
    """A field linear in the world point, f = a . x + b, which the trilinear interpolant reproduces (up to rounding): the grid,
    the float32 field, (a, b), a sensor pose outside the level plane's air side, the world hull."""
    counts = (17, 9, 33)
    lo, hi = yc.hull(counts)
    axes = [np.array([F32(F32(i) + F32(0.5)) * F32(s) + F32(m) for i in range(c)], np.float64) for c, m, s in zip(counts, MINS, SPACINGS)]
    X, Y, Z = np.meshgrid(*axes, indexing='ij')
    a = np.array([0.31, -0.17, 0.23])
    centre = 0.5 * (lo + hi)
    b = float(LEVEL) - float(a @ centre)                        # the level plane passes through the centre of the hull
    field = (a[0] * X + a[1] * Y + a[2] * Z + b).astype(F32).reshape(-1)
    origin = centre - 0.35 * (hi - lo) * np.sign(a)             # on the air side, inside the hull
    rng = np.random.default_rng(17)
    return counts, field, a, b, pose_of(origin, rotation(rng))[None], centre


def check_analytic_plane(device):
    """(a) A linear field: range and cos of every return against the float64 plane intersection d* = (level - b - a . P0) /
    (a . dir) and |a . dir| / (|a| |dir|), with P0 and dir the float64 product of the float32 pose and directions.  On the g++ twin
    the worst differences are ANALYTIC_RANGE_WORST and ANALYTIC_COS_WORST; the tolerances are 4 x those, on the twin and on the
    device."""
    counts, field, a, b, pose, centre = linear_case()
    Rm, t = pose[0].reshape(3, 4)[:, :3].astype(np.float64), pose[0].reshape(3, 4)[:, 3].astype(np.float64)
    towards = Rm.T @ (centre - t)                               # the bundle looks at the centre of the hull
    az, el = np.degrees(np.arctan2(towards[1], towards[0])), np.degrees(np.arcsin(towards[2] / np.linalg.norm(towards)))
    dirs = pk.sweep.lidar_directions(9, 17, el + 10.0, el - 10.0, (az - 12.0, az + 12.0))
    got = call(device, field, counts, MINS, SPACINGS, LEVEL, pose, dirs, (9, 17), 0.0, 0.05, 200, background=BG)
    assert (got['cell'] >= 0).all()
    world = dirs.astype(np.float64) @ Rm.T
    d_star = (float(LEVEL) - b - a @ t) / (world @ a)
    cos_star = np.abs(world @ a) / (np.linalg.norm(a) * np.linalg.norm(world, axis=1))
    assert (d_star > 0.1).all()
    worst_range = float(np.abs(got['range'][0].astype(np.float64) - d_star).max())
    worst_cos = float(np.abs(got['cos'][0].astype(np.float64) - cos_star).max())
    print('analytic plane: %d rays, ranges %.3f .. %.3f, worst |range - d*| = %.3e, worst |cos - cos*| = %.3e'
          % (len(d_star), d_star.min(), d_star.max(), worst_range, worst_cos))
    assert worst_range <= ANALYTIC_RANGE_TOL and worst_cos <= ANALYTIC_COS_TOL, (worst_range, ANALYTIC_RANGE_TOL, worst_cos, ANALYTIC_COS_TOL)


def check_replay_of_plane_points(device):
    """(b) Points ON the level plane of the linear field, taken as the returns of a measured sweep: the bundle directions_to makes
    of them (in the sensor frame) is replayed, and residual(predicted, hit, measured) is ~0.  On the g++ twin the worst |residual|
    is REPLAY_WORST; the tolerance is 4 x that, on the twin and on the device."""
    counts, field, a, b, pose, centre = linear_case()
    Rm, t = pose[0].reshape(3, 4)[:, :3].astype(np.float64), pose[0].reshape(3, 4)[:, 3].astype(np.float64)
    rng = np.random.default_rng(18)
    lo, hi = yc.hull(counts)
    u, w = np.linalg.svd(a[None])[2][1:]                        # two directions in the plane
    world = centre + np.outer(rng.uniform(-0.25, 0.25, 200), u) * (hi - lo).min() + np.outer(rng.uniform(-0.25, 0.25, 200), w) * (hi - lo).min()
    assert np.abs(world @ a + b - float(LEVEL)).max() < 1e-12
    sensor = (world - t) @ Rm                                   # Rm^T (p - t)
    sensor = np.concatenate([sensor, np.zeros((1, 3))])         # a return AT the origin is dropped
    dirs, measured = pk.sweep.directions_to(sensor)
    assert dirs.shape == (200, 3) and measured.shape == (200,) and dirs.dtype == F32 and measured.dtype == F32
    got = call(device, field, counts, MINS, SPACINGS, LEVEL, pose, dirs, (1, 200), 0.0, 0.05, 200, background=BG)
    hit = got['cell'][0] >= 0
    assert hit.all()
    res = pk.sweep.residual(got['range'][0], hit, measured)
    worst = float(np.abs(res).max())
    print('replay: %d rays, measured ranges %.3f .. %.3f, worst |residual| = %.3e' % (len(res), measured.min(), measured.max(), worst))
    assert worst <= REPLAY_TOL, (worst, REPLAY_TOL)
    none = pk.sweep.residual(got['range'][0], np.zeros(200, bool), measured)
    assert np.isnan(none).all()
    as_torch = pk.sweep.residual(torch.from_numpy(got['range'][0]), torch.from_numpy(hit), measured)
    assert same_bits(as_torch.numpy(), res)


# ---------------------------------------------------------------------------------------------------------------- host helpers
def check_host_helpers():
    """lidar_directions, directions_to, poses and march_range by hand."""
    sw = pk.sweep
    d = sw.lidar_directions(3, 4, 10.0, -10.0)
    assert d.shape == (12, 3) and d.dtype == F32
    el, az = np.deg2rad([10.0, 0.0, -10.0]), np.deg2rad([-180.0, -90.0, 0.0, 90.0])
    want = np.array([[np.cos(e) * np.cos(z), np.cos(e) * np.sin(z), np.sin(e)] for e in el for z in az]).astype(F32)
    assert np.array_equal(d, want)                                                         # beam-major, the end point excluded
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-7
    assert sw.lidar_directions(0, 5, 1, -1).shape == (0, 3) and sw.lidar_directions(1, 1, 3.0, -3.0).shape == (1, 3)
    dirs, ranges = sw.directions_to(np.array([[3.0, 0, 4.0, 9.0], [0, 0, 0, 1.0], [0, -2.0, 0, 0]]))
    assert np.array_equal(dirs, np.array([[0.6, 0, 0.8], [0, -1, 0]], F32)) and np.array_equal(ranges, np.array([5, 2], F32))
    dirs, ranges = sw.directions_to(torch.tensor([[1.0, 1.0, 1.0]]), origin=(1.0, 1.0, 0.0))
    assert np.array_equal(dirs, np.array([[0, 0, 1]], F32)) and ranges[0] == 1
    m = np.arange(32, dtype=np.float64).reshape(2, 4, 4)
    p = sw.poses(m)
    assert p.shape == (2, 12) and p.dtype == F32 and np.array_equal(p[1], np.arange(16, 28))
    assert np.array_equal(sw.poses(m[:, :3]), p) and np.array_equal(sw.poses(m[0]), p[:1])
    with pytest.raises(ValueError, match='sensor_RT'):
        sw.poses(np.zeros((2, 3, 3)))
    counts, mins, spacings = (4, 4, 4), (0.0, 0.0, 0.0), (1.0, 1.0, 2.0)                  # hull 0.5 .. 3.5, 0.5 .. 3.5, 1 .. 7
    pose64 = np.concatenate([np.eye(3), np.array([[0.5], [0.5], [1.0]])], axis=1)[None]
    near, step, n_steps = sw.march_range(counts, mins, spacings, pose64)
    far = np.sqrt(9 + 9 + 36)
    assert (near, step) == (0.0, 0.5) and n_steps == int(np.ceil(far / 0.5)) + 1
    assert sw.march_range(counts, mins, spacings, pose64, min_range=1.0, max_range=3.0, step=0.25) == (1.0, 0.25, 9)
    assert sw.march_range(counts, mins, spacings, np.zeros((0, 3, 4)))[2] == 1
    for kw, text in ((dict(step=0.0), 'step'), (dict(min_range=-1.0), 'min_range'), (dict(step=1e-7), 'n_steps'),
                     (dict(max_range=float('nan')), 'far')):
        with pytest.raises(ValueError, match=text):
            sw.march_range(counts, mins, spacings, pose64, **kw)


def check_argument_errors(device):
    """ops.sweep_rays: rejected arguments raise AssertionError with the library's text (the table of both libraries' texts is
    tests/test_gpu_sweep_contract_texts.py); V = 0 and R = 0 are no-ops."""
    counts, n = (3, 2, 5), 30
    z = lambda *s: torch.zeros(*s, device=device)
    base = dict(values=z(n), counts=counts, mins=MINS, spacings=SPACINGS, level=0.5, pose=z(1, 12), dirs=z(8, 3), shape=(2, 4), near=0.1,
                step=0.1, n_steps=4)
    run = lambda **k: pk.ops.sweep_rays(**dict(base, **k))
    for kw, text in ((dict(counts=(30, 1, 1)), 'must be >= 2'), (dict(step=0.0), 'step = 0 must be finite and > 0'),
                     (dict(near=float('inf')), 'near = inf must be finite'), (dict(n_steps=0), 'n_steps = 0 must be in 1 .. 65536'),
                     (dict(attrs=z(n, 2), channels=[2]), 'column 2 must be in 0 .. d - 1 = 1'),
                     (dict(attrs=z(n, 2), channels=[0] * 33), 'C = 33 must be in 0 .. 32'),
                     (dict(attrs=z(n, 4), sem=(2, 3)), 'sem_first = 2, n_sem = 3'), (dict(labels=z(n).int(), k=-1), 'K = -1'),
                     (dict(shape=(-2, -4)), 'B = -2, A = -4 must be >= 0'), (dict(dirs=z(7, 3)), 'dirs must hold 8 rows'),
                     (dict(per_view=True, pose=z(2, 12)), 'dirs must hold 16 rows')):
        with pytest.raises(AssertionError, match=text):
            run(**kw)
    for kw in (dict(pose=z(0, 12)), dict(shape=(0, 4), dirs=z(0, 3)), dict(shape=(2, 0), dirs=z(0, 3))):
        got = run(**kw)
        assert got['range'].numel() == 0 and got['cell'].numel() == 0
    got = run(n_steps=65536, step=1e-6, dirs=z(8, 3) + 1.0)
    assert (got['cell'].cpu().numpy() == -1).all()
    got = run(want=('range', 'cell'))
    assert sorted(got) == ['cell', 'range']


# ---------------------------------------------------------------------------------------------------------------- option
def check_option():
    """FieldSweep's own checks, without a library."""
    S = pk.sweep.FieldSweep
    eye, d = np.eye(4)[None], pk.sweep.lidar_directions(2, 3, 5, -5)
    opt = S(eye, d)
    assert opt.shape == (1, 6) and opt.per_view is False and opt.of is None and opt.rows is None and opt.poses.shape == (1, 12)
    assert S(eye, d, shape=(2, 3)).shape == (2, 3) and S(np.tile(eye, (2, 1, 1)), np.tile(d, (2, 1)), per_view=True).shape == (1, 6)
    assert S(np.tile(eye, (2, 1, 1)), np.stack([d, d]), shape=(3, 2), per_view=True).dirs.shape == (12, 3)
    assert 'FieldSweep(V=1' in repr(opt) and S.keyword == 'sweep' and S.clip_list[0] == 'sweeps'
    for kw, text in ((dict(shape=(4, 2)), 'holds 8 rays, dirs hold 6'), (dict(shape=(-1, -6)), 'B, A >= 0'), (dict(shape=5), 'must be'),
                     (dict(level=float('nan')), 'NaN'), (dict(of='boxes'), "of = 'boxes'"), (dict(rows=(1, 2)), 'three colour columns')):
        with pytest.raises(ValueError, match=text):
            S(eye, d, **kw)
    with pytest.raises(ValueError, match='per_view needs dirs of V \\* R rows, got 6 rows for V = 4'):
        S(np.tile(eye, (4, 1, 1)), d, per_view=True)
    with pytest.raises(ValueError, match='need per_view=True'):
        S(np.tile(eye, (2, 1, 1)), np.stack([d, d]))
    with pytest.raises(ValueError, match='dirs must be'):
        S(eye, np.zeros((6, 2)))


def check_signatures():
    """sweep stands directly in front of layers in perform_inference, sweep and sweeps in evaluate_clip."""
    names = list(inspect.signature(pk.inference.perform_inference).parameters)
    assert names[-8] == 'sweep' and names[-7:] == ['layers', 'boxes', 'next_view', 'sight', 'segments', 'tracker', 'clearance']
    names = list(inspect.signature(pk.evaluation.evaluate_clip).parameters)
    assert names[-13:-10] == ['sweep', 'sweeps', 'layers']
    for fn in (pk.inference.perform_inference, pk.evaluation.evaluate_clip):
        assert inspect.signature(fn).parameters['sweep'].default is None and 'sweep' in fn.__doc__ and 'FieldSweep' in fn.__doc__
    assert inspect.signature(pk.evaluation.evaluate_clip).parameters['sweeps'].default is None
    assert 'FieldSweep' in pk.products.__doc__


# ---------------------------------------------------------------------------------------------------------------- end to end
COUNTS = rc.COUNTS
SHAPE = (6, 20)
COLOUR = (1, 2, 3)


def fixture_option(shared, **kw):
    """Two sensors round the fixture's query grid, one inside it and one outside, with one lidar table of 6 x 20 rays."""
    mins, spacings = yc.frame_of(shared)
    lo, hi = yc.hull(COUNTS, mins, spacings)
    centre, ext = 0.5 * (lo + hi), hi - lo
    rng = np.random.default_rng(19)
    poses = np.stack([pose_of(centre + 0.1 * ext, rotation(rng)), pose_of(centre + np.array([-0.8, -0.5, 0.4]) * np.linalg.norm(ext))])
    dirs = pk.sweep.lidar_directions(*SHAPE, 35.0, -35.0)
    kw.setdefault('shape', SHAPE)
    return pk.sweep.FieldSweep(poses.reshape(2, 3, 4), dirs, **kw)


def without(result):
    return {k: v for k, v in result.items() if k not in ('components', 'segments', 'sweep')}


def check_product(shared, got, option, level=0.5, of=None):
    """result['sweep'] EQUAL to sweep.cast on the call's own implicit_output (with the labels of the `of` product), and to the
    restatement; rows and n_rows equal to the numpy selection of the dense arrays in ray order."""
    device = shared.device
    mins, spacings = yc.frame_of(shared)
    sweep, output = got['sweep'], got['implicit_output']
    keys = ['range', 'point', 'cell', 'owner', 'cos'] + (['inst'] if of else []) + ['features'] + (['rows', 'n_rows'] if option.rows else []) + ['march']
    assert list(sweep) == keys and all(isinstance(a, np.ndarray) for a in sweep.values()), list(sweep)
    labels, K = (got[of]['labels'], len(got[of]['table'])) if of else (None, 0)
    alone = pk.sweep.cast(torch.from_numpy(output).to(device), COUNTS, mins, spacings, option.pose64, option.dirs, level,
                          shape=option.shape, per_view=option.per_view, channels=option.channels, select=option.select,
                          min_range=option.min_range, max_range=option.max_range, step=option.step, labels=labels, k=K, rows=option.rows)
    assert list(alone) == keys
    for name in keys:
        a, b = sweep[name], alone[name].cpu().numpy()
        if name == 'rows':                                       # (the rows behind n_rows are uninitialised)
            a, b = a[:int(sweep['n_rows'][0])], b[:int(sweep['n_rows'][0])]
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), name
    near, step, n_steps = pk.sweep.march_range(COUNTS, mins, spacings, option.pose64, option.min_range, option.max_range, option.step)
    assert same_bits(sweep['march'], np.array([near, step], F32))
    field = output[:, 0]
    if option.select is not None:
        field = np.where(output[:, option.select[0]] >= F32(option.select[1]), field, F32(0))
    expect = restate(field, COUNTS, mins, spacings, level, option.poses, option.dirs, option.shape, option.per_view, near, step, n_steps,
                     output, option.channels, None, labels, K, pk.sweep.NO_RETURN)
    same(sweep, expect, names=keys[:keys.index('features') + 1])
    hit = expect['hit']
    assert hit.any() and not hit.all()
    assert np.array_equal(hit, sweep['range'] >= 0) and np.array_equal(hit, sweep['cell'] >= 0)
    if of:
        own = sweep['owner'][hit].astype(np.int64)
        lab = labels[own]
        assert np.array_equal(sweep['inst'][hit], np.where((lab >= 0) & (lab < K), lab, -1)) and (sweep['inst'][hit] >= 0).any()
    if option.rows:
        V, R = hit.shape
        n = int(sweep['n_rows'][0])
        assert sweep['rows'].shape == (V * R, 10) and sweep['rows'].dtype == F32 and sweep['n_rows'].dtype == I32 and n == hit.sum()
        flat = hit.reshape(-1)
        own = sweep['owner'].reshape(-1)[flat].astype(np.int64)
        inst = sweep['inst'].reshape(-1)[flat].astype(F32) if of else np.full(n, -1, F32)
        dense = np.concatenate([sweep['point'].reshape(-1, 3)[flat], sweep['cos'].reshape(-1, 1)[flat], inst[:, None], np.full((n, 1), -1, F32),
                                output[own][:, list(option.rows)], np.repeat(np.arange(V), R)[flat].astype(F32)[:, None]], axis=1)
        assert same_bits(sweep['rows'][:n], dense.astype(F32))
        rows, views = pk.sweep.rows_of(got)
        assert same_bits(rows, dense[:, :9].astype(F32)) and views.dtype == I32 and np.array_equal(views, dense[:, 9].astype(I32))
        again = pk.sweep.rows_of(sweep)
        assert same_bits(again[0], rows) and np.array_equal(again[1], views)
    return expect


def check_end_to_end(shared, monkeypatch):
    device = shared.device
    option = fixture_option(shared, channels=(0, 4))
    calls = rc.count_waits(monkeypatch)
    res = rc.infer(device, shared.inputs, sweep=option)
    assert calls['wait'] == 1                                    # exactly one host wait
    monkeypatch.undo()
    check_product(shared, res, option)
    same_result(without(res), shared.dense)
    # another level and step, a select column, a range limit
    track = pk.inference.get_track_idx(shared.inputs[3]['color_mode'])
    option = fixture_option(shared, level=0.47, step=0.05, select=(track, 0.1), max_range=30.0, min_range=0.2)
    res = rc.infer(device, shared.inputs, sweep=option)
    check_product(shared, res, option, level=0.47)
    same_result(without(res), shared.dense)
    # of='components' with rows: inst from that call's labels, the rows feed the lidar front end
    comp = pk.components.Components()
    option = fixture_option(shared, of='components', rows=COLOUR)
    calls = rc.count_waits(monkeypatch)
    res = rc.infer(device, shared.inputs, components=comp, sweep=option)
    assert calls['wait'] == 1
    monkeypatch.undo()
    check_product(shared, res, option, of='components')
    alone = rc.infer(device, shared.inputs, components=comp)
    assert sorted(list(alone) + ['sweep']) == sorted(res) and list(alone['components']) == list(res['components'])
    for k in alone['components']:
        assert np.array_equal(alone['components'][k], res['components'][k])
    same_result(without(res), shared.dense)
    rows, views = pk.sweep.rows_of(res)
    assert rows.shape[1] == 9 and len(rows) == len(views) > 0
    fed, key = pk.frontend.lidar_rows(torch.from_numpy(rows).to(device), cube_mode=4, min_z=-100.0, other_bounds=100.0)
    assert tuple(fed.shape) == rows.shape and same_bits(fed.cpu().numpy()[:, 3:], rows[:, 3:]) and tuple(key.shape) == (len(rows),)
    # of='segments' beside components; rows without a label product: inst -1
    option = fixture_option(shared, of='segments')
    res = rc.infer(device, shared.inputs, components=comp, segments=pk.watershed.Segments(h=1), sweep=option)
    check_product(shared, res, option, of='segments')
    option = fixture_option(shared, rows=COLOUR)
    res = rc.infer(device, shared.inputs, sweep=option)
    check_product(shared, res, option)
    with pytest.raises(ValueError, match='rows='):
        pk.sweep.rows_of(dict(sweep=dict(range=np.zeros((1, 1), F32))))
    # under refine and in track_mode 'all': the expanded / merged array is what is scanned
    option = fixture_option(shared, of='components', channels=(0,))
    plain = rc.infer(device, shared.inputs, refine=pk.inference.GridRefine(2, 0.46, 1))
    res = rc.infer(device, shared.inputs, refine=pk.inference.GridRefine(2, 0.46, 1), components=comp, sweep=option)
    check_product(shared, res, option, of='components')
    same_result({k: v for k, v in without(res).items() if k != 'refine'}, {k: v for k, v in plain.items() if k != 'refine'})
    res = rc.infer(device, shared.inputs, track_mode='all', components=comp, sweep=option)
    check_product(shared, res, option, of='components')
    same_result(without(res), shared.dense_all)


def check_segmentation(device):
    """The small CARLA case, which predicts segmentation: result['sweep'] holds `sem`, made from the LAST 13 columns of the call's
    own output -- the numpy argmax (the first maximum as well) gathered at `owner`, -1 without a return --, EQUAL to the restatement
    with sem = (G - 13, 13), and the rows carry it in their sem column and the components' labels in their inst column."""
    import golden_cases as gc
    case = [c for c in gc.INFER_CASES if gc.infer_inputs(c)[3]['predict_segmentation']][0]
    pcl, pa, ia, inf, esd, dsd = gc.infer_inputs(case)
    enc = pk.model.PointCompletionNetV3(**pa).to(device).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).to(device).eval()
    dec.load_state_dict(dsd)
    counts, mins, spacings = pk.geometry.grid_frame(case['num_sample'], inf['min_z'], inf['cube_bounds'], inf['data_kind'], 4)
    counts = tuple(int(c) for c in counts)
    lo, hi = yc.hull(counts, mins, spacings)
    centre, ext = 0.5 * (lo + hi), hi - lo
    outside = centre + np.array([-0.8, -0.5, 0.4]) * np.linalg.norm(ext)
    poses = np.stack([pose_of(centre + 0.1 * ext, rotation(np.random.default_rng(23))), pose_of(outside, facing(outside, centre))])
    option = pk.sweep.FieldSweep(poses.reshape(2, 3, 4), pk.sweep.lidar_directions(*SHAPE, 35.0, -35.0), shape=SHAPE, level=0.45,
                                 channels=(0, 2), of='components', rows=COLOUR)
    got = pk.inference.perform_inference(
        pcl.clone(), None, None, [enc, dec], device, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], case['time_idx'], None,
        sample_implicit=True, num_sample=case['num_sample'], point_sample_mode='grid', batch_size=case['batch_size'],
        predict_segmentation=True, track_mode='none', semantic_classes=13, density_threshold=0.5, data_kind=inf['data_kind'],
        cube_mode=4, compress_air=True, components=pk.components.Components(connectivity=26, level=0.45), sweep=option)
    out, sweep = got['implicit_output'], got['sweep']
    G = out.shape[1]
    assert G > 13 and list(sweep) == ['range', 'point', 'cell', 'owner', 'cos', 'sem', 'inst', 'features', 'rows', 'n_rows', 'march']
    hit = sweep['cell'] >= 0
    assert hit.any() and not hit.all()
    own = sweep['owner'][hit].astype(np.int64)
    classes = np.argmax(out[own, G - 13:], axis=1).astype(I32)
    assert sweep['sem'].dtype == I32 and np.array_equal(sweep['sem'][hit], classes) and (sweep['sem'][~hit] == -1).all()
    assert len(np.unique(classes)) >= 2                              # (the case's condition: the classes are not all one)
    labels, K = got['components']['labels'], len(got['components']['table'])
    near, step, n_steps = pk.sweep.march_range(counts, mins, spacings, option.pose64)
    expect = restate(out[:, 0], counts, mins, spacings, 0.45, option.poses, option.dirs, SHAPE, False, near, step, n_steps, out, (0, 2),
                     (G - 13, 13), labels, K, pk.sweep.NO_RETURN)
    same(sweep, expect, names=['range', 'point', 'cell', 'owner', 'cos', 'sem', 'inst', 'features'])
    rows, views = pk.sweep.rows_of(got)
    assert len(rows) == int(hit.sum()) == int(sweep['n_rows'][0])
    assert np.array_equal(rows[:, 5], classes.astype(F32)) and np.array_equal(rows[:, 4], sweep['inst'][hit].astype(F32))
    assert same_bits(rows[:, 6:9], out[own][:, list(COLOUR)]) and np.array_equal(views, np.repeat(np.arange(2), hit.shape[1])[hit.reshape(-1)])


def check_clip(shared):
    """evaluate_clip(sweep=..., sweeps=[]): one dict per output frame, that of the perform_inference call; the tuples as without."""
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = rc.clip_inputs(shared)
    run = lambda **kw: pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True, **kw)
    option, sweeps, objects = fixture_option(shared, of='components', rows=COLOUR), [], []
    clip = run(components=pk.components.Components(), objects=objects, sweep=option, sweeps=sweeps)
    dense = run()
    assert len(clip) == len(dense) == len(sweeps) == len(objects) == 2
    for t in range(2):
        for got, want in zip(clip[t], dense[t]):
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        res = pk.inference.perform_inference(
            pcl.clone(), None, frames[t], [enc, dec], shared.device, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], t, None,
            sample_implicit=True, num_sample=rc.CASE['num_sample'], point_sample_mode='grid', batch_size=rc.CASE['batch_size'],
            predict_segmentation=False, track_mode='none', semantic_classes=13, density_threshold=0.5, data_kind='greater',
            cube_mode=4, compress_air=True, point_occupancy_radius=0.8, components=pk.components.Components(), sweep=option)
        assert list(sweeps[t]) == list(res['sweep'])
        n = int(sweeps[t]['n_rows'][0])
        for name, a in sweeps[t].items():
            b = res['sweep'][name]
            assert np.array_equal(a[:n] if name == 'rows' else a, b[:n] if name == 'rows' else b, equal_nan=True), name
        assert (sweeps[t]['cell'] >= 0).any()
    with pytest.raises(ValueError, match='sweeps'):
        run(components=pk.components.Components(), objects=[], sweep=option)
    with pytest.raises(ValueError, match='sweep needs components='):
        run(sweep=option, sweeps=[])


def check_none_is_untouched(shared, monkeypatch):
    """sweep=None: no new key, one host wait, and neither the op nor the entry point is reached."""
    def forbidden(*a, **k):
        raise AssertionError('sweep=None must not reach the sweep entry point')
    monkeypatch.setattr(pk.ops, 'sweep_rays', forbidden)
    L = pk._lib.lib()
    for name in SYMBOLS:
        monkeypatch.setattr(L, name, forbidden)
    calls = rc.count_waits(monkeypatch)
    res = rc.infer(shared.device, shared.inputs, sweep=None)
    assert calls == dict(wait=1)
    assert sorted(res) == sorted(shared.dense)
    same_result(res, shared.dense)
    res = rc.infer(shared.device, shared.inputs, components=pk.components.Components())
    assert list(res['components']) == ['labels', 'table'] and 'sweep' not in res


def check_value_errors(shared):
    comp, option = pk.components.Components(), fixture_option(shared)
    with pytest.raises(ValueError, match='sweep must be a sweep.FieldSweep or None'):
        rc.infer(shared.device, shared.inputs, sweep=comp)
    with pytest.raises(ValueError, match='sweep needs components=<a components.Components>'):
        rc.infer(shared.device, shared.inputs, sweep=fixture_option(shared, of='components'))
    with pytest.raises(ValueError, match='sweep needs segments=<a watershed.Segments>'):
        rc.infer(shared.device, shared.inputs, components=comp, sweep=fixture_option(shared, of='segments'))
    with pytest.raises(ValueError, match="needs point_sample_mode 'grid'"):
        rc.infer(shared.device, shared.inputs, sweep=option, point_sample_mode='random')
    with pytest.raises(ValueError, match='n_steps'):
        rc.infer(shared.device, shared.inputs, sweep=fixture_option(shared, step=1e-7))
    with pytest.raises(ValueError, match='NaN'):
        fixture_option(shared, level=float('nan'))
    with pytest.raises(ValueError, match='holds 100 rays'):
        fixture_option(shared, shape=(5, 20))
    with pytest.raises(ValueError, match='B, A >= 0'):
        fixture_option(shared, shape=(-6, -20))
    with pytest.raises(ValueError, match='per_view needs dirs of V'):
        pk.sweep.FieldSweep(np.tile(np.eye(4), (7, 1, 1)), pk.sweep.lidar_directions(*SHAPE, 35.0, -35.0), per_view=True)
    mins, spacings = yc.frame_of(shared)
    with pytest.raises(ValueError, match='NaN'):
        pk.sweep.cast(torch.zeros((rc.N_QUERIES, 5), device=shared.device), COUNTS, mins, spacings, option.pose64, option.dirs, float('nan'))
