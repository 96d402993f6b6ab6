"""Shared by tests/test_surface_host.py (through the g++ twin) and tests/test_gpu_surface.py (on the device): the numpy float32
restatement of the surface-nets rules (include/occ4d_surface.h) in the stated operation order, the case matrix of the two entry
points, the guard of the data-dependent positions, the property checks that do not use the restatement, and the end-to-end
comparisons of perform_inference(surface=...) on the tracking fixture.
Everything but the properties is compared EQUAL: the non-NaN elements bit for bit, the NaN positions as positions."""

import numpy as np
import pytest
import torch

import refine_cases as rc
import occlusions4d_amd as pk
from track_cases import same_bits, same_result

F32 = np.float32
GRIDS = [(1, 1, 1), (2, 2, 2), (3, 3, 3), (2, 5, 1), (3, 5, 7), (9, 7, 5), (17, 9, 33)]
LARGE_GRID = (65, 65, 65)             # 274 625 points = 1073 tiles of 256 points: a second trip of the prefix
WIDTHS = [0, 1, 5, 32]
PAD = 3                               # a strided array has ld = width + PAD
SENTINEL = 777.0
LEVEL = F32(0.46)
POOL = np.array([LEVEL, np.nextafter(LEVEL, F32(-1)), np.nextafter(LEVEL, F32(2)), 0.0, -0.0, np.nan, np.inf, -np.inf, 100.0, -100.0],
                dtype=F32)
MINS, SPACINGS = (-1.25, 0.5, 3.0), (0.3, 0.7, 0.11)
TILE = 256


# ---------------------------------------------------------------------------------------------------------------- restatement
def corner_view(a, counts, o):
    """The values at corner offset o = (ox, oy, oz) of every cell: (nx - 1, ny - 1, nz - 1, ...)."""
    return a[o[0]:o[0] + counts[0] - 1, o[1]:o[1] + counts[1] - 1, o[2]:o[2] + counts[2] - 1]


def edges():
    """The 12 edges of a cell in the header's order: (axis a, b, c, j, k, lower corner offset, upper corner offset)."""
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for j in (0, 1):
            for k in (0, 1):
                lo = [0, 0, 0]
                lo[b], lo[c] = j, k
                hi = list(lo)
                hi[a] = 1
                yield a, b, c, j, k, tuple(lo), tuple(hi)


def restate_cells(density, counts, level, mins, spacings, attrs=None):
    """-> (crossed (n,) bool per grid point = per cell by its low corner, rows (n, 3 + A) float32: the vertex row of every
    crossed cell, NaN-free garbage elsewhere)."""
    counts = tuple(int(c) for c in counts)
    n = counts[0] * counts[1] * counts[2]
    n_attr = 0 if attrs is None else attrs.shape[1]
    crossed = np.zeros(counts, bool)
    rows = np.zeros(counts + (3 + n_attr,), F32)
    if min(counts) < 2:
        return crossed.reshape(n), rows.reshape(n, 3 + n_attr)
    level = F32(level)
    f = np.asarray(density, F32).reshape(counts)
    with np.errstate(invalid='ignore'):
        ins = f >= level
    cells = tuple(c - 1 for c in counts)
    corners = [corner_view(ins, counts, (o >> 2 & 1, o >> 1 & 1, o & 1)) for o in range(8)]
    cell_crossed = np.logical_or.reduce(corners) & ~np.logical_and.reduce(corners)
    s = np.zeros((3,) + cells, F32)
    k_count = np.zeros(cells, np.int32)
    acc = np.zeros(cells + (n_attr,), F32)
    A = None if attrs is None else np.asarray(attrs, F32).reshape(counts + (n_attr,))
    for a, b, c, j, k, lo, hi in edges():
        fl, fu = corner_view(f, counts, lo), corner_view(f, counts, hi)
        differ = corner_view(ins, counts, lo) != corner_view(ins, counts, hi)
        with np.errstate(all='ignore'):
            t = (level - fl) / (fu - fl)
            t = np.where((t >= F32(0)) & (t <= F32(1)), t, F32(0.5)).astype(F32)
            s[a] = np.where(differ, s[a] + t, s[a])
            s[b] = np.where(differ, s[b] + F32(j), s[b])
            s[c] = np.where(differ, s[c] + F32(k), s[c])
            if n_attr:
                al, au = corner_view(A, counts, lo), corner_view(A, counts, hi)
                term = al + t[..., None] * (au - al)
                acc = np.where(differ[..., None], acc + term, acc)
        k_count += differ
    with np.errstate(all='ignore'):
        kf = k_count.astype(F32)
        for a in range(3):
            shape = [1, 1, 1]
            shape[a] = cells[a]
            index = np.arange(cells[a], dtype=F32).reshape(shape)
            u = s[a] / kf
            rows[:cells[0], :cells[1], :cells[2], a] = ((index + F32(0.5)) + u) * F32(spacings[a]) + F32(mins[a])
        if n_attr:
            rows[:cells[0], :cells[1], :cells[2], 3:] = acc / kf[..., None]
    assert rows.dtype == F32 and s.dtype == F32 and acc.dtype == F32
    crossed[:cells[0], :cells[1], :cells[2]] = cell_crossed
    return crossed.reshape(n), rows.reshape(n, 3 + n_attr)


def restate_quads(density, counts, level):
    """-> (emit (n, 3) bool: point p's edge on axis a emits a quad; inside (n,) bool)."""
    counts = tuple(int(c) for c in counts)
    n = counts[0] * counts[1] * counts[2]
    f = np.asarray(density, F32).reshape(counts)
    with np.errstate(invalid='ignore'):
        ins = f >= F32(level)
    emit = np.zeros(counts + (3,), bool)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        if counts[a] < 2 or counts[b] < 3 or counts[c] < 3:
            continue
        sl_p, sl_q = [None] * 3, [None] * 3
        sl_p[a], sl_q[a] = slice(0, counts[a] - 1), slice(1, counts[a])
        sl_p[b] = sl_q[b] = slice(1, counts[b] - 1)
        sl_p[c] = sl_q[c] = slice(1, counts[c] - 1)
        emit[tuple(sl_p) + (a,)] = ins[tuple(sl_p)] != ins[tuple(sl_q)]
    return emit.reshape(n, 3), ins.reshape(n)


def tile_numbers(flags, per_item, offsets):
    """The number of every item's first output: offsets[tile] + the outputs of the items in front of it in its tile (int64)."""
    n = flags.shape[0]
    per_item = per_item.astype(np.int64)
    before = np.cumsum(per_item) - per_item
    tile = np.arange(n) // TILE
    first = before[np.minimum(tile * TILE, max(n - 1, 0))] if n else before
    return np.asarray(offsets, np.int64)[tile] + (before - first)


def true_offsets(per_item):
    per_item = per_item.astype(np.int64)
    tiles = -(-per_item.shape[0] // TILE)
    sums = np.add.reduceat(per_item, np.arange(tiles) * TILE) if tiles else np.zeros(0, np.int64)
    return (np.cumsum(sums) - sums).astype(np.int32)


def restate(density, counts, level, mins, spacings, attrs=None, cell_offsets=None, face_offsets=None, vertex_cap=None,
            face_cap=None, ld_v=None):
    """The two entry points: -> dict(cell_offsets, face_offsets, totals (2,), work (n,) int32, vertices (vertex_cap, ld_v) with
    SENTINEL where nothing is written, faces (face_cap, 4) int32 with -7 where nothing is written).  With the offsets and
    capacities left out: the true ones, so vertices / faces are the mesh."""
    counts = tuple(int(c) for c in counts)
    n = counts[0] * counts[1] * counts[2]
    crossed, rows = restate_cells(density, counts, level, mins, spacings, attrs)
    emit, ins = restate_quads(density, counts, level)
    n_quads = emit.sum(axis=1)
    true_cells, true_faces = true_offsets(crossed), true_offsets(n_quads)
    totals = np.array([crossed.sum(), n_quads.sum()], np.int32)
    cell_offsets = true_cells if cell_offsets is None else cell_offsets
    face_offsets = true_faces if face_offsets is None else face_offsets
    vertex_cap = int(totals[0]) if vertex_cap is None else vertex_cap
    face_cap = int(totals[1]) if face_cap is None else face_cap
    width = rows.shape[1]
    ld_v = width if ld_v is None else ld_v
    number = tile_numbers(crossed, crossed, cell_offsets)
    work = np.where(crossed, number, -1).astype(np.int64).astype(np.int32)             # (wraps like the C conversion)
    vertices = np.full((vertex_cap, ld_v), SENTINEL, F32)
    ok = crossed & (number >= 0) & (number < vertex_cap)
    unique = np.unique(number[ok]).shape[0] == int(ok.sum())           # (offsets that send two items to one position: no owner)
    vertices[number[ok], :width] = rows[ok]
    # the quad of (p, a): work at p - e_b - e_c, p - e_c, p, p - e_b; reversed when p is outside
    grid_work = work.reshape(counts)
    quads = np.zeros((n, 3, 4), np.int32)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        wb, wc = np.roll(grid_work, 1, axis=b), np.roll(grid_work, 1, axis=c)
        wbc = np.roll(wb, 1, axis=c)
        quad = np.stack([wbc, wc, grid_work, wb], axis=-1).reshape(n, 4)
        quads[:, a] = np.where(ins[:, None], quad, quad[:, ::-1])
    first = tile_numbers(n_quads > 0, n_quads, face_offsets)
    local = np.cumsum(emit, axis=1) - emit
    face_number = first[:, None] + local
    faces = np.full((face_cap, 4), -7, np.int32)
    ok = emit & (face_number >= 0) & (face_number < face_cap)
    unique = unique and np.unique(face_number[ok]).shape[0] == int(ok.sum())
    faces[face_number[ok]] = quads[ok]
    return dict(unique=unique, cell_offsets=true_cells, face_offsets=true_faces, totals=totals, work=work, vertices=vertices, faces=faces,
                crossed=crossed)


def same_mesh(got_v, got_f, want):
    return (same_bits(np.ascontiguousarray(got_v), want['vertices']) and got_f.dtype == np.int32
            and np.array_equal(got_f, want['faces']))


# ---------------------------------------------------------------------------------------------------------------- entry points
def densities(scenario, n, rng):
    if scenario == 'pool':
        d = POOL[rng.integers(0, len(POOL), size=n)]
        mix = rng.uniform(size=n) < 0.5
        d[mix] = rng.uniform(-1.0, 1.0, size=int(mix.sum())).astype(F32)
        return d
    if scenario == 'all_inside':
        return np.full(n, 0.9, F32)
    if scenario == 'all_outside':
        return np.full(n, -2.0, F32)
    raise ValueError(scenario)


def attributes(n, n_attr, rng):
    a = rng.uniform(-2.0, 2.0, size=(n, n_attr)).astype(F32)
    if n_attr:
        special = rng.uniform(size=(n, n_attr)) < 0.05
        a[special] = np.array([np.nan, np.inf, -np.inf, 0.0], F32)[rng.integers(0, 4, size=int(special.sum()))]
    return a


def padded(device, values, strided, dtype=torch.float32):
    """(buffer (rows, width + PAD) with the sentinel in the padding, or the dense array; its (rows, width) view)."""
    values = np.asarray(values)
    rows, width = values.shape
    buf = torch.full((rows, width + PAD if strided else width), SENTINEL, dtype=dtype)
    buf[:, :width] = torch.from_numpy(values)
    buf = buf.to(device)
    return buf, buf[:, :width]


def raw_call(device, density_col, ld, attrs, ld_attr, n_attr, counts, level, cell_offsets=None, face_offsets=None, vertex_cap=None,
             face_cap=None, ld_v=None, guard=2):
    """The two entry points as they are, with every stride and capacity the caller's.  -> dict like restate()'s, where vertices /
    faces are (guard + cap + guard) rows: the rows around the capacity must keep their fill."""
    L, p = pk._lib.lib(), pk.ops._ptr
    n = counts[0] * counts[1] * counts[2]
    tiles = -(-n // TILE)
    co = torch.full((tiles,), -9, dtype=torch.int32, device=device)
    fo = torch.full((tiles,), -9, dtype=torch.int32, device=device)
    totals = torch.full((2,), -9, dtype=torch.int32, device=device)
    rc_ = L.occ4d_surface_count_f32(p(density_col), ld, *counts, float(level), p(co), p(fo), p(totals), pk.ops._stream())
    assert rc_ == pk._lib.OK, L.occ4d_last_error()
    true = dict(cell_offsets=co.cpu().numpy(), face_offsets=fo.cpu().numpy(), totals=totals.cpu().numpy())
    if cell_offsets is not None:
        co = torch.from_numpy(np.asarray(cell_offsets, np.int32)).to(device)
    if face_offsets is not None:
        fo = torch.from_numpy(np.asarray(face_offsets, np.int32)).to(device)
    vertex_cap = int(true['totals'][0]) if vertex_cap is None else vertex_cap
    face_cap = int(true['totals'][1]) if face_cap is None else face_cap
    ld_v = 3 + n_attr if ld_v is None else ld_v
    vertices = torch.full((vertex_cap + 2 * guard, ld_v), SENTINEL, dtype=torch.float32, device=device)
    faces = torch.full((face_cap + 2 * guard, 4), -7, dtype=torch.int32, device=device)
    work = torch.full((n + 2 * guard,), -7, dtype=torch.int32, device=device)
    rc_ = L.occ4d_surface_write_f32(p(density_col), ld, p(attrs), ld_attr, n_attr, *counts, float(level), MINS[0], SPACINGS[0], MINS[1],
                                    SPACINGS[1], MINS[2], SPACINGS[2], p(co), p(fo), p(work[guard:]), p(vertices[guard:]), ld_v,
                                    vertex_cap, p(faces[guard:]), face_cap, pk.ops._stream())
    assert rc_ == pk._lib.OK, L.occ4d_last_error()
    return dict(true, work=work.cpu().numpy(), vertices=vertices.cpu().numpy(), faces=faces.cpu().numpy(), guard=guard)


def check_raw(got, want, tag, owned=True):
    """A raw call's arrays against the restatement's, the guard rows around them untouched.  owned=False: the offsets send
    several items to one position, so what lies inside the capacity has no single owner and is not compared."""
    g = got['guard']
    for k in ('cell_offsets', 'face_offsets', 'totals'):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (tag, k)
    assert np.array_equal(got['work'][g:-g], want['work']), tag
    assert want['unique'] == owned, tag
    if owned:
        assert same_bits(got['vertices'][g:-g], want['vertices']), tag
        assert np.array_equal(got['faces'][g:-g], want['faces']), tag
    for k, fill in (('work', -7), ('vertices', SENTINEL), ('faces', -7)):
        assert (got[k][:g] == fill).all() and (got[k][-g:] == fill).all(), (tag, k)


def check_cell(device, counts, n_attr, strided, scenario, rng):
    """One cell of the matrix: the raw entry points with padded strides when `strided`, ops.surface_nets otherwise."""
    tag = (counts, n_attr, strided, scenario)
    n = counts[0] * counts[1] * counts[2]
    dens = densities(scenario, n, rng)
    attrs = attributes(n, n_attr, rng)
    want = restate(dens, counts, LEVEL, MINS, SPACINGS, attrs if n_attr else None)
    if scenario != 'pool':
        assert want['totals'].tolist() == [0, 0], tag
    dens_buf, dens_view = padded(device, dens[:, None], strided)
    attr_buf, attr_view = padded(device, attrs, strided) if n_attr else (None, None)
    if strided:
        width = 3 + n_attr
        want = restate(dens, counts, LEVEL, MINS, SPACINGS, attrs if n_attr else None, ld_v=width + PAD)
        got = raw_call(device, dens_view, dens_buf.stride(0), attr_view, attr_buf.stride(0) if n_attr else 0, n_attr, counts, LEVEL,
                       ld_v=width + PAD)
        check_raw(got, want, tag)
        assert (dens_buf.cpu().numpy()[:, 1:] == SENTINEL).all(), tag
        assert attr_buf is None or (attr_buf.cpu().numpy()[:, n_attr:] == SENTINEL).all(), tag
    else:
        v, f = pk.ops.surface_nets(dens_view[:, 0], counts, float(LEVEL), MINS, SPACINGS, attrs=attr_view)
        assert v.shape == (int(want['totals'][0]), 3 + n_attr) and f.shape == (int(want['totals'][1]), 4) and f.dtype == torch.int32, tag
        assert same_mesh(v.cpu().numpy(), f.cpu().numpy(), want), tag
        bv, bf, totals = pk.ops.surface_nets(dens_view[:, 0], counts, float(LEVEL), MINS, SPACINGS, attrs=attr_view, sync=False)
        nv, nf = totals.cpu().numpy().tolist()
        assert [nv, nf] == want['totals'].tolist() and (bv.shape[0], bf.shape[0]) == pk.ops.surface_capacity(counts), tag
        assert nv <= bv.shape[0] and nf <= bf.shape[0] and same_mesh(bv[:nv].cpu().numpy(), bf[:nf].cpu().numpy(), want), tag
    return want


def cells_of():
    return len(WIDTHS) * 2 + 2


def check_matrix(counts, device):
    rng = np.random.default_rng(9000 + counts[0] * 10000 + counts[1] * 100 + counts[2])
    cells = 0
    some = 0
    for n_attr in WIDTHS:
        for strided in (False, True):
            some += int(check_cell(device, counts, n_attr, strided, 'pool', rng)['totals'][0])
            cells += 1
    if min(counts) >= 3:
        assert some > 0, counts                       # (the pool does cross these grids)
    if min(counts) < 2:
        assert some == 0, counts                      # an axis of 1: no cells
    check_cell(device, counts, 5, True, 'all_inside', rng)
    check_cell(device, counts, 1, False, 'all_outside', rng)
    return cells + 2


def check_large(device):
    rng = np.random.default_rng(65)
    want = check_cell(device, LARGE_GRID, 5, True, 'pool', rng)
    assert -(-LARGE_GRID[0] ** 3 // TILE) > 1024 and want['totals'][0] > 10 ** 5


def check_one_inside_point(device):
    dens = np.zeros((3, 3, 3), F32)
    dens[1, 1, 1] = 1.0
    v, f = pk.ops.surface_nets(torch.from_numpy(dens.reshape(-1)).to(device), (3, 3, 3), 0.5, MINS, SPACINGS)
    assert v.shape == (8, 3) and f.shape == (6, 4)
    assert same_mesh(v.cpu().numpy(), f.cpu().numpy(), restate(dens.reshape(-1), (3, 3, 3), 0.5, MINS, SPACINGS))
    assert sorted(f.cpu().numpy().reshape(-1).tolist()) == sorted(list(range(8)) * 3)
    properties(v.cpu().numpy(), f.cpu().numpy(), positive=True)


def check_guard(device):
    """Capacities below the totals and offset arrays filled with garbage: OK is returned, what lies inside the capacity is the
    restatement's (a number outside is dropped; where the offsets send two items to one position, that position has no owner
    and is not compared), and nothing behind the capacity changes.  Nothing is provoked: the arrays are
    windows of larger tensors whose other rows carry a fill of their own."""
    counts, n_attr = (9, 7, 5), 5
    n = 9 * 7 * 5
    rng = np.random.default_rng(5)
    dens, attrs = densities('pool', n, rng), attributes(n, n_attr, rng)
    dens_t, attrs_t = torch.from_numpy(dens).to(device), torch.from_numpy(attrs).to(device)
    full = restate(dens, counts, LEVEL, MINS, SPACINGS, attrs)
    nv, nf = (int(t) for t in full['totals'])
    assert nv > 40 and nf > 20 and full['cell_offsets'].shape == (2,)
    cases = [(None, None, nv // 2, nf // 3), (None, None, 0, 0), ((5, nv + 100), (-3, 10 ** 6), nv, nf),
             ((-10 ** 6, -256), (2 ** 31 - 1, -2 ** 31), nv, nf), ((2 ** 31 - 1, -2 ** 31), (nf - 4, -1), nv + 3, nf + 3),
             ((nv - 7, -3), (3, -2 ** 31), 11, 7), ((0, 0), (0, 0), 11, 7)]
    for co, fo, vcap, fcap in cases:
        want = restate(dens, counts, LEVEL, MINS, SPACINGS, attrs, cell_offsets=co, face_offsets=fo, vertex_cap=vcap, face_cap=fcap)
        got = raw_call(device, dens_t, 1, attrs_t, n_attr, n_attr, counts, LEVEL, cell_offsets=co, face_offsets=fo, vertex_cap=vcap,
                       face_cap=fcap, guard=64)
        check_raw(got, want, (co, fo, vcap, fcap), owned=(co, fo) != ((0, 0), (0, 0)))      # (the last case: both tiles from 0)


# ---------------------------------------------------------------------------------------------------------------- properties
def properties(vertices, faces, positive):
    """A closed oriented surface: every directed edge once, with its reverse; V - E + F = 2; the sign of the fp64 volume."""
    f = faces.astype(np.int64)
    assert f.min() >= 0 and f.max() < vertices.shape[0] and np.unique(f).shape[0] == vertices.shape[0]
    directed = np.concatenate([np.stack([f[:, i], f[:, (i + 1) % 4]], axis=1) for i in range(4)])
    as_set = set(map(tuple, directed.tolist()))
    assert len(as_set) == directed.shape[0]
    assert all((b, a) in as_set for a, b in as_set)
    n_edges = len(as_set) // 2
    assert vertices.shape[0] - n_edges + f.shape[0] == 2, (vertices.shape[0], n_edges, f.shape[0])
    p = vertices[:, :3].astype(np.float64)
    volume = 0.0
    for tri in (f[:, [0, 1, 2]], f[:, [0, 2, 3]]):
        volume += np.einsum('ij,ij->i', p[tri[:, 0]], np.cross(p[tri[:, 1]], p[tri[:, 2]])).sum() / 6.0
    assert (volume > 0) if positive else (volume < 0), volume
    return volume


def sphere_field(counts=(12, 13, 14), centre=(5.3, 6.1, 6.7), radius=3.6):
    """sigmoid(radius - distance to the centre), in grid units: 0.5 on the sphere, which lies strictly inside the grid."""
    idx = np.indices(counts).astype(np.float64)
    dist = np.sqrt(sum((idx[a] - centre[a]) ** 2 for a in range(3)))
    return (1.0 / (1.0 + np.exp(-(radius - dist)))).astype(F32).reshape(-1)


def check_sphere(device):
    counts = (12, 13, 14)
    field = sphere_field(counts)
    attrs = torch.from_numpy(np.stack([field, 1 - field], axis=1)).to(device)
    v, f = pk.ops.surface_nets(torch.from_numpy(field).to(device), counts, 0.5, MINS, SPACINGS, attrs=attrs)
    vol = properties(v.cpu().numpy(), f.cpu().numpy(), positive=True)
    cell = SPACINGS[0] * SPACINGS[1] * SPACINGS[2]
    assert 0.7 < vol / (4.0 / 3.0 * np.pi * 3.6 ** 3 * cell) < 1.1, vol
    v2, f2 = pk.ops.surface_nets(torch.from_numpy(-field).to(device), counts, -0.5, MINS, SPACINGS)
    assert properties(v2.cpu().numpy(), f2.cpu().numpy(), positive=False) < 0


def check_plane(device):
    counts = (6, 5, 4)
    field = (F32(0.25) * np.indices(counts)[0].astype(F32)).reshape(-1)
    v, f = pk.ops.surface_nets(torch.from_numpy(field).to(device), counts, 0.625, MINS, SPACINGS)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert v.shape == (12, 3) and f.shape == (6, 4)
    assert same_bits(v[:, 0], np.full(12, F32(3.0) * F32(SPACINGS[0]) + F32(MINS[0]), F32))
    normal = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 3]] - v[f[:, 0]])
    assert (normal[:, 0] < 0).all() and (normal[:, 1:] == 0).all()       # inside is ix >= 3: the normal points to -x


def check_argument_errors(device):
    """The contracts through the Python layer and the raw entry points, as the library on `device` states them."""
    z = lambda *shape, **k: torch.zeros(*shape, device=device, **k)
    I32 = torch.int32
    nets = pk.ops.surface_nets
    with pytest.raises(AssertionError, match='values must be'):
        nets(z(63), (4, 4, 4), 0.5, MINS, SPACINGS)
    with pytest.raises(AssertionError, match='attrs must hold'):
        nets(z(64), (4, 4, 4), 0.5, MINS, SPACINGS, attrs=z(63, 2))
    with pytest.raises(AssertionError, match='n_attr = 33'):
        nets(z(64), (4, 4, 4), 0.5, MINS, SPACINGS, attrs=z(64, 33))
    v, f = nets(z(0), (4, 0, 4), 0.5, MINS, SPACINGS, attrs=z(0, 2))          # an empty grid
    assert v.shape == (0, 5) and f.shape == (0, 4)
    v, f, totals = nets(z(0), (0, 4, 4), 0.5, MINS, SPACINGS, sync=False)
    assert v.shape == (0, 3) and f.shape == (0, 4) and totals.cpu().tolist() == [0, 0]
    L, p = pk._lib.lib(), pk.ops._ptr
    EINVAL, OK = pk._lib.EINVAL, pk._lib.OK
    count = lambda d, ld, nx, ny, nz, co, fo, t: L.occ4d_surface_count_f32(p(d), ld, nx, ny, nz, 0.5, p(co), p(fo), p(t), None)
    assert count(z(64), 1, -1, 4, 4, z(1, dtype=I32), z(1, dtype=I32), z(2, dtype=I32)) == EINVAL
    assert count(z(64), 0, 4, 4, 4, z(1, dtype=I32), z(1, dtype=I32), z(2, dtype=I32)) == EINVAL
    assert count(None, 1, 4, 4, 4, z(1, dtype=I32), z(1, dtype=I32), z(2, dtype=I32)) == EINVAL
    assert count(z(64), 1, 4, 4, 4, z(1, dtype=I32), z(1, dtype=I32), None) == EINVAL
    assert count(z(64), 1, 1024, 1024, 1024, z(1, dtype=I32), z(1, dtype=I32), z(2, dtype=I32)) == EINVAL
    assert b'INT32_MAX' in L.occ4d_last_error()
    assert count(None, 1, 0, 4, 4, None, None, None) == OK                    # an empty grid touches no pointer

    def write(**k):
        a = dict(density=p(z(64)), ld=1, attrs=p(z(64, 2)), ld_attr=2, n_attr=2, nx=4, ny=4, nz=4, level=0.5, x0=0.0, sx=1.0, y0=0.0,
                 sy=1.0, z0=0.0, sz=1.0, cell_offsets=p(z(1, dtype=I32)), face_offsets=p(z(1, dtype=I32)), work=p(z(64, dtype=I32)),
                 vertices=p(z(27, 5)), ld_v=5, vertex_cap=27, faces=p(z(36, 4, dtype=I32)), face_cap=36)
        a.update(k)
        return L.occ4d_surface_write_f32(*a.values(), None)
    assert write() == OK
    assert write(n_attr=33) == EINVAL and write(n_attr=-1) == EINVAL
    assert write(ld_attr=1) == EINVAL and write(ld_v=4) == EINVAL
    assert write(attrs=None) == EINVAL and b'null attrs' in L.occ4d_last_error()
    assert write(vertex_cap=-1) == EINVAL and write(face_cap=-1) == EINVAL
    assert write(work=None) == EINVAL and write(vertices=None) == EINVAL and write(faces=None) == EINVAL
    assert write(attrs=None, n_attr=0, ld_attr=0, ld_v=3) == OK
    assert write(vertices=None, vertex_cap=0, faces=None, face_cap=0) == OK
    assert write(nx=0, density=None, attrs=None, cell_offsets=None, face_offsets=None, work=None, vertices=None, faces=None) == OK
    if device.type == 'cuda':
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- end to end
COUNTS, N_QUERIES = rc.COUNTS, rc.N_QUERIES


def frame_of(shared):
    inf = shared.inputs[3]
    counts, mins, spacings = pk.geometry.grid_frame(rc.CASE['num_sample'], inf['min_z'], inf['cube_bounds'], 'greater', 4)
    assert tuple(counts) == COUNTS
    return mins, spacings


def check_against_restatement(shared, got, level=0.5):
    """result['surface'] equals the restatement on result['implicit_output'] (density column 0, all columns as attributes)."""
    mins, spacings = frame_of(shared)
    out = got['implicit_output']
    want = restate(out[:, 0], COUNTS, level, mins, spacings, out)
    mesh = got['surface']
    assert sorted(mesh) == ['faces', 'vertices'] and all(isinstance(a, np.ndarray) for a in mesh.values())
    assert mesh['vertices'].shape[1] == 3 + out.shape[1]
    assert same_mesh(mesh['vertices'], mesh['faces'], want)
    return want


def without_surface(result):
    return {k: v for k, v in result.items() if k != 'surface'}


def check_single_run(shared):
    got = rc.infer(shared.device, shared.inputs, surface=pk.surface.Surface())
    want = check_against_restatement(shared, got)
    assert want['totals'][0] > 0 and want['totals'][1] > 0                  # the fixture's condition: there is a surface
    same_result(without_surface(got), shared.dense)
    # another level than the split's
    got = rc.infer(shared.device, shared.inputs, surface=pk.surface.Surface(level=0.47))
    assert check_against_restatement(shared, got, level=0.47)['totals'][0] > 0
    same_result(without_surface(got), shared.dense)
    # the positions lie inside the query grid's hull, the attributes' density column around the level
    v = got['surface']['vertices']
    q = shared.dense['points_query']
    assert (v[:, :3] >= q[:, :3].min(axis=0)).all() and (v[:, :3] <= q[:, :3].max(axis=0)).all()


def check_refine(shared):
    """Under refine the mesh is that of the expanded array; a cell whose corners all lie in inactive blocks is never crossed."""
    refine = pk.inference.GridRefine(2, 0.46, 1)
    plain = rc.infer(shared.device, shared.inputs, refine=refine)
    got = rc.infer(shared.device, shared.inputs, refine=refine, surface=pk.surface.Surface())
    want = check_against_restatement(shared, got)
    assert got['refine'] == plain['refine']
    plain.pop('refine')
    rest = without_surface(got)
    rest.pop('refine')
    same_result(rest, plain)
    _, active, _ = rc.restate_refine(shared.dense['implicit_output'], COUNTS, 2, 1, 0.46)
    inactive = (active[rc.block_of_points(COUNTS, 2)] == 0).reshape(COUNTS)
    assert inactive.any() and not inactive.all()
    all_inactive = np.zeros(COUNTS, bool)
    all_inactive[:-1, :-1, :-1] = np.logical_and.reduce([corner_view(inactive, COUNTS, (o >> 2 & 1, o >> 1 & 1, o & 1)) for o in range(8)])
    assert all_inactive.any() and not want['crossed'].reshape(COUNTS)[all_inactive].any()
    assert (want['work'].reshape(COUNTS)[all_inactive] == -1).all()


def check_track_all(shared):
    """track_mode 'all': the mesh of the merged array, the device merge equal to the host merge."""
    on_device = rc.infer(shared.device, shared.inputs, track_mode='all', surface=pk.surface.Surface(), track_merge='device')
    on_host = rc.infer(shared.device, shared.inputs, track_mode='all', surface=pk.surface.Surface(), track_merge='host')
    for got in (on_device, on_host):
        assert check_against_restatement(shared, got)['totals'][0] > 0
        same_result(without_surface(got), shared.dense_all)
    assert same_mesh(on_device['surface']['vertices'], on_device['surface']['faces'], on_host['surface'])


def check_clip(shared):
    """evaluate_clip(surface=..., meshes=[]) over two frames: one mesh per frame, that of the perform_inference call."""
    device = shared.device
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = rc.clip_inputs(shared)
    meshes = []
    clip = pk.evaluation.evaluate_clip(batch, [enc, dec], device, args, 'greater', save_gt=True, surface=pk.surface.Surface(),
                                       meshes=meshes)
    dense = pk.evaluation.evaluate_clip(batch, [enc, dec], device, args, 'greater', save_gt=True)
    assert len(clip) == len(dense) == len(meshes) == 2
    for t in range(2):
        assert len(clip[t]) == 7
        for got, want in zip(clip[t], dense[t]):
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        res = pk.inference.perform_inference(
            pcl.clone(), None, frames[t], [enc, dec], device, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], t, None,
            sample_implicit=True, num_sample=rc.CASE['num_sample'], point_sample_mode='grid', batch_size=rc.CASE['batch_size'],
            predict_segmentation=False, track_mode='none', semantic_classes=13, density_threshold=0.5, data_kind='greater',
            cube_mode=4, compress_air=True, point_occupancy_radius=0.8, surface=pk.surface.Surface())
        assert same_mesh(meshes[t]['vertices'], meshes[t]['faces'], res['surface']) and meshes[t]['vertices'].shape[0] > 0
    with pytest.raises(ValueError, match='meshes'):
        pk.evaluation.evaluate_clip(batch, [enc, dec], device, args, 'greater', surface=pk.surface.Surface())


def check_none_is_untouched(shared, monkeypatch):
    """surface=None: no new key, the one host wait, and no surface entry point is called."""
    calls = rc.count_waits(monkeypatch)

    def forbidden(*a, **k):
        raise AssertionError('surface=None must not reach the surface extraction')
    monkeypatch.setattr(pk.ops, 'surface_nets', forbidden)
    monkeypatch.setattr(pk.surface, 'extract', forbidden)
    L = pk._lib.lib()
    for name in pk._lib.SURFACE_SIGNATURES:
        monkeypatch.setattr(L, name, forbidden)
    res = rc.infer(shared.device, shared.inputs, surface=None)
    assert calls == dict(wait=1)
    assert sorted(res) == ['features_global', 'gt_air', 'gt_solid', 'implicit_output', 'output_air', 'output_solid', 'pcl_abstract',
                           'points_query']
    same_result(res, shared.dense)
    monkeypatch.undo()
    calls = rc.count_waits(monkeypatch)
    rc.infer(shared.device, shared.inputs, surface=pk.surface.Surface())
    assert calls['wait'] == 1                                           # (the mesh adds a count read, not a wait on the copies)


def check_value_errors(shared):
    with pytest.raises(ValueError, match='grid'):
        rc.infer(shared.device, shared.inputs, surface=pk.surface.Surface(), point_sample_mode='random')
    with pytest.raises(ValueError, match='NaN'):
        pk.surface.Surface(level=float('nan'))
    with pytest.raises(ValueError, match='NaN'):
        pk.surface.Surface().resolve(float('nan'))
    with pytest.raises(ValueError, match='NaN'):
        pk.surface.extract(torch.zeros((8, 2), device=shared.device), (2, 2, 2), (0, 0, 0), (1, 1, 1), float('nan'))
    with pytest.raises(ValueError):
        rc.infer(shared.device, shared.inputs, surface=0.5)
    assert pk.surface.Surface().level is None and pk.surface.Surface(1).level == 1.0


def read_ply(path):
    with open(path, 'rb') as f:
        data = f.read()
    head, body = data.split(b'end_header\n', 1)
    lines = head.decode('ascii').split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0'
    nv = int([ln for ln in lines if ln.startswith('element vertex')][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith('element face')][0].split()[-1])
    colour = 'property uchar red' in lines
    vdt = np.dtype([('xyz', '<f4', (3,))] + ([('rgb', 'u1', (3,))] if colour else []))
    fdt = np.dtype([('count', 'u1'), ('index', '<i4', (4,))])
    assert len(body) == nv * vdt.itemsize + nf * fdt.itemsize
    vert = np.frombuffer(body, vdt, nv)
    face = np.frombuffer(body, fdt, nf, offset=nv * vdt.itemsize)
    assert (face['count'] == 4).all()
    return vert['xyz'], (vert['rgb'] if colour else None), face['index']


def check_write_ply(tmp_path):
    rng = np.random.default_rng(1)
    v = rng.uniform(-3, 3, size=(37, 8)).astype(F32)
    v[:, 4:7] = rng.uniform(-0.2, 1.2, size=(37, 3)).astype(F32)
    f = rng.integers(0, 37, size=(21, 4)).astype(np.int32)
    path = str(tmp_path / 'mesh.ply')
    pk.surface.write_ply(path, v, f)
    xyz, rgb, index = read_ply(path)
    assert rgb is None and same_bits(np.ascontiguousarray(xyz), v[:, :3]) and np.array_equal(index, f)
    pk.surface.write_ply(path, torch.from_numpy(v), torch.from_numpy(f), rgb_columns=(4, 5, 6))
    xyz, rgb, index = read_ply(path)
    assert same_bits(np.ascontiguousarray(xyz), v[:, :3]) and np.array_equal(index, f)
    assert np.array_equal(rgb, np.rint(np.clip(v[:, 4:7], 0, 1) * 255).astype(np.uint8))
    pk.surface.write_ply(path, v[:0], f[:0])
    xyz, rgb, index = read_ply(path)
    assert xyz.shape == (0, 3) and index.shape == (0, 4)
