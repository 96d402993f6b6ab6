"""Shared by tests/test_components_host.py (g++ twin) and tests/test_gpu_components.py (HIP): the yardstick of the connected
components of the grid's solid set -- a plain breadth-first-search restatement of the rules of include/ext/occ4d_components.h in
numpy / Python --, the case matrix, and the comparison, which is EQUAL everywhere: integers only, no tolerance.

TILE.  Pass 1 of csrc/components.hip labels tiles of (6, 7, 6) points (x, y, z) in LDS; the numbering passes work on tiles of 256
consecutive flat indices.  The grids below are chosen against the first: (6, 7, 6) is exactly one tile, (7, 8, 7) one point larger on
every axis, (40, 24, 20) is 7 x 4 x 4 tiles with no axis a multiple of its tile edge (40 = 6 * 6 + 4, 24 = 3 * 7 + 3, 20 = 3 * 6 + 2);
(2, 3, 70) has z-runs longer than a wave, and 420 points: two numbering tiles."""
import functools

import numpy as np
import pytest
import torch

import raycast_cases as yc
import refine_cases as rc
import occlusions4d_amd as pk

SYMBOLS = ['occ4d_components_label_f32', 'occ4d_components_table_i64']

TILE = (6, 7, 6)
GRIDS = [(1, 1, 1), (1, 1, 5), (2, 3, 70), (6, 7, 6), (7, 8, 7), (17, 9, 33), (40, 24, 20)]
BIG = (40, 24, 20)
CONNECTIVITIES = (6, 18, 26)
COLS = 12
CANARY = -0x0123456789ABCDEF
NAN, INF = float('nan'), float('inf')


# ---------------------------------------------------------------------------------------------------------------- the restatement
def offsets(connectivity):
    rank = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
            if 1 <= (dx != 0) + (dy != 0) + (dz != 0) <= rank]


def members(field, level, mask=None, mask_level=0.0, klass=None):
    with np.errstate(invalid='ignore'):
        m = field >= np.float32(level)                                    # a NaN on either side: False
        if mask is not None:
            m &= mask >= np.float32(mask_level)
    if klass is not None:
        m &= klass >= 0
    return m


def restate(field, counts, level, connectivity=6, min_size=1, mask=None, mask_level=0.0, klass=None):
    """-> (labels (n,) int32, totals (3,) int32, table (K, 12) int64) by the rules, one breadth-first search per component in the
    order of the flat index: the first point a search starts from is its component's root."""
    nx, ny, nz = counts
    n = nx * ny * nz
    m = members(field, level, mask, mask_level, klass).reshape(counts)
    k3 = None if klass is None else klass.reshape(counts)
    offs = offsets(connectivity)
    comp = np.full(counts, -1, np.int64)                                  # component index in the order of roots, all of them
    rows = []
    for p in np.flatnonzero(m.reshape(-1)):
        start = (p // (ny * nz), (p // nz) % ny, p % nz)
        if comp[start] >= 0:
            continue
        c = len(rows)
        comp[start] = c
        queue, points = [start], []
        while queue:
            x, y, z = queue.pop()
            points.append((x, y, z))
            for dx, dy, dz in offs:
                q = (x + dx, y + dy, z + dz)
                if 0 <= q[0] < nx and 0 <= q[1] < ny and 0 <= q[2] < nz and m[q] and comp[q] < 0 \
                        and (k3 is None or k3[q] == k3[start]):
                    comp[q] = c
                    queue.append(q)
        pts = np.array(points, np.int64)
        rows.append([len(pts), int(p), -1 if k3 is None else int(k3[start])] + pts.sum(0).tolist() + pts.min(0).tolist()
                    + pts.max(0).tolist())
    full = np.array(rows, np.int64).reshape(-1, COLS)
    kept = full[:, 0] >= min_size
    number = np.where(kept, np.cumsum(kept) - 1, -1)
    comp = comp.reshape(-1)
    labels = np.where(comp >= 0, number[np.maximum(comp, 0)] if len(number) else -1, -1).astype(np.int32)
    table = full[kept]
    totals = np.array([kept.sum(), table[:, 0].sum(), len(full)], np.int32)
    return labels, totals, table


# ---------------------------------------------------------------------------------------------------------------- the fields
def coords(counts):
    return np.meshgrid(*(np.arange(c) for c in counts), indexing='ij')


def checkerboard(counts):
    x, y, z = coords(counts)
    return ((x + y + z) % 2 == 0).astype(np.float32).reshape(-1)


def boxes(counts, *ranges):
    f = np.zeros(counts, np.float32)
    for (x0, x1), (y0, y1), (z0, z1) in ranges:
        f[x0:x1, y0:y1, z0:z1] = 1.0
    return f.reshape(-1)


def edge_cubes(counts):
    """Two boxes that share only an edge (they differ on x and y across it): separate at 6, one at 18."""
    return boxes(counts, ((2, 4), (2, 4), (2, 6)), ((4, 6), (4, 6), (2, 6)))


def corner_cubes(counts):
    """Two cubes that share only the corner between points (5, 6, 5) and (6, 7, 6): the corner of the first (6, 7, 6) tile."""
    return boxes(counts, ((4, 6), (5, 7), (4, 6)), ((6, 8), (7, 9), (6, 8)))


def serpentine(counts):
    """A single-voxel-wide path through the whole grid: the z-lines at even x and even y, walked back and forth, joined by one voxel
    at the end where the walk turns (at odd y inside a plane, at odd x between planes).  At 6-connectivity one chain; its root
    (0, 0, 0) is as far from its tail as a path in this grid gets."""
    nx, ny, nz = counts
    f = np.zeros(counts, np.float32)
    lines = []
    for xi, x in enumerate(range(0, nx, 2)):
        ys = list(range(0, ny, 2))
        lines += [(x, y) for y in (ys if xi % 2 == 0 else ys[::-1])]
    for i, (x, y) in enumerate(lines):
        f[x, y, :] = 1.0
        if i + 1 < len(lines):
            x2, y2 = lines[i + 1]
            z_end = nz - 1 if i % 2 == 0 else 0
            f[(x + x2) // 2, (y + y2) // 2, z_end] = 1.0
    return f.reshape(-1)


def comb(counts):
    """Teeth: the x-lines (0 .. nx - 2, y, z) at even y and z in {1, 8, 15}: 36 teeth through every layer of tiles, no two adjacent at
    any connectivity.  They meet only in the last layer of tiles: the plane x = nx - 1 joins the teeth of one z along y, and the
    three z-groups join only through the line (nx - 1, ny - 1, :), which ends in the last tile in raster order: every equivalence
    between teeth is found late."""
    nx, ny, nz = counts
    f = np.zeros(counts, np.float32)
    for z in (1, 8, 15):
        f[:nx - 1, 0:ny:2, z] = 1.0
        f[nx - 1, :, z] = 1.0
    f[nx - 1, ny - 1, :] = 1.0
    return f.reshape(-1)


def random_field(counts, density, seed):
    """Uniform values in [0, 1): the fraction `density` lies at or above level 1 - density."""
    return np.random.default_rng(seed).random(counts[0] * counts[1] * counts[2], dtype=np.float32)


def with_specials(values, seed):
    """NaN, +inf and -inf sprinkled over an array: each on about 3 % of the points."""
    out = values.copy()
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, 33, len(out))
    out[pick == 0], out[pick == 1], out[pick == 2] = NAN, INF, -INF
    return out


def classes(counts, seed):
    """Three classes, random per point but one per (x, y) column on every other z-layer, plus 10 % negative entries; (5, 3, 3) and (6, 3, 3), neighbours across the first
    tile border on x, get classes 0 and 1."""
    rng = np.random.default_rng(seed)
    n = counts[0] * counts[1] * counts[2]
    k = rng.integers(0, 3, n).astype(np.int32).reshape(counts)
    k[:, :, ::2] = k[:, :, :1]                                            # some structure: every other z-layer one class per (x, y)
    k = k.reshape(-1)
    k[rng.random(n) < 0.1] = -rng.integers(1, 5)
    k = k.reshape(counts)
    if counts[0] > 6 and counts[1] > 3 and counts[2] > 3:
        k[5, 3, 3], k[6, 3, 3] = 0, 1
    return k.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- the matrix
def case(name, counts, field, level=0.5, connectivity=6, min_size=1, mask=None, mask_level=0.5, klass=None, cap=None, wide=False):
    return dict(name=name, counts=counts, field=np.ascontiguousarray(field, np.float32), level=level, connectivity=connectivity,
                min_size=min_size, mask=mask, mask_level=mask_level, klass=klass, cap=cap, wide=wide)


def _cases():
    out = []
    for counts in GRIDS:
        n = counts[0] * counts[1] * counts[2]
        g = '%dx%dx%d' % counts
        for c in CONNECTIVITIES:
            out.append(case('%s-air-%d' % (g, c), counts, np.zeros(n), connectivity=c))
            out.append(case('%s-solid-%d' % (g, c), counts, np.ones(n), connectivity=c))
            out.append(case('%s-checker-%d' % (g, c), counts, checkerboard(counts), connectivity=c))
        out.append(case('%s-checker-min2' % g, counts, checkerboard(counts), min_size=2))           # drops every component
        out.append(case('%s-level-nan' % g, counts, np.ones(n), level=NAN))
    for counts in ((17, 9, 33), BIG):
        n = counts[0] * counts[1] * counts[2]
        g = '%dx%dx%d' % counts
        for c in CONNECTIVITIES:
            out.append(case('%s-edge-cubes-%d' % (g, c), counts, edge_cubes(counts), connectivity=c))
            out.append(case('%s-corner-cubes-%d' % (g, c), counts, corner_cubes(counts), connectivity=c))
            for density, seed in ((0.2, 11), (0.31, 12), (0.6, 13)):
                out.append(case('%s-random-%g-%d' % (g, density, c), counts, random_field(counts, density, seed), level=1.0 - density,
                                connectivity=c))
        field = random_field(counts, 0.31, 12)
        for min_size in (2, 50):
            out.append(case('%s-random-min%d' % (g, min_size), counts, field, level=0.69, min_size=min_size))
        out.append(case('%s-random-min-all' % g, counts, field, level=0.69, min_size=n))             # drops every component
        mask = random_field(counts, 0.7, 14)
        out.append(case('%s-mask' % g, counts, random_field(counts, 0.6, 13), level=0.4, mask=mask, mask_level=0.3, connectivity=18))
        out.append(case('%s-specials' % g, counts, with_specials(random_field(counts, 0.5, 15), 16), level=0.5,
                        mask=with_specials(mask, 17), mask_level=0.3, connectivity=26))
        out.append(case('%s-level-inf' % g, counts, with_specials(random_field(counts, 0.5, 15), 16), level=INF))
        out.append(case('%s-level-minus-inf' % g, counts, with_specials(random_field(counts, 0.5, 15), 16), level=-INF, min_size=2))
        for c in CONNECTIVITIES:
            out.append(case('%s-classes-%d' % (g, c), counts, np.maximum(random_field(counts, 0.6, 18), boxes(counts, ((5, 7), (3, 4), (3, 4)))),
                            level=0.4, klass=classes(counts, 19), connectivity=c))
        out.append(case('%s-classes-mask-min2' % g, counts, random_field(counts, 0.6, 18), level=0.4, klass=classes(counts, 19),
                        mask=mask, mask_level=0.2, min_size=2, connectivity=26))
        out.append(case('%s-wide' % g, counts, random_field(counts, 0.31, 12), level=0.69, mask=mask, mask_level=0.1, wide=True))
        out.append(case('%s-cap-small' % g, counts, random_field(counts, 0.2, 11), level=0.8, cap=7))
        out.append(case('%s-cap-one' % g, counts, random_field(counts, 0.2, 11), level=0.8, klass=classes(counts, 19), cap=1))
        out.append(case('%s-cap-large' % g, counts, edge_cubes(counts), cap=5))
    for c in CONNECTIVITIES:
        out.append(case('serpentine-%d' % c, BIG, serpentine(BIG), connectivity=c))
        out.append(case('comb-%d' % c, BIG, comb(BIG), connectivity=c))
    out.append(case('serpentine-min', BIG, serpentine(BIG), min_size=int(serpentine(BIG).sum())))
    return out


CASES = _cases()
NAMES = [c['name'] for c in CASES]
BY_NAME = dict(zip(NAMES, CASES))
assert len(BY_NAME) == len(CASES)
RANDOM_BIG = [n for n in NAMES if n.startswith('40x24x20-random-')]


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement of a case, computed once per process; the arrays are read-only."""
    c = BY_NAME[name]
    got = restate(c['field'], c['counts'], c['level'], c['connectivity'], c['min_size'], c['mask'], c['mask_level'], c['klass'])
    for a in got:
        a.setflags(write=False)
    return got


# ---------------------------------------------------------------------------------------------------------------- the comparison
def run(c, device):
    """The case through ops.grid_components -> numpy (labels, totals, table, rows behind the table or None)."""
    n = c['counts'][0] * c['counts'][1] * c['counts'][2]
    if c['wide']:                                                         # the field and the mask as columns 2 and 4 of an (n, 5) array
        wide = np.full((n, 5), 7.0, np.float32)
        wide[:, 2] = c['field']
        wide[:, 4] = c['mask']
        wide = torch.from_numpy(wide).to(device)
        values, mask = wide[:, 2], wide[:, 4]
    else:
        values = torch.from_numpy(c['field']).to(device)
        mask = None if c['mask'] is None else torch.from_numpy(np.ascontiguousarray(c['mask'], np.float32)).to(device)
    klass = None if c['klass'] is None else torch.from_numpy(c['klass']).to(device)
    buffer = None
    if c['cap'] is not None:
        buffer = torch.full((c['cap'] + 2, COLS), CANARY, dtype=torch.int64, device=device)
    labels, totals, table = pk.ops.grid_components(values, c['counts'], c['level'], c['connectivity'], c['min_size'], mask, c['mask_level'],
                                                   klass, cap=c['cap'], table=buffer)
    return (labels.cpu().numpy(), totals.cpu().numpy(), table.cpu().numpy(), None if buffer is None else buffer.cpu().numpy())


def same(got, name):
    """Whether a run's arrays equal the restatement of the case: labels and totals whole; the table's rows below min(cap, kept
    components); with a cap every row from there on, the two behind the table included, still the canary."""
    c = BY_NAME[name]
    labels, totals, table, buffer = got
    want_labels, want_totals, want_table = expected(name)
    assert labels.dtype == np.int32 and totals.dtype == np.int32 and table.dtype == np.int64
    ok = np.array_equal(labels, want_labels) and np.array_equal(totals, want_totals)
    if c['cap'] is None:
        return ok and np.array_equal(table, want_table)
    rows = min(c['cap'], len(want_table))
    return ok and np.array_equal(buffer[:rows], want_table[:rows]) and bool((buffer[rows:] == CANARY).all()) \
        and len(buffer) == c['cap'] + 2


def check(name, device):
    assert same(run(BY_NAME[name], device), name), name


def check_expectations_by_hand():
    """What the patterns are there for, checked on the restatement itself."""
    for counts in GRIDS:
        n = counts[0] * counts[1] * counts[2]
        g = '%dx%dx%d' % counts
        for c in CONNECTIVITIES:
            labels, totals, table = expected('%s-air-%d' % (g, c))
            assert totals.tolist() == [0, 0, 0] and (labels == -1).all() and table.shape == (0, COLS)
            labels, totals, table = expected('%s-solid-%d' % (g, c))
            assert totals.tolist() == [1, n, 1] and (labels == 0).all()
            assert table.tolist() == [[n, 0, -1] + [s * (s - 1) // 2 * (n // s) for s in counts] + [0, 0, 0] + [s - 1 for s in counts]]
        assert expected('%s-checker-6' % g)[1].tolist() == [(n + 1) // 2] * 3
        if sum(s >= 2 for s in counts) >= 2:                              # (on a line the checkerboard's points are two apart)
            assert expected('%s-checker-18' % g)[1].tolist() == expected('%s-checker-26' % g)[1].tolist() == [1, (n + 1) // 2, 1]
        assert expected('%s-checker-min2' % g)[1].tolist() == [0, 0, (n + 1) // 2]
        assert expected('%s-level-nan' % g)[1].tolist() == [0, 0, 0]
    for g in ('17x9x33', '40x24x20'):
        assert [int(expected('%s-edge-cubes-%d' % (g, c))[1][0]) for c in CONNECTIVITIES] == [2, 1, 1]
        assert [int(expected('%s-corner-cubes-%d' % (g, c))[1][0]) for c in CONNECTIVITIES] == [2, 2, 1]
        assert expected('%s-random-min-all' % g)[1][:2].tolist() == [0, 0] and expected('%s-random-min-all' % g)[1][2] > 50
        assert expected('%s-level-inf' % g)[1][0] > 0 and expected('%s-cap-small' % g)[1][0] > 7
        k = BY_NAME['%s-classes-6' % g]['klass'].reshape(BY_NAME['%s-classes-6' % g]['counts'])
        lab = expected('%s-classes-26' % g)[0].reshape(k.shape)
        assert k[5, 3, 3] == 0 and k[6, 3, 3] == 1 and lab[5, 3, 3] >= 0 and lab[6, 3, 3] >= 0 and lab[5, 3, 3] != lab[6, 3, 3]
    length = int(serpentine(BIG).sum())
    for c in CONNECTIVITIES:
        assert expected('serpentine-%d' % c)[1].tolist() == [1, length, 1] and expected('serpentine-%d' % c)[2][0, 1] == 0
        assert expected('comb-%d' % c)[1].tolist() == [1, int(comb(BIG).sum()), 1]
    assert expected('serpentine-min')[1].tolist() == [1, length, 1] and length > 20 * 12 * 20


def scipy_labels(name, ndimage):
    c = BY_NAME[name]
    m = members(c['field'], c['level'], c['mask'], c['mask_level']).reshape(c['counts'])
    rank = {6: 1, 18: 2, 26: 3}[c['connectivity']]
    lab, count = ndimage.label(m, structure=ndimage.generate_binary_structure(3, rank))
    return lab.reshape(-1).astype(np.int32) - 1, count


SCIPY_NAMES = [n for n in NAMES if BY_NAME[n]['klass'] is None and BY_NAME[n]['min_size'] == 1]


# ---------------------------------------------------------------------------------------------------------------- the rejected calls
def check_argument_errors(device):
    """ops.grid_components: rejected arguments raise AssertionError with the library's text (the table of both libraries' texts is
    tests/test_gpu_components_contract_texts.py); an empty grid is a no-op."""
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=device)
    call = lambda **k: pk.ops.grid_components(**dict(dict(values=z(30), counts=(3, 2, 5), level=0.5), **k))
    for kw, text in ((dict(connectivity=4), 'connectivity = 4 must be 6, 18 or 26'), (dict(min_size=0), 'min_size = 0 must be >= 1'),
                     (dict(counts=(-3, -2, 5)), 'nx = -3, ny = -2, nz = 5 must be >= 0'), (dict(cap=-1), 'cap = -1 must be >= 0'),
                     (dict(values=z(29)), r'values must be \(30,\)'), (dict(mask=z(31)), r'mask must be \(30,\)'),
                     (dict(klass=z(30)), 'klass must be torch.int32'), (dict(klass=z(60, dtype=torch.int32)[::2]), 'klass must be a contiguous'),
                     (dict(cap=3, table=z(2, 12, dtype=torch.int64)), 'table must be a contiguous'), (dict(table=z(2, 12, dtype=torch.int64)), 'needs cap')):
        with pytest.raises(AssertionError, match=text):
            call(**kw)
    for counts in ((0, 2, 5), (3, 0, 0)):
        labels, totals, table = call(values=z(0), counts=counts)
        assert labels.shape == (0,) and totals.tolist() == [0, 0, 0] and table.shape == (0, COLS)
    labels, totals, table = call(values=z(30) + 1, cap=0)
    assert totals.tolist() == [1, 30, 1] and table.shape == (0, COLS)


# ---------------------------------------------------------------------------------------------------------------- end to end
def restate_result(got, counts, level=0.5, **kw):
    return restate(np.ascontiguousarray(got['implicit_output'][:, 0]), counts, level, **kw)


def check_result(got, counts, level=0.5, **kw):
    comp = got['components']
    assert sorted(comp) == ['labels', 'table'] and all(isinstance(a, np.ndarray) for a in comp.values())
    labels, totals, table = restate_result(got, counts, level, **kw)
    assert comp['labels'].dtype == np.int32 and comp['table'].dtype == np.int64 and comp['table'].shape == (totals[0], COLS)
    assert np.array_equal(comp['labels'], labels) and np.array_equal(comp['table'], table)
    return labels, totals, table


def without_components(result):
    return {k: v for k, v in result.items() if k != 'components'}


def direct(shared, **kw):
    """perform_inference on the fixture with compress_air=False."""
    pcl, sem, target, inf, enc, dec = shared.inputs
    return pk.inference.perform_inference(
        pcl.clone(), None, target.copy(), [enc, dec], shared.device, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'],
        rc.CASE['time_idx'], None, sample_implicit=True, num_sample=rc.CASE['num_sample'], batch_size=rc.CASE['batch_size'],
        predict_segmentation=False, track_mode='none', semantic_classes=13, density_threshold=0.5, data_kind='greater', cube_mode=4,
        compress_air=False, point_occupancy_radius=0.8, point_sample_mode='grid', **kw)


def check_end_to_end(shared):
    views = yc.fixture_views(shared)
    got = direct(shared, components=pk.components.Components(), views=views)
    labels, totals, table = check_result(got, rc.COUNTS)
    assert totals[0] >= 1 and (got['components']['labels'][got['implicit_output'][:, 0] < 0.5] == -1).all()
    assert totals[1] == len(got['output_solid']) == (got['components']['labels'] >= 0).sum()
    cell = got['views']['cell']
    ids = got['components']['labels'][cell[cell >= 0]]                     # a component id per pixel that shows something
    assert (cell >= 0).any() and ids.shape == (int((cell >= 0).sum()),) and ids.min() >= -1 and ids.max() < totals[0]
    rc.same_result({k: v for k, v in got.items() if k not in ('components', 'views', 'output_air', 'gt_air')},
                   {k: v for k, v in shared.dense.items() if k not in ('output_air', 'gt_air')})
    # the options: level, connectivity, min_size, select
    track = pk.inference.get_track_idx(shared.inputs[3]['color_mode'])
    got = rc.infer(shared.device, shared.inputs, components=pk.components.Components(level=0.47, connectivity=26, min_size=3,
                                                                                     select=(track, 0.5)))
    out = got['implicit_output']
    check_result(got, rc.COUNTS, 0.47, connectivity=26, min_size=3, mask=np.ascontiguousarray(out[:, track]), mask_level=0.5)
    rc.same_result(without_components(got), shared.dense)
    # under refine and in track_mode 'all': the components of the array the call returns
    refine = pk.inference.GridRefine(2, 0.46, 1)
    got = rc.infer(shared.device, shared.inputs, refine=refine, components=pk.components.Components(connectivity=18))
    check_result(got, rc.COUNTS, connectivity=18)
    got = rc.infer(shared.device, shared.inputs, track_mode='all', components=pk.components.Components())
    check_result(got, rc.COUNTS)
    rc.same_result(without_components(got), shared.dense_all)
    # the host summary of the call's own table
    counts, mins, spacings = pk.geometry.grid_frame(rc.CASE['num_sample'], shared.inputs[3]['min_z'], shared.inputs[3]['cube_bounds'], 'greater', 4)
    boxes = pk.components.boxes_and_centroids(got['components']['table'], mins, spacings)
    points = got['points_query'][:, :3].astype(np.float64)
    for k in range(len(boxes['size'])):
        mine = points[got['components']['labels'] == k]
        assert len(mine) == boxes['size'][k]
        assert np.allclose(mine.mean(0), boxes['centroid'][k], atol=1e-5) and np.allclose(mine.min(0), boxes['box_min'][k], atol=1e-5) \
            and np.allclose(mine.max(0), boxes['box_max'][k], atol=1e-5)


def check_clip(shared):
    """evaluate_clip(components=..., objects=[]) over two frames: one dict per frame, that of the perform_inference call."""
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = rc.clip_inputs(shared)
    objects = []
    option = pk.components.Components(connectivity=26)
    clip = pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True, components=option, objects=objects)
    dense = pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True)
    assert len(clip) == len(dense) == len(objects) == 2
    for t in range(2):
        for got, want in zip(clip[t], dense[t]):
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        assert objects[t]['labels'].shape == (rc.N_QUERIES,) and (objects[t]['labels'] >= 0).sum() == len(clip[t][2])
        assert objects[t]['table'][:, 0].sum() == len(clip[t][2])
    with pytest.raises(ValueError, match='objects'):
        pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', components=option)


def check_none_is_untouched(shared, monkeypatch):
    """components=None: no new key, the entry points are not called; with components still one host wait."""
    def forbidden(*a, **k):
        raise AssertionError('components=None must not reach the labelling')
    monkeypatch.setattr(pk.ops, 'grid_components', forbidden)
    L = pk._lib.lib()
    for name in SYMBOLS:
        monkeypatch.setattr(L, name, forbidden)
    res = rc.infer(shared.device, shared.inputs, components=None)
    assert 'components' not in res
    rc.same_result(res, shared.dense)
    monkeypatch.undo()
    calls = rc.count_waits(monkeypatch)
    rc.infer(shared.device, shared.inputs, components=pk.components.Components())
    assert calls['wait'] == 1


def check_value_errors(shared):
    option = pk.components.Components()
    with pytest.raises(ValueError, match="components needs point_sample_mode 'grid'"):
        rc.infer(shared.device, shared.inputs, components=option, point_sample_mode='random')
    with pytest.raises(ValueError, match='components must be a components.Components or None'):
        rc.infer(shared.device, shared.inputs, components=0.5)
    with pytest.raises(ValueError, match='by_class=True needs predict_segmentation'):
        rc.infer(shared.device, shared.inputs, components=pk.components.Components(by_class=True))


# ---------------------------------------------------------------------------------------------------------------- a second handle
def run_raw(L, c):
    """The case on HOST arrays through the two entry points of a plain library handle `L` (the g++ twin loaded beside the HIP
    library, never enabled) -> numpy (labels, totals, table of totals[0] rows)."""
    import ctypes
    nx, ny, nz = c['counts']
    n = nx * ny * nz
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    field = np.ascontiguousarray(c['field'], np.float32)
    mask = None if c['mask'] is None else np.ascontiguousarray(c['mask'], np.float32)
    work = np.zeros(pk.ops.components_work_len(n), np.int32)
    labels, totals = np.zeros(n, np.int32), np.zeros(3, np.int32)
    assert L.occ4d_components_label_f32(ptr(field), 1, c['level'], ptr(mask), 1, c['mask_level'], ptr(c['klass']), nx, ny, nz,
                                        c['connectivity'], c['min_size'], ptr(work), ptr(labels), ptr(totals), None) == pk._lib.OK
    table = np.zeros((int(totals[0]), COLS), np.int64)
    assert L.occ4d_components_table_i64(ptr(labels), ptr(c['klass']), nx, ny, nz, ptr(totals), ptr(table), len(table), None) == pk._lib.OK
    return labels, totals, table


def check_by_class(device):
    """by_class on the small CARLA case, which predicts segmentation: the class of a query is the first maximum of its 13 semantic
    columns (the last ones), and the components equal the restatement with those classes; without predict_segmentation: ValueError."""
    import golden_cases as gc
    case = [c for c in gc.INFER_CASES if gc.infer_inputs(c)[3]['predict_segmentation']][0]
    pcl, pa, ia, inf, esd, dsd = gc.infer_inputs(case)
    enc = pk.model.PointCompletionNetV3(**pa).to(device).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).to(device).eval()
    dec.load_state_dict(dsd)
    got = pk.inference.perform_inference(
        pcl.clone(), None, None, [enc, dec], device, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], case['time_idx'], None,
        sample_implicit=True, num_sample=case['num_sample'], point_sample_mode='grid', batch_size=case['batch_size'],
        predict_segmentation=True, track_mode='none', semantic_classes=13, density_threshold=0.5, data_kind=inf['data_kind'],
        cube_mode=4, compress_air=True, components=pk.components.Components(by_class=True, connectivity=26, level=0.45))
    out = got['implicit_output']
    counts = pk.geometry.grid_counts(case['num_sample'], inf['min_z'], inf['cube_bounds'], inf['data_kind'], 4)
    klass = np.argmax(out[:, -13:], axis=1).astype(np.int32)              # (numpy: the first maximum as well)
    labels, totals, table = check_result(got, counts, 0.45, connectivity=26, klass=klass)
    plain = restate_result(got, counts, 0.45, connectivity=26)
    assert totals[1] == plain[1][1] > 0 and totals[0] >= plain[1][0] and set(table[:, 2].tolist()) <= set(range(13))
    return totals, plain[1]
