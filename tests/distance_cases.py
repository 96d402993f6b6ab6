"""Shared by tests/test_distance_host.py (g++ twin) and tests/test_gpu_distance.py (HIP): the yardstick of the distance transform of
the grid's solid set -- two independent restatements of the rules of include/ext/occ4d_distance.h in numpy int64 --, the case matrix,
and the comparison, which is EQUAL everywhere: integers only, no tolerance.

  (a) restate: the STAGED rule by brute force per line -- every candidate of the line, np.argmin = the first minimum = the lower
      axis index --, giving dist2 and nearest;
  (b) brute_dist2: the global minimum of the cost over all sites, for dist2 alone, on grids of at most 4096 points.

TILES.  The launcher of csrc/distance.hip works on tiles of whole lines whose widths ops.distance_tile_width gives; the widths are
IMPORTED from there (never copied): for every width T the launcher has, a grid whose lines select it and whose `inner` extent is
T - 1, T and T + 1, for the y stage (inner = nz) and for the x stage (inner = ny * nz)."""
import functools

import numpy as np
import pytest
import torch

import refine_cases as rc
import occlusions4d_amd as pk

SYMBOLS = ['occ4d_distance_grid_f32']
NONE = 2 ** 31 - 1
MAX_AXIS = 512
CANARY = -0x01234567
NAN = float('nan')
INF64 = np.int64(2) ** 62
ISO, ANISO = (1, 1, 1), (4, 1, 9)
LAST_WEIGHT = 536870911               # on (3, 1, 1): the largest cost is 4 * 536870911 = 2147483644 <= INT32_MAX - 1, and one more is not

GRIDS = [(1, 1, 1), (1, 1, 70), (1, 70, 1), (70, 1, 1), (5, 7, 6), (3, 65, 2), (2, 3, 65), (33, 9, 17), (40, 24, 20), (512, 1, 2)]
BIG = (40, 24, 20)


def tile_widths():
    """{width: the shortest line of >= 3 points the launcher gives that width} over every legal line length, from the launcher."""
    out = {}
    for length in range(3, pk._lib.DISTANCE_CONSTANTS['MAX_AXIS'] + 1):
        out.setdefault(pk.ops.distance_tile_width(length), length)
    return out


WIDTHS = tile_widths()
WIDTH_GRIDS = [g for T, L in sorted(WIDTHS.items()) for inner in (T - 1, T, T + 1) for g in ((2, L, inner), (L, 1, inner))]


# ---------------------------------------------------------------------------------------------------------------- the restatements
def sites_of(field, level, target=0, mask=None, mask_level=0.0):
    with np.errstate(invalid='ignore'):
        m = field >= np.float32(level)                                    # a NaN on either side: False
        if mask is not None:
            m &= mask >= np.float32(mask_level)
    return m if target == 0 else ~m


def restate(field, counts, level, weights=ISO, target=0, mask=None, mask_level=0.0):
    """(a) -> (dist2 (n,) int32, nearest (n,) int32): the stages z, y, x, each one brute force over every line."""
    n = counts[0] * counts[1] * counts[2]
    site = sites_of(field, level, target, mask, mask_level).reshape(counts)
    cost = np.where(site, np.int64(0), INF64)
    near = np.where(site, np.arange(n, dtype=np.int64).reshape(counts), -1)
    for axis in (2, 1, 0):
        idx = np.arange(counts[axis], dtype=np.int64)
        step = np.int64(weights[axis]) * (idx[None, :] - idx[:, None]) ** 2                  # [l, at]
        c, s = np.moveaxis(cost, axis, -1), np.moveaxis(near, axis, -1)
        cand = np.where(c[..., None, :] >= INF64, INF64, c[..., None, :] + step)             # [..., l, at]
        at = np.argmin(cand, axis=-1)                                                         # the first minimum: the lower index
        best = np.take_along_axis(cand, at[..., None], -1)[..., 0]
        who = np.where(best >= INF64, -1, np.take_along_axis(s, at, -1))
        cost, near = np.moveaxis(best, -1, axis), np.moveaxis(who, -1, axis)
    assert cost.min() >= 0 and (cost[cost < INF64] <= NONE - 1).all()
    return np.where(cost >= INF64, NONE, cost).astype(np.int32).reshape(-1), near.astype(np.int32).reshape(-1)


def coords(counts):
    return np.stack(np.meshgrid(*(np.arange(c, dtype=np.int64) for c in counts), indexing='ij'), -1).reshape(-1, 3)


def cost_between(counts, weights, p, q):
    """cost(p, q) of flat indices, int64, elementwise."""
    xyz = coords(counts)
    return (((xyz[p] - xyz[q]) ** 2) * np.asarray(weights, np.int64)).sum(-1)


def brute_dist2(field, counts, level, weights=ISO, target=0, mask=None, mask_level=0.0):
    """(b) -> dist2 (n,) int32: the minimum of the cost over ALL sites."""
    xyz = coords(counts)
    where = xyz[sites_of(field, level, target, mask, mask_level)]
    out = np.full(len(xyz), NONE, np.int64)
    if len(where):
        w = np.asarray(weights, np.int64)
        for lo in range(0, len(xyz), 256):
            out[lo:lo + 256] = (((xyz[lo:lo + 256, None, :] - where[None, :, :]) ** 2) * w).sum(-1).min(1)
    return out.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- the matrix
def case(name, counts, field, level=0.5, weights=ISO, target=0, mask=None, mask_level=0.5, wide=False, nearest=True):
    return dict(name=name, counts=counts, field=np.ascontiguousarray(field, np.float32), level=level, weights=weights, target=target,
                mask=None if mask is None else np.ascontiguousarray(mask, np.float32), mask_level=mask_level, wide=wide, nearest=nearest)


def random_field(n, seed):
    """Uniform values in [0, 1): the fraction d lies at or above level 1 - d."""
    return np.random.default_rng(seed).random(n, dtype=np.float32)


def corner_field(counts, k):
    f = np.zeros(counts, np.float32)
    f[tuple((c - 1) if (k >> (2 - a)) & 1 else 0 for a, c in enumerate(counts))] = 1.0
    return f.reshape(-1)


def _cases():
    out = []
    for counts in GRIDS:
        n = counts[0] * counts[1] * counts[2]
        g = '%dx%dx%d' % counts
        for k in range(8):                                                # one site in each of the eight corners in turn
            out.append(case('%s-corner%d' % (g, k), counts, corner_field(counts, k), weights=ANISO if k % 2 else ISO))
        for target in (0, 1):
            for weights in (ISO, ANISO):
                tag = '-t%d-w%d%d%d' % ((target,) + weights)
                out.append(case(g + '-air' + tag, counts, np.zeros(n), weights=weights, target=target))       # target 0: no site at all
                out.append(case(g + '-solid' + tag, counts, np.ones(n), weights=weights, target=target))      # target 1: no site at all
                out.append(case(g + '-random2' + tag, counts, random_field(n, 21), level=0.98, weights=weights, target=target))
                out.append(case(g + '-random30' + tag, counts, random_field(n, 22), level=0.7, weights=weights, target=target))
                out.append(case(g + '-level-nan' + tag, counts, np.ones(n), level=NAN, weights=weights, target=target))
                out.append(case(g + '-mask' + tag, counts, random_field(n, 23), level=0.4, weights=weights, target=target,
                                mask=random_field(n, 24), mask_level=0.8))
        out.append(case(g + '-random30-dist2-only', counts, random_field(n, 22), level=0.7, nearest=False))
        out.append(case(g + '-mask-dist2-only', counts, random_field(n, 23), level=0.4, weights=ANISO, target=1, mask=random_field(n, 24),
                        mask_level=0.8, nearest=False))
        out.append(case(g + '-wide', counts, random_field(n, 25), level=0.9, weights=ANISO, mask=random_field(n, 26), mask_level=0.2,
                        wide=True))
        out.append(case(g + '-wide-t1', counts, random_field(n, 25), level=0.1, target=1, wide=True))
    for counts in WIDTH_GRIDS:
        n = counts[0] * counts[1] * counts[2]
        g = '%dx%dx%d' % counts
        out.append(case(g + '-random2', counts, random_field(n, 27), level=0.98, weights=ANISO))
        out.append(case(g + '-random30-t1', counts, random_field(n, 28), level=0.7, target=1))
        out.append(case(g + '-last-corner', counts, corner_field(counts, 7), nearest=False))
    for k, field in enumerate(([1, 0, 0], [0, 0, 1], [0, 1, 0])):          # the last legal weight: costs up to 2147483644
        for target in (0, 1):
            out.append(case('3x1x1-last-weight-%d-t%d' % (k, target), (3, 1, 1), np.array(field), weights=(LAST_WEIGHT, 1, 1), target=target))
    return out


CASES = _cases()
NAMES = [c['name'] for c in CASES]
BY_NAME = dict(zip(NAMES, CASES))
assert len(BY_NAME) == len(CASES)
RANDOM_BIG = [n for n in NAMES if n.startswith('40x24x20-random')]


def _rules(c):
    return c['field'], c['counts'], c['level'], c['weights'], c['target'], c['mask'], c['mask_level']


@functools.lru_cache(maxsize=None)
def expected(name):
    """Restatement (a) of a case, computed once per process; the arrays are read-only."""
    got = restate(*_rules(BY_NAME[name]))
    for a in got:
        a.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def expected_global(name):
    """Restatement (b), or None on a grid of more than 4096 points."""
    c = BY_NAME[name]
    if c['counts'][0] * c['counts'][1] * c['counts'][2] > 4096:
        return None
    got = brute_dist2(*_rules(c))
    got.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def expected_scipy(name):
    """rint(scipy's Euclidean distance transform squared), or None: without scipy, with other weights, or with no site."""
    c = BY_NAME[name]
    site = sites_of(c['field'], c['level'], c['target'], c['mask'], c['mask_level'])
    if c['weights'] != ISO or not site.any():
        return None
    try:
        from scipy import ndimage
    except ImportError:
        return None
    got = np.rint(ndimage.distance_transform_edt(~site.reshape(c['counts'])) ** 2).astype(np.int64).reshape(-1)
    got.setflags(write=False)
    return got


# ---------------------------------------------------------------------------------------------------------------- the comparison
def run(c, device):
    """The case through ops.grid_distance into buffers of n + 1 words -> numpy (dist2 buffer, nearest buffer or None)."""
    n = c['counts'][0] * c['counts'][1] * c['counts'][2]
    if c['wide']:                                                         # the field and the mask as columns 2 and 4 of an (n, 5) array
        wide = np.full((n, 5), 7.0, np.float32)
        wide[:, 2] = c['field']
        wide[:, 4] = 1.0 if c['mask'] is None else c['mask']
        wide = torch.from_numpy(wide).to(device)
        values, mask = wide[:, 2], (None if c['mask'] is None else wide[:, 4])
    else:
        values = torch.from_numpy(c['field']).to(device)
        mask = None if c['mask'] is None else torch.from_numpy(c['mask']).to(device)
    bufs = (torch.full((n + 1,), CANARY, dtype=torch.int32, device=device),
            torch.full((n + 1,), CANARY, dtype=torch.int32, device=device) if c['nearest'] else None)
    dist2, nearest = pk.ops.grid_distance(values, c['counts'], c['level'], c['weights'], c['target'], mask, c['mask_level'],
                                          nearest=c['nearest'], out=bufs)
    assert dist2.data_ptr() == bufs[0].data_ptr() and dist2.shape == (n,) and (nearest is None) == (not c['nearest'])
    return bufs[0].cpu().numpy(), None if bufs[1] is None else bufs[1].cpu().numpy()


def same(got, name):
    """A run's buffers against the REQUIRED RESULTS: equal to (a), and to (b) and to scipy where they apply; nearest[p] a site at
    cost dist2[p], or -1 where dist2 is NONE; the canary word behind each output untouched."""
    c = BY_NAME[name]
    n = c['counts'][0] * c['counts'][1] * c['counts'][2]
    want_dist2, want_nearest = expected(name)
    dist2, canary = got[0][:n], got[0][n:]
    assert dist2.dtype == np.int32 and canary.tolist() == [CANARY], name
    assert np.array_equal(dist2, want_dist2), name
    for other in (expected_global(name), expected_scipy(name)):
        assert other is None or np.array_equal(dist2, other), name
    if not c['nearest']:
        return got[1] is None
    nearest, canary = got[1][:n], got[1][n:]
    assert nearest.dtype == np.int32 and canary.tolist() == [CANARY], name
    assert np.array_equal(nearest, want_nearest), name
    site = sites_of(c['field'], c['level'], c['target'], c['mask'], c['mask_level'])
    has = dist2 != NONE
    assert (nearest[~has] == -1).all() and has.all() == site.any() and (has.all() or not has.any()), name
    if has.any():
        assert nearest.min() >= 0 and nearest.max() < n and site[nearest].all(), name
        assert np.array_equal(cost_between(c['counts'], c['weights'], np.arange(n), nearest.astype(np.int64)), dist2.astype(np.int64)), name
    return True


def check(name, device):
    assert same(run(BY_NAME[name], device), name), name


def check_by_hand():
    """The restatement itself on cases worked by hand, and what the patterns of the matrix are there for."""
    # midway between two sites on one axis: the lower index wins
    dist2, nearest = restate(np.array([0, 1, 0, 1, 0], np.float32), (1, 1, 5), 0.5)
    assert dist2.tolist() == [1, 0, 1, 0, 1] and nearest.tolist() == [1, 1, 1, 3, 3]
    # a tie of the y stage between lines with different z costs: (1, 4, 3), sites (iy 1, iz 2) = 5 and (iy 3, iz 0) = 9.  For the
    # point (1, 0) = 3 its own line's entry costs 4 + 0 and the line iy = 3 costs 0 + 4: the lower j = 1 wins, the site is 5.
    field = np.zeros(12, np.float32)
    field[[5, 9]] = 1.0
    dist2, nearest = restate(field, (1, 4, 3), 0.5)
    assert dist2[3] == 4 and nearest[3] == 5 and nearest[9] == 9 and nearest[0] == 5 and dist2[0] == 5
    assert np.array_equal(dist2, brute_dist2(field, (1, 4, 3), 0.5))
    # weights under which the nearest site is another one: (1, 3, 2), sites (iy 0, iz 1) = 1 and (iy 2, iz 0) = 4, seen from point 0
    field = np.array([0, 1, 0, 0, 1, 0], np.float32)
    iso, aniso = restate(field, (1, 3, 2), 0.5), restate(field, (1, 3, 2), 0.5, ANISO)
    assert (iso[0][0], iso[1][0]) == (1, 1) and (aniso[0][0], aniso[1][0]) == (4, 4)
    # target 1 is the depth inside; NaN is no member
    dist2, nearest = restate(np.array([1, 1, 1, 0, NAN], np.float32), (1, 1, 5), 0.5, target=1)
    assert dist2.tolist() == [9, 4, 1, 0, 0] and nearest.tolist() == [3, 3, 3, 3, 4]
    for counts in GRIDS:
        g = '%dx%dx%d' % counts
        n = counts[0] * counts[1] * counts[2]
        for name in (g + '-air-t0-w111', g + '-solid-t1-w419', g + '-level-nan-t0-w419'):
            assert (expected(name)[0] == NONE).all() and (expected(name)[1] == -1).all(), name
        for name in (g + '-solid-t0-w111', g + '-air-t1-w419', g + '-level-nan-t1-w111'):
            assert (expected(name)[0] == 0).all() and np.array_equal(expected(name)[1], np.arange(n)), name
        far = [int(expected('%s-corner%d' % (g, k))[0].max()) for k in range(8)]
        assert far[0] == far[6] == sum((c - 1) ** 2 for c in counts) and far[1] == far[7] == sum(w * (c - 1) ** 2 for w, c in zip(ANISO, counts))
    assert expected('3x1x1-last-weight-0-t0')[0].tolist() == [0, LAST_WEIGHT, 4 * LAST_WEIGHT] and 4 * LAST_WEIGHT == NONE - 3
    assert expected('3x1x1-last-weight-2-t0')[1].tolist() == [1, 1, 1] and expected('3x1x1-last-weight-2-t1')[1].tolist() == [0, 0, 2]
    assert sorted(WIDTHS) == sorted(set(WIDTHS)) and max(WIDTHS) == pk._lib.DISTANCE_CONSTANTS['TILE_WIDTH'] and len(WIDTHS) >= 2
    assert all(L * T <= pk._lib.DISTANCE_CONSTANTS['TILE_POINTS'] for T, L in WIDTHS.items()) and len(WIDTH_GRIDS) == 6 * len(WIDTHS)


# ---------------------------------------------------------------------------------------------------------------- the rejected calls
def check_argument_errors(device):
    """ops.grid_distance: rejected arguments raise AssertionError with the library's text (the table of both libraries' texts is
    tests/test_gpu_distance_contract_texts.py); an empty grid is a no-op."""
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=device)
    call = lambda **k: pk.ops.grid_distance(**dict(dict(values=z(30), counts=(3, 2, 5), level=0.5), **k))
    for kw, text in ((dict(weights=(1, 0, 1)), 'wx = 1, wy = 0, wz = 1 must be >= 1'), (dict(weights=(-4, 1, 1)), 'wx = -4, wy = 1, wz = 1 must be >= 1'),
                     (dict(target=2), 'target = 2 must be 0 or 1'), (dict(counts=(-3, -2, 5)), 'nx = -3, ny = -2, nz = 5 must be >= 0'),
                     (dict(values=z(513), counts=(1, 513, 1)), 'nx = 1, ny = 513, nz = 1 must be <= 512'),
                     (dict(values=z(3), counts=(3, 1, 1), weights=(LAST_WEIGHT + 1, 1, 1)), 'the largest cost 2147483648 = 536870912'),
                     (dict(values=z(29)), r'values must be \(30,\)'), (dict(mask=z(31)), r'mask must be \(30,\)'),
                     (dict(out=(z(29, dtype=torch.int32), None)), 'out dist2 must be a contiguous'),
                     (dict(out=(z(30), None)), 'out dist2 must be torch.int32'),
                     (dict(nearest=True, out=(z(30, dtype=torch.int32), z(60, dtype=torch.int32)[::2])), 'out nearest must be a contiguous'),
                     (dict(out=(z(30, dtype=torch.int32), z(30, dtype=torch.int32))), 'without nearest=True')):
        with pytest.raises(AssertionError, match=text):
            call(**kw)
    for counts in ((0, 2, 5), (3, 0, 0)):
        dist2, nearest = call(values=z(0), counts=counts, nearest=True)
        assert dist2.shape == (0,) and nearest.shape == (0,) and dist2.dtype == torch.int32
    dist2, nearest = call(values=z(30) + 1)
    assert nearest is None and dist2.tolist() == [0] * 30


# ---------------------------------------------------------------------------------------------------------------- end to end
KEYS = ('clearance', 'components')


def without(result):
    return {k: v for k, v in result.items() if k not in KEYS}


def check_result(got, counts, option, level=0.5, **kw):
    """result['clearance'] against the restatement run over the returned implicit_output's density column."""
    field = np.ascontiguousarray(got['implicit_output'][:, 0])
    c = got['clearance']
    assert sorted(c) == sorted(['dist2'] + ['nearest'] * option.nearest + ['inside2'] * option.inside)
    assert all(isinstance(a, np.ndarray) and a.dtype == np.int32 and a.shape == (len(field),) for a in c.values())
    dist2, nearest = restate(field, counts, level, option.weights, 0, **kw)
    assert np.array_equal(c['dist2'], dist2)
    if option.nearest:
        assert np.array_equal(c['nearest'], nearest)
    if option.inside:
        assert np.array_equal(c['inside2'], restate(field, counts, level, option.weights, 1, **kw)[0])
    return dist2, nearest


def check_end_to_end(shared):
    option = pk.distance.Clearance(nearest=True, inside=True)
    got = rc.infer(shared.device, shared.inputs, clearance=option, components=pk.components.Components())
    dist2, nearest = check_result(got, rc.COUNTS, option)
    solid = got['implicit_output'][:, 0] >= np.float32(0.5)
    assert 0 < solid.sum() < len(solid) and ((dist2 == 0) == solid).all() and ((got['clearance']['inside2'] == 0) == ~solid).all()
    rc.same_result(without(got), shared.dense)
    # the Voronoi regions of the call's own components: the restatement's gather
    labels = got['components']['labels']
    regions = pk.distance.expand_labels(torch.from_numpy(labels), torch.from_numpy(got['clearance']['nearest']))
    assert regions.dtype == torch.int32 and np.array_equal(regions.numpy(), np.where(nearest >= 0, labels[np.maximum(nearest, 0)], -1))
    assert (regions.numpy() >= 0).all() and np.array_equal(regions.numpy()[solid], labels[solid])
    # the metric and the sign of the call's own arrays
    sdf = pk.distance.signed(torch.from_numpy(got['clearance']['dist2']), torch.from_numpy(got['clearance']['inside2']), 0.25).numpy()
    assert ((sdf < 0) == solid).all() and np.isfinite(sdf).all()
    # the options: level, weights, select; dist2 alone
    track = pk.inference.get_track_idx(shared.inputs[3]['color_mode'])
    option = pk.distance.Clearance(level=0.47, weights=ANISO, select=(track, 0.5), inside=True)
    got = rc.infer(shared.device, shared.inputs, clearance=option)
    check_result(got, rc.COUNTS, option, 0.47, mask=np.ascontiguousarray(got['implicit_output'][:, track]), mask_level=0.5)
    rc.same_result(without(got), shared.dense)
    # under refine and in track_mode 'all': the transform of the array the call returns
    option = pk.distance.Clearance(nearest=True)
    got = rc.infer(shared.device, shared.inputs, refine=pk.inference.GridRefine(2, 0.46, 1), clearance=option)
    check_result(got, rc.COUNTS, option)
    got = rc.infer(shared.device, shared.inputs, track_mode='all', clearance=option)
    check_result(got, rc.COUNTS, option)
    rc.same_result(without(got), shared.dense_all)


def check_clip(shared):
    """evaluate_clip(clearance=..., clearances=[]) over two frames: one dict per frame, that of the perform_inference call."""
    pcl, sem, target, inf, enc, dec = shared.inputs
    frames, batch, args = rc.clip_inputs(shared)
    clearances = []
    option = pk.distance.Clearance(nearest=True)
    clip = pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True, clearance=option, clearances=clearances)
    dense = pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', save_gt=True)
    assert len(clip) == len(dense) == len(clearances) == 2
    for t in range(2):
        for got, want in zip(clip[t], dense[t]):
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        assert sorted(clearances[t]) == ['dist2', 'nearest'] and clearances[t]['dist2'].shape == (rc.N_QUERIES,)
        assert (clearances[t]['dist2'] == 0).sum() == len(clip[t][2])                       # the solid rows
    with pytest.raises(ValueError, match='clearances'):
        pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', clearance=option)
    with pytest.raises(ValueError, match='clearance must be a distance.Clearance'):
        pk.evaluation.evaluate_clip(batch, [enc, dec], shared.device, args, 'greater', clearance=0.5, clearances=[])


def check_none_is_untouched(shared, monkeypatch):
    """clearance=None: no new key, the entry point is not called; with a clearance still one host wait."""
    def forbidden(*a, **k):
        raise AssertionError('clearance=None must not reach the distance transform')
    monkeypatch.setattr(pk.ops, 'grid_distance', forbidden)
    L = pk._lib.lib()
    for name in SYMBOLS:
        monkeypatch.setattr(L, name, forbidden)
    res = rc.infer(shared.device, shared.inputs, clearance=None)
    assert 'clearance' not in res
    rc.same_result(res, shared.dense)
    monkeypatch.undo()
    calls = rc.count_waits(monkeypatch)
    rc.infer(shared.device, shared.inputs, clearance=pk.distance.Clearance(nearest=True, inside=True))
    assert calls['wait'] == 1


def check_value_errors(shared):
    option = pk.distance.Clearance()
    with pytest.raises(ValueError, match="clearance needs point_sample_mode 'grid'"):
        rc.infer(shared.device, shared.inputs, clearance=option, point_sample_mode='random')
    with pytest.raises(ValueError, match='clearance must be a distance.Clearance or None'):
        rc.infer(shared.device, shared.inputs, clearance=0.5)
    with pytest.raises(ValueError, match='clearance must be a distance.Clearance or None'):
        rc.infer(shared.device, shared.inputs, clearance=pk.components.Components())


# ---------------------------------------------------------------------------------------------------------------- a second handle
def run_raw(L, c):
    """The case on HOST arrays through the entry point of a plain library handle `L` (the g++ twin loaded beside the HIP library,
    never enabled) -> numpy (dist2 buffer, nearest buffer or None), n + 1 words each as run() returns them."""
    import ctypes
    nx, ny, nz = c['counts']
    n = nx * ny * nz
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    dist2 = np.full(n + 1, CANARY, np.int32)
    nearest = np.full(n + 1, CANARY, np.int32) if c['nearest'] else None
    assert L.occ4d_distance_grid_f32(ptr(c['field']), 1, c['level'], ptr(c['mask']), 1, c['mask_level'], c['target'], nx, ny, nz,
                                     *c['weights'], ptr(dist2), ptr(nearest), None) == pk._lib.OK
    return dist2, nearest
