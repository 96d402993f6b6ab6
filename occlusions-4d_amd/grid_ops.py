"""Tensor-level wrappers of the grid products (include/occ4d_surface.h aside, the headers of include/ext/): what turns the decoded
occupancy of a (nx, ny, nz) grid into more device tensors -- views, components, links, clearance, routes, segments, sight,
waypoints, next views, boxes, layers.  ops.py re-exports every name: callers use ops.<name>, looked up at call time."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._plumbing import _dev, _inst_column, _int32_out, _merge_rows, _ptr, _rows, _stream


def _grid(counts):
    """(nx, ny, nz, nx * ny * nz) of the grid `counts`.  The product is NOT clamped: a wrapper whose shapes need max(n, 0) for the
    counts the library rejects says so itself."""
    nx, ny, nz = (int(c) for c in counts)
    return nx, ny, nz, nx * ny * nz


def _contiguous(t):
    """`t` itself when it is contiguous, else a contiguous copy."""
    return t if t.is_contiguous() else t.contiguous()


def _bit_words(bits, n, name):
    """The contiguous (ceil(n / 32),) int32 words of ops.grid_solid_bits / ops.grid_blocked_bits for n grid points."""
    words = _dev(bits, torch.int32, name)
    assert words.dim() == 1 and words.shape[0] == (max(n, 0) + 31) // 32 and words.is_contiguous(), \
        '%s must be a contiguous (%d,) tensor, got %s' % (name, (max(n, 0) + 31) // 32, tuple(words.shape))
    return words


def _outs(out, count):
    """The caller's `out` tuple of `count` buffers, all None when there is none."""
    return (None,) * count if out is None else out


def _capped_table(cap, totals, n, device, table=None):
    """(cap, the (>= cap, COLS) int64 components table): cap=None is one device->host read of totals[0] (none on an empty grid); a
    caller's `table` needs a cap and is checked, else a new one of cap rows."""
    cols = _lib.COMPONENTS_CONSTANTS['COLS']
    if cap is None:
        assert table is None, 'a caller\'s table needs cap'
        cap = int(totals.tolist()[0]) if n else 0
    cap = int(cap)
    assert cap >= 0, 'cap = %d must be >= 0' % cap
    if table is None:
        table = torch.empty((cap, cols), dtype=torch.int64, device=device)
    else:
        table = _dev(table, torch.int64, 'table')
        assert table.dim() == 2 and table.shape[1] == cols and table.shape[0] >= cap and table.is_contiguous(), \
            'table must be a contiguous (>= %d, %d) tensor, got %s' % (cap, cols, tuple(table.shape))
    return cap, table


def raycast_grid(values, counts, mins, spacings, level, rt_inv, k_inv, height, width, near, step, n_steps, attrs=None, channels=(),
                 background=0.0, feature_background=None):
    """The field `values` on the (nx, ny, nz) = `counts` grid ray-cast into V views (occ4d_raycast_grid_f32, the rules in
    include/ext/occ4d_raycast.h): per pixel the first of the n_steps samples at depths near + i * step whose trilinear value is
    >= level, refined against the sample before it.  values (n,): one value per grid point, x slowest, z fastest (a strided
    column view is read in place); mins / spacings: the three floats each that ops.grid_points took for this grid; rt_inv,
    k_inv (V, 16) or (V, 4, 4): the INVERSES of the expanded camera matrices.  attrs (n, d) and `channels`: the columns
    sampled at the hit.  -> (depth (V, H, W) fp32, `background` where nothing is hit; cell (V, H, W) int32, the flat index of
    the hit cell's low corner or -1; features (V, H, W, C), `feature_background` (default: `background`) where nothing is hit),
    on the device.  No host read."""
    nx, ny, nz, n = _grid(counts)
    v = _dev(values, name='values')
    assert v.dim() == 1 and v.shape[0] == n, 'values must be (%d,), got %s' % (n, tuple(v.shape))
    rt, k = _dev(rt_inv, name='rt_inv'), _dev(k_inv, name='k_inv')
    V = rt.shape[0] if rt.dim() else -1
    assert rt.dim() in (2, 3) and rt.numel() == V * 16 and tuple(k.shape) == tuple(rt.shape), \
        'rt_inv / k_inv must both be (V, 16) or (V, 4, 4), got %s and %s' % (tuple(rt.shape), tuple(k.shape))
    rt, k = rt.contiguous(), k.contiguous()
    H, W = int(height), int(width)
    cols = [int(c) for c in channels]
    n_ch = len(cols)
    a, ld_attr, d = None, 0, 0
    if n_ch:
        assert attrs is not None, 'channels need attrs'
        a, ld_attr = _merge_rows(attrs, 'attrs')
        assert a.shape[0] == n, 'attrs must hold %d rows, got %d' % (n, a.shape[0])
        d = a.shape[1]
    depth = torch.empty((V, H, W), dtype=torch.float32, device=v.device)
    cell = torch.empty((V, H, W), dtype=torch.int32, device=v.device)
    feat = torch.empty((V, H, W, n_ch), dtype=torch.float32, device=v.device)
    arr = (C.c_int32 * n_ch)(*cols) if n_ch else None
    fbg = background if feature_background is None else feature_background
    _lib.check(_lib.lib().occ4d_raycast_grid_f32(
        _ptr(v), v.stride(0) if n > 1 else 1, nx, ny, nz, float(mins[0]), float(spacings[0]), float(mins[1]), float(spacings[1]),
        float(mins[2]), float(spacings[2]), float(level), _ptr(k), _ptr(rt), V, H, W, float(near), float(step), int(n_steps), _ptr(a),
        max(ld_attr, d), d, arr, n_ch, float(background), float(fbg), _ptr(depth), _ptr(cell), _ptr(feat) if n_ch else None, _stream()))
    return depth, cell, feat


def components_work_len(n):
    """Elements of the int32 work array of occ4d_components_label_f32 for n grid points (the formula of the header)."""
    tile = _lib.COMPONENTS_CONSTANTS['TILE']
    return 3 * n + 3 * ((n + tile - 1) // tile)


def grid_components(values, counts, level, connectivity=6, min_size=1, mask=None, mask_level=0.0, klass=None, cap=None, table=None):
    """The connected components of the set values >= level of the (nx, ny, nz) = `counts` grid (occ4d_components_label_f32 /
    occ4d_components_table_i64, the rules in include/ext/occ4d_components.h).  values (n,): one value per grid point, x slowest,
    z fastest (a strided column view is read in place); mask (n,) with mask_level: a second such column, members also need
    mask >= mask_level; klass (n,) int32: members need klass >= 0 and neighbours equal classes.  Components of fewer than min_size
    points are dropped, the others numbered in the order of their lowest flat index.
    -> (labels (n,) int32, -1 = none; totals (3,) int32: kept components, kept points, all components; table (K, 12) int64, one row
    per kept component), on the device.  cap=None: one 12-byte device->host read of totals sizes the table, K = totals[0].  cap = an
    int: no read, K = cap, and only the rows below min(cap, totals[0]) are written.  `table`: a caller's contiguous int64 (>= K, 12)
    buffer whose first K rows are used (cap required)."""
    nx, ny, nz, n = _grid(counts)
    v, ld = _inst_column(values, n, 'values')
    m, ld_mask = (None, 0) if mask is None else _inst_column(mask, n, 'mask')
    kl = None
    if klass is not None:
        kl = _dev(klass, torch.int32, 'klass')
        assert tuple(kl.shape) == (n,) and kl.is_contiguous(), 'klass must be a contiguous (%d,) tensor, got %s' % (n, tuple(kl.shape))
    connectivity, min_size = int(connectivity), int(min_size)
    # (an empty grid is a no-op of the library: its totals are the zeros put here)
    scratch = (torch.empty if n else torch.zeros)(components_work_len(n) + 3, dtype=torch.int32, device=v.device)
    work, totals = scratch[:-3], scratch[-3:]
    labels = torch.empty((n,), dtype=torch.int32, device=v.device)
    st = _stream()
    _lib.check(_lib.lib().occ4d_components_label_f32(_ptr(v), ld, float(level), _ptr(m), ld_mask, float(mask_level), _ptr(kl), nx, ny, nz,
                                                     connectivity, min_size, _ptr(work), _ptr(labels), _ptr(totals), st))
    cap, table = _capped_table(cap, totals, n, v.device, table)
    _lib.check(_lib.lib().occ4d_components_table_i64(_ptr(labels), _ptr(kl), nx, ny, nz, _ptr(totals), _ptr(table), cap, st))
    return labels, totals, table[:cap]


def watershed_work_len(n):
    """Elements of the int32 work array of occ4d_watershed_label_i32 for n grid points (the formula of the header)."""
    k = _lib.WATERSHED_CONSTANTS
    return 4 * n + 4 * ((n + k['TILE'] - 1) // k['TILE']) + k['ROUND_WORDS']


def grid_watershed(height, counts, h, connectivity=26, min_size=1, cap=None):
    """The watershed segments of an integer height map on the (nx, ny, nz) = `counts` grid (occ4d_watershed_label_i32 /
    occ4d_components_table_i64 / occ4d_watershed_peaks_i32, the rules in include/ext/occ4d_watershed.h).  height (n,) int32, x
    slowest, z fastest: the members are height >= 1 (ops.grid_distance's inside2 with target=1: the squared depth of every solid
    point).  Every member climbs to its highest neighbour -- ties to the lower flat index -- until a maximum; two basins merge when
    the highest saddle between them lies within `h` (an integer in [0, 2^31 - 1]) of the lower peak.  Segments of fewer than
    min_size points are dropped, the others numbered in the order of their lowest flat index.
    -> (labels (n,) int32, -1 = none; totals (4,) int32: kept segments, kept points, all segments, basins; table (K, 12) int64, the
    components table of the segments; peaks (K, 2) int32: per kept segment the flat index and the height of its highest point), on
    the device.  cap=None: one 16-byte device->host read of totals sizes table and peaks, K = totals[0].  cap = an int: no read, K =
    cap, and only the rows below min(cap, totals[0]) are written."""
    nx, ny, nz, n = _grid(counts)
    n = max(n, 0)
    hgt, _ = _inst_column(height, n, 'height', torch.int32)
    hgt = _contiguous(hgt)
    words = _lib.WATERSHED_CONSTANTS['TOTALS']
    # (an empty grid is a no-op of the library: its totals are the zeros put here)
    scratch = (torch.empty if n else torch.zeros)(watershed_work_len(n) + words, dtype=torch.int32, device=hgt.device)
    work, totals = scratch[:-words], scratch[-words:]
    labels = torch.empty((n,), dtype=torch.int32, device=hgt.device)
    st = _stream()
    _lib.check(_lib.lib().occ4d_watershed_label_i32(_ptr(hgt), nx, ny, nz, int(connectivity), int(h), int(min_size), _ptr(work),
                                                    _ptr(labels), _ptr(totals), st))
    cap, table = _capped_table(cap, totals, n, hgt.device)
    peaks = torch.empty((cap, 2), dtype=torch.int32, device=hgt.device)
    _lib.check(_lib.lib().occ4d_components_table_i64(_ptr(labels), None, nx, ny, nz, _ptr(totals), _ptr(table), cap, st))
    _lib.check(_lib.lib().occ4d_watershed_peaks_i32(_ptr(hgt), _ptr(labels), n, _ptr(totals), _ptr(peaks), cap, st))
    return labels, totals, table, peaks


def grid_solid_bits(values, level, mask=None, mask_level=0.0):
    """The solid set values >= level (with mask (n,) also mask >= mask_level) packed one bit per grid point (occ4d_sight_bits_f32,
    the rules in include/ext/occ4d_sight.h): values (n,), a strided column view is read in place -> (ceil(n / 32),) int32 on the
    device, bit p % 32 of word p // 32 is point p, the unused bits of the last word are 0.  No host read."""
    n = int(values.shape[0])
    v, ld = _inst_column(values, n, 'values')
    m, ld_mask = (None, 0) if mask is None else _inst_column(mask, n, 'mask')
    bits = torch.empty(((n + 31) // 32,), dtype=torch.int32, device=v.device)
    _lib.check(_lib.lib().occ4d_sight_bits_f32(_ptr(v), ld, float(level), _ptr(m), ld_mask, float(mask_level), n, _ptr(bits), _stream()))
    return bits


def grid_sight(bits, counts, origins, framed=None, blocker=False, flags=0):
    """Line of sight on the (nx, ny, nz) = `counts` grid (occ4d_sight_grid_u32, the rules in include/ext/occ4d_sight.h): bits
    (ceil(n / 32),) int32 from ops.grid_solid_bits; origins (V, 3) integer lattice points ON THE HOST (numpy or a list), 1 <= V <=
    31, inside the grid or not; framed (n,) int32 or None: bit v = origin v may look at the query; blocker: also the blocking cells;
    flags: 0 (the header has no flag bit).  -> (seen (n,) int32, bit v = seen from origin v; blocker (V, n) int32, -1
    where seen or not framed, or None), on the device.  No host read."""
    nx, ny, nz, n = _grid(counts)
    words = _bit_words(bits, n, 'bits')
    org = np.ascontiguousarray(origins, dtype=np.int64)
    assert org.ndim == 2 and org.shape[1] == 3, 'origins must be (V, 3), got %s' % (org.shape,)
    assert org.size == 0 or (org.min() >= -2 ** 31 and org.max() <= 2 ** 31 - 1), 'origins must fit int32'
    org = org.astype(np.int32)
    V = org.shape[0]
    fr = None if framed is None else _dev(framed, torch.int32, 'framed')
    assert fr is None or (tuple(fr.shape) == (max(n, 0),) and fr.is_contiguous()), 'framed must be a contiguous (%d,) tensor' % n
    seen = torch.empty((max(n, 0),), dtype=torch.int32, device=words.device)
    block = torch.empty((max(V, 0), max(n, 0)), dtype=torch.int32, device=words.device) if blocker else None
    _lib.check(_lib.lib().occ4d_sight_grid_u32(_ptr(words), nx, ny, nz, org.ctypes.data_as(C.c_void_p), V, _ptr(fr), _ptr(seen),
                                               _ptr(block), int(flags), _stream()))
    return seen, block


def distance_tile_width(length, stage=1):
    """Lines of a workgroup's tile in the launcher of occ4d_distance_grid_f32 for lines of `length` points (the formulas of the
    header's constants): stage 0 (z) max(1, RUN_POINTS // length) consecutive lines; stages 1, 2 (y, x) TILE_WIDTH halved until
    length * width <= TILE_POINTS."""
    k = _lib.DISTANCE_CONSTANTS
    if stage == 0:
        return max(1, k['RUN_POINTS'] // length)
    width = k['TILE_WIDTH']
    while width > 1 and width * length > k['TILE_POINTS']:
        width //= 2
    return width


def grid_distance(values, counts, level, weights=(1, 1, 1), target=0, mask=None, mask_level=0.0, nearest=False, out=None):
    """The exact squared Euclidean distance of every point of the (nx, ny, nz) = `counts` grid to the nearest SITE
    (occ4d_distance_grid_f32, the rules in include/ext/occ4d_distance.h).  values (n,): one value per grid point, x slowest, z
    fastest (a strided column view is read in place); the members are values >= level, with mask (n,) also mask >= mask_level.
    target 0: the members are the sites; 1: the non-members.  weights = (wx, wy, wz): integers >= 1, the cost of a step along each
    axis is its weight times the squared number of points.  nearest: also the flat index of the site.
    `out` = (dist2, nearest or None): the caller's contiguous int32 buffers of >= n elements, whose first n are used.
    -> (dist2 (n,) int32, DISTANCE_CONSTANTS['NONE'] where there is no site; nearest (n,) int32, -1 there, or None), on the device.
    No host read."""
    nx, ny, nz, n = _grid(counts)
    v, ld = _inst_column(values, n, 'values')
    m, ld_mask = (None, 0) if mask is None else _inst_column(mask, n, 'mask')
    wx, wy, wz = (int(w) for w in weights)
    bufs = []
    for i, (name, wanted) in enumerate((('dist2', True), ('nearest', bool(nearest)))):
        buf = None if out is None else out[i]
        if not wanted:
            assert buf is None, 'out holds a nearest buffer without nearest=True'
        elif buf is None:
            buf = torch.empty((max(n, 0),), dtype=torch.int32, device=v.device)
        else:
            buf = _dev(buf, torch.int32, 'out ' + name)
            assert buf.dim() == 1 and buf.shape[0] >= n and buf.is_contiguous(), \
                'out %s must be a contiguous (>= %d,) tensor, got %s' % (name, n, tuple(buf.shape))
        bufs.append(buf)
    _lib.check(_lib.lib().occ4d_distance_grid_f32(_ptr(v), ld, float(level), _ptr(m), ld_mask, float(mask_level), int(target), nx, ny, nz,
                                                  wx, wy, wz, _ptr(bufs[0]), _ptr(bufs[1]), _stream()))
    return bufs[0][:max(n, 0)], None if bufs[1] is None else bufs[1][:max(n, 0)]


def geodesic_default_rounds(counts):
    """The default number of relaxation rounds of ops.grid_geodesic on a (nx, ny, nz) grid: twice the sum of the tile counts along
    the three axes (the tile shape is the header's), 64 at 96 x 96 x 58.  A heuristic: status[0] says whether it was enough."""
    k = _lib.GEODESIC_CONSTANTS
    return 2 * sum(-(-int(c) // k[t]) for c, t in zip(counts, ('TILE_X', 'TILE_Y', 'TILE_Z')))


def geodesic_work_len(rounds):
    """Elements of the int32 work array of occ4d_geodesic_grid_i32 for `rounds` rounds (the formula of the header): one word per
    round and one in front."""
    return int(rounds) + 1


def grid_geodesic(clear, counts, seeds, min_clear=1, connectivity=26, steps=(3, 4, 5), rounds=None, parent=False, resume=None,
                  out=None, work=None):
    """The least total step cost of a path from any seed to every point of the (nx, ny, nz) = `counts` grid that stays on passable
    points (occ4d_geodesic_grid_i32, the rules in include/ext/occ4d_geodesic.h).  clear (n,) int32, x slowest, z fastest: a point
    is passable when clear >= min_clear (ops.grid_distance's dist2: 1 = not solid, r * r = a ball of radius r fits); seeds (S,)
    int32 flat indices, those out of range or not passable are no sources (decided on the device); connectivity 6, 18 or 26; steps
    = the integer costs >= 1 of a face, an edge and a corner move; rounds: the number of relaxation rounds = launches, None =
    geodesic_default_rounds(counts); parent: also each point's predecessor.  resume: the cost tensor of an earlier call with the same
    arguments, relaxed further IN PLACE (seeds is not read).  `out` = (cost, status, parent or None), `work`: the caller's
    contiguous int32 buffers (>= n, >= 2, >= n, >= geodesic_work_len(rounds) elements).
    -> (cost (n,) int32, GEODESIC_CONSTANTS['NONE'] where no path arrives; status (2,) int32: 1 iff a round changed nothing -- cost
    is then THE shortest-path cost --, and the rounds that changed something; parent (n,) int32, -1 at seeds and unreached points,
    or None), on the device.  rounds + 2 launches, one more with parent, whatever the data.  No host read."""
    nx, ny, nz, n = _grid(counts)
    n = max(n, 0)
    c, _ = _inst_column(clear, n, 'clear', torch.int32)
    c = _contiguous(c)
    rounds = geodesic_default_rounds((nx, ny, nz)) if rounds is None else int(rounds)
    face, edge, corner = (int(s) for s in steps)
    if resume is None:
        s = _dev(seeds, torch.int32, 'seeds')
        assert s.dim() == 1, 'seeds must be (S,), got %s' % (tuple(s.shape),)
        s = _contiguous(s)
    else:
        assert out is None or out[0] is None, 'resume is relaxed in place: out must not hold a cost buffer'
        s = None
    out = _outs(out, 3)
    assert parent or out[2] is None, 'out holds a parent buffer without parent=True'
    cost = _int32_out(out[0] if resume is None else resume, (n,), c.device, 'resume' if resume is not None else 'out cost')
    status = _int32_out(out[1], (2,), c.device, 'out status')
    up = _int32_out(out[2], (n,), c.device, 'out parent') if parent else None
    wk = _int32_out(work, (geodesic_work_len(max(rounds, 0)),), c.device, 'work')
    if n == 0:
        status.zero_()                   # (the entry point touches no pointer of an empty grid)
    _lib.check(_lib.lib().occ4d_geodesic_grid_i32(_ptr(c), int(min_clear), nx, ny, nz, _ptr(s), 0 if s is None else s.shape[0],
                                                  int(connectivity), face, edge, corner, rounds, 0 if resume is None else 1, _ptr(wk),
                                                  _ptr(cost), _ptr(up), _ptr(status), _stream()))
    return cost, status, up


def geodesic_trace(cost, parent, goals, cap, out=None):
    """The paths from `goals` (G,) int32 flat indices back to a seed along `parent` (occ4d_geodesic_trace_i32): cost, parent (n,)
    int32 of ops.grid_geodesic(parent=True), cap: the most points of a path.  `out` = (paths, path_len): the caller's contiguous
    int32 buffers (>= G * cap, >= G).  -> (paths (G, cap) int32: goal first, the seed last, -1 behind it; path_len (G,) int32: the
    number of points, 0 for a goal that is out of range or unreached, -needed when the path has more than cap points), on the
    device.  One launch, one serial chain per goal.  No host read."""
    c = _dev(cost, torch.int32, 'cost')
    p = _dev(parent, torch.int32, 'parent')
    g = _dev(goals, torch.int32, 'goals')
    assert c.dim() == 1 and p.shape == c.shape and c.is_contiguous() and p.is_contiguous(), \
        'cost and parent must be contiguous (n,) tensors of one length, got %s and %s' % (tuple(c.shape), tuple(p.shape))
    assert g.dim() == 1, 'goals must be (G,), got %s' % (tuple(g.shape),)
    g = _contiguous(g)
    cap = int(cap)
    out = _outs(out, 2)
    paths = _int32_out(out[0], (g.shape[0], max(cap, 0)), c.device, 'out paths')
    path_len = _int32_out(out[1], (g.shape[0],), c.device, 'out path_len')
    _lib.check(_lib.lib().occ4d_geodesic_trace_i32(_ptr(c), _ptr(p), c.shape[0], _ptr(g), g.shape[0], cap, _ptr(paths), _ptr(path_len),
                                                   _stream()))
    return paths, path_len


def _blocked_words(blocked, counts):
    """(the contiguous (ceil(n / 32),) int32 words of ops.grid_blocked_bits, nx, ny, nz) for the grid `counts`."""
    nx, ny, nz, n = _grid(counts)
    return _bit_words(blocked, n, 'blocked'), nx, ny, nz


def grid_blocked_bits(clear, min_clear=1):
    """The blocked set !(clear >= min_clear), the complement of ops.grid_geodesic's passable set, packed one bit per grid point
    (occ4d_pull_bits_i32, the rules in include/ext/occ4d_pull.h): clear (n,) int32 -> (ceil(n / 32),) int32 on the device, bit
    p % 32 of word p // 32 is point p, the unused bits of the last word are 0.  One launch, no host read."""
    n = int(clear.shape[0])
    c, _ = _inst_column(clear, n, 'clear', torch.int32)
    c = _contiguous(c)
    bits = torch.empty(((n + 31) // 32,), dtype=torch.int32, device=c.device)
    _lib.check(_lib.lib().occ4d_pull_bits_i32(_ptr(c), int(min_clear), n, _ptr(bits), _stream()))
    return bits


def grid_segments(blocked, counts, a, b):
    """Line of sight between arbitrary pairs of points of the (nx, ny, nz) = `counts` grid (occ4d_pull_pairs_u32, HIT of include/
    ext/occ4d_pull.h): blocked (ceil(n / 32),) int32 from ops.grid_blocked_bits, a, b (P,) int32 flat indices, any values.
    -> hit (P,) int32 on the device: -1 where the segment a -> b is free, -2 where an index is outside the grid, else the flat
    index of the first blocked cell (a or b itself when blocked).  One launch, no host read."""
    words, nx, ny, nz = _blocked_words(blocked, counts)
    a, b = _dev(a, torch.int32, 'a'), _dev(b, torch.int32, 'b')
    assert a.dim() == 1 and a.shape == b.shape, 'a and b must be (P,) tensors of one length, got %s and %s' % (tuple(a.shape), tuple(b.shape))
    a, b = _contiguous(a), _contiguous(b)
    hit = torch.empty((a.shape[0],), dtype=torch.int32, device=words.device)
    _lib.check(_lib.lib().occ4d_pull_pairs_u32(_ptr(words), nx, ny, nz, _ptr(a), _ptr(b), a.shape[0], _ptr(hit), _stream()))
    return hit


def geodesic_pull(blocked, counts, paths, path_len, out=None):
    """The traced paths of ops.geodesic_trace pulled straight (occ4d_pull_paths_i32, PULL of include/ext/occ4d_pull.h): blocked
    (ceil(n / 32),) int32 from ops.grid_blocked_bits, paths (G, cap) int32, path_len (G,) int32.  `out` = (waypoints, waypoint_len):
    the caller's contiguous int32 buffers (>= G * cap, >= G).  -> (waypoints (G, cap) int32: a subsequence of the path, goal first,
    whose legs are free segments or single moves of the path, -1 behind it; waypoint_len (G,) int32: their number, path_len itself
    where that is <= 0 or > cap), on the device.  One launch, one workgroup per goal.  No host read."""
    words, nx, ny, nz = _blocked_words(blocked, counts)
    p, length = _dev(paths, torch.int32, 'paths'), _dev(path_len, torch.int32, 'path_len')
    assert p.dim() == 2 and tuple(length.shape) == (p.shape[0],) and p.is_contiguous() and length.is_contiguous(), \
        'paths and path_len must be contiguous (G, cap) and (G,) tensors, got %s and %s' % (tuple(p.shape), tuple(length.shape))
    goals, cap = int(p.shape[0]), int(p.shape[1])
    out = _outs(out, 2)
    waypoints = _int32_out(out[0], (goals, cap), words.device, 'out waypoints')
    waypoint_len = _int32_out(out[1], (goals,), words.device, 'out waypoint_len')
    if goals and nx * ny * nz <= 0:
        waypoints.fill_(-1)              # (the entry point touches no pointer of an empty grid, where the trace leaves no chain)
        waypoint_len.copy_(length)
    _lib.check(_lib.lib().occ4d_pull_paths_i32(_ptr(words), nx, ny, nz, _ptr(p), _ptr(length), goals, cap, _ptr(waypoints),
                                               _ptr(waypoint_len), _stream()))
    return waypoints, waypoint_len


def viewplan_work_len(C, W):
    """Elements of the int32 work array of occ4d_viewplan_greedy_u32 for C candidates and W words (the formula of the header):
    remaining (W), count (C + 1), the flag word."""
    return int(W) + int(C) + 2


def grid_visible(solid_bits, counts, targets, candidates, max_dist2=None, weights=(1, 1, 1), out=None):
    """Which of the target points of the (nx, ny, nz) = `counts` grid each candidate viewpoint sees (occ4d_viewplan_visible_u32, VIS
    of include/ext/occ4d_viewplan.h): solid_bits (W,) int32 from ops.grid_solid_bits, W = ceil(n / 32); targets (W,) int32 of the
    same layout, the points that count (ops.grid_blocked_bits(seen, 1): the points no sensor sees); candidates (C, 3) int32 lattice
    points ON THE DEVICE, any values: one beyond 2^20 cells or inside a solid cell sees nothing (decided on the device); max_dist2:
    None or negative = no limit, else a point counts when wx dx^2 + wy dy^2 + wz dz^2 <= max_dist2 with weights = (wx, wy, wz),
    integers in [1, 1024].  `out`: the caller's contiguous int32 buffer (>= C * W).  -> vis (C, W) int32 on the device: bit p % 32
    of word p // 32 of row c says that candidate c sees target point p.  One launch, no host read."""
    words, nx, ny, nz = _blocked_words(solid_bits, counts)
    tgt = _dev(targets, torch.int32, 'targets')
    assert tgt.shape == words.shape and tgt.is_contiguous(), \
        'targets must be a contiguous %s tensor, got %s' % (tuple(words.shape), tuple(tgt.shape))
    cand = _dev(candidates, torch.int32, 'candidates')
    assert cand.dim() == 2 and cand.shape[1] == 3, 'candidates must be (C, 3), got %s' % (tuple(cand.shape),)
    cand = _contiguous(cand)
    C, W = int(cand.shape[0]), int(words.shape[0])
    wx, wy, wz = (int(w) for w in weights)
    vis = _int32_out(out, (C, W), words.device, 'out')
    _lib.check(_lib.lib().occ4d_viewplan_visible_u32(_ptr(words), nx, ny, nz, _ptr(tgt), _ptr(cand), C, wx, wy, wz,
                                                     -1 if max_dist2 is None else int(max_dist2), _ptr(vis), _stream()))
    return vis


def viewplan_greedy(vis, targets, k, work=None, out=None):
    """The greedy choice of up to k candidates that together see the most target points (occ4d_viewplan_greedy_u32, GREEDY of
    include/ext/occ4d_viewplan.h): vis (C, W) int32 from ops.grid_visible, targets (W,) int32, k in [0, 32].  `work`: the caller's
    contiguous int32 buffer (>= viewplan_work_len(C, W)); `out` = (gain, picks, pick_gain, status): the caller's contiguous int32
    buffers (>= C, >= k, >= k, >= 2).  -> (gain (C,) int32: the target points each candidate sees on its own; picks (k,) int32: in
    each round the lowest candidate that sees the most of what no earlier pick sees, -1 from the round on in which nothing is left
    to see; pick_gain (k,) int32: what it added; status (2,) int32: the number of target points and how many of them no pick
    sees), on the device.  1 + 2 * max(k, 1) launches, whatever the data.  No host read."""
    v, tgt = _dev(vis, torch.int32, 'vis'), _dev(targets, torch.int32, 'targets')
    assert v.dim() == 2 and tuple(tgt.shape) == (v.shape[1],) and v.is_contiguous() and tgt.is_contiguous(), \
        'vis and targets must be contiguous (C, W) and (W,) tensors, got %s and %s' % (tuple(v.shape), tuple(tgt.shape))
    C, W, k = int(v.shape[0]), int(v.shape[1]), int(k)
    out = _outs(out, 4)
    gain = _int32_out(out[0], (C,), v.device, 'out gain')
    picks = _int32_out(out[1], (max(k, 0),), v.device, 'out picks')
    pick_gain = _int32_out(out[2], (max(k, 0),), v.device, 'out pick_gain')
    status = _int32_out(out[3], (2,), v.device, 'out status')
    wk = _int32_out(work, (viewplan_work_len(C, W),), v.device, 'work')
    if C == 0 or W == 0:
        gain.zero_(), status.zero_(), picks.fill_(-1), pick_gain.zero_()      # (the entry point touches no pointer then)
    _lib.check(_lib.lib().occ4d_viewplan_greedy_u32(_ptr(v), C, W, _ptr(tgt), k, _ptr(wk), _ptr(gain), _ptr(picks), _ptr(pick_gain),
                                                    _ptr(status), _stream()))
    return gain, picks, pick_gain, status


def grid_box_extents(labels, counts, K, dirs, out=None):
    """Per object and heading the extent of the object's footprint (occ4d_boxes_extents_i32, EXTENTS and RANGE of include/ext/
    occ4d_boxes.h): labels (n,) int32 on the (nx, ny, nz) = `counts` grid, any values -- point p belongs to object labels[p] when
    0 <= labels[p] < K --; dirs (A, 4) int32 ON THE DEVICE, rows (ax, ay, bx, by), any values: a row with a coefficient beyond
    2^15 is DEAD (decided on the device).  `out` = (extent, zr): the caller's contiguous int32 buffers (>= K * A * 4, >= K * 3).
    -> (extent (K, A, 4) int32: [min u, max u, min v, max v] of u = ax ix + ay iy, v = bx ix + by iy over the object's points,
    [INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN] for an object without points and a DEAD row; zr (K, 3) int32: [min iz, max iz,
    points]), on the device.  Two launches, whatever the data.  No host read."""
    nx, ny, nz, n = _grid(counts)
    n = max(n, 0)
    lab = _dev(labels, torch.int32, 'labels')
    assert lab.dim() == 1 and lab.shape[0] == n, 'labels must be (%d,), got %s' % (n, tuple(lab.shape))
    lab = _contiguous(lab)
    d = _dev(dirs, torch.int32, 'dirs')
    assert d.dim() == 2 and d.shape[1] == 4, 'dirs must be (A, 4), got %s' % (tuple(d.shape),)
    d = _contiguous(d)
    K, A = int(K), int(d.shape[0])
    out = _outs(out, 2)
    extent = _int32_out(out[0], (max(K, 0), A, 4), lab.device, 'out extent')
    zr = _int32_out(out[1], (max(K, 0), 3), lab.device, 'out zr')
    _lib.check(_lib.lib().occ4d_boxes_extents_i32(_ptr(lab), nx, ny, nz, K, _ptr(d), A, _ptr(extent), _ptr(zr), _stream()))
    return extent, zr


def boxes_choose(extent, zr, dirs, out=None):
    """Per object the heading whose rectangle has the least area (occ4d_boxes_choose_i32, CHOICE of include/ext/occ4d_boxes.h):
    extent (K, A, 4) int32, zr (K, 3) int32 of ops.grid_box_extents (or any values), dirs (A, 4) int32.  `out`: the caller's
    contiguous int32 buffer (>= K * 8).  -> box (K, 8) int32 on the device: [a*, min u, max u, min v, max v, min iz, max iz,
    points]; a* the lowest heading of least area (W1 * W2 with W = max - min + the width of one cell along the heading), -1 with
    zeros for an object without points, -1 with the z range and the count kept when no heading qualifies.  One launch, no host
    read."""
    e, z, d = _dev(extent, torch.int32, 'extent'), _dev(zr, torch.int32, 'zr'), _dev(dirs, torch.int32, 'dirs')
    assert d.dim() == 2 and d.shape[1] == 4, 'dirs must be (A, 4), got %s' % (tuple(d.shape),)
    K, A = int(z.shape[0]), int(d.shape[0])
    assert tuple(e.shape) == (K, A, 4) and tuple(z.shape) == (K, 3) and e.is_contiguous() and z.is_contiguous(), \
        'extent and zr must be contiguous (K, %d, 4) and (K, 3) tensors, got %s and %s' % (A, tuple(e.shape), tuple(z.shape))
    d = _contiguous(d)
    box = _int32_out(out, (K, _lib.BOXES_CONSTANTS['COLS']), e.device, 'out')
    _lib.check(_lib.lib().occ4d_boxes_choose_i32(_ptr(e), _ptr(z), _ptr(d), K, A, _ptr(box), _stream()))
    return box


LAYER_ARRAYS = ('label', 'first', 'samples', 'point', 'count', 'table', 'status')


def grid_layers(labels, k, counts, mins, spacings, rt_inv, k_inv, height, width, near, step, n_steps, max_layers, want=LAYER_ARRAYS):
    """The labelled objects of the (nx, ny, nz) = `counts` grid as depth layers in V camera views (occ4d_layers_march_i32, the rules
    in include/ext/occ4d_layers.h): labels (n,) int32, any values -- point p belongs to object labels[p] when 0 <= labels[p] < k --;
    mins / spacings, rt_inv, k_inv, near, step, n_steps as ops.raycast_grid takes them.  Per pixel the objects its ray passes
    through (the OWNER of a sample is the label of its nearest grid point) in the order of first entry, at most L = max_layers of
    them.  want: which of the seven arrays are made (the others are null in the call).
    -> dict of device tensors: label, first, samples, point (V, H, W, L) int32 (-1 / 0 in unused layers), count (V, H, W) int32 in
    0 .. L + 1 (L + 1: an object was dropped), table (V, k, 7) int32 = [amodal pixels, visible pixels, least first, xmin, xmax, ymin,
    ymax] per view and object, status (2,) int32 = [pixels with a dropped object, pixels with any object].  Two launches, whatever
    the data.  No host read."""
    nx, ny, nz, n = _grid(counts)
    lab = _dev(labels, torch.int32, 'labels')
    assert lab.dim() == 1 and lab.shape[0] == n, 'labels must be (%d,), got %s' % (n, tuple(lab.shape))
    lab = _contiguous(lab)
    rt, kk = _dev(rt_inv, name='rt_inv'), _dev(k_inv, name='k_inv')
    V = rt.shape[0] if rt.dim() else -1
    assert rt.dim() in (2, 3) and rt.numel() == V * 16 and tuple(kk.shape) == tuple(rt.shape), \
        'rt_inv / k_inv must both be (V, 16) or (V, 4, 4), got %s and %s' % (tuple(rt.shape), tuple(kk.shape))
    rt, kk = rt.contiguous(), kk.contiguous()
    K, H, W, L = int(k), int(height), int(width), int(max_layers)
    want = tuple(want)
    assert set(want) <= set(LAYER_ARRAYS), 'want = %r: names of %r' % (want, LAYER_ARRAYS)
    shapes = dict(label=(V, H, W, L), first=(V, H, W, L), samples=(V, H, W, L), point=(V, H, W, L), count=(V, H, W),
                  table=(V, max(K, 0), _lib.LAYERS_CONSTANTS['COLS']), status=(2,))
    ok = K >= 0 and H >= 0 and W >= 0 and L >= 0                 # (else the library's message; nothing is allocated)
    out = {name: torch.empty(shapes[name] if ok else (0,), dtype=torch.int32, device=lab.device) for name in LAYER_ARRAYS if name in want}
    _lib.check(_lib.lib().occ4d_layers_march_i32(
        _ptr(lab), nx, ny, nz, K, float(mins[0]), float(spacings[0]), float(mins[1]), float(spacings[1]), float(mins[2]),
        float(spacings[2]), _ptr(kk), _ptr(rt), V, H, W, float(near), float(step), int(n_steps), L,
        *(_ptr(out.get(name)) for name in LAYER_ARRAYS), _stream()))
    if V * H * W == 0:                                           # the call was a no-op: the table and the status of no pixel
        if 'table' in out and out['table'].numel():
            c = _lib.LAYERS_CONSTANTS
            fill = [2 ** 31 - 1] * c['COLS']
            fill[c['AMODAL']] = fill[c['VISIBLE']] = 0
            fill[c['XMAX']] = fill[c['YMAX']] = -1
            out['table'].copy_(torch.tensor(fill, dtype=torch.int32).to(lab.device).expand_as(out['table']))
        if 'status' in out:
            out['status'].zero_()
    return out


SWEEP_ARRAYS = ('range', 'point', 'cell', 'owner', 'cos', 'sem', 'inst', 'features')


def sweep_rays(values, counts, mins, spacings, level, pose, dirs, shape, near, step, n_steps, per_view=False, attrs=None, channels=(),
               sem=None, labels=None, k=0, background=0.0, feature_background=None, want=SWEEP_ARRAYS):
    """The field `values` on the (nx, ny, nz) = `counts` grid scanned along V bundles of R = B * A rays (occ4d_sweep_rays_f32, the
    rules in include/ext/occ4d_sweep.h): per ray the first of the n_steps samples at ranges near + i * step whose trilinear value
    is >= level, refined against the sample before it.  values (n,): one value per grid point, x slowest, z fastest (a strided
    column view is read in place); mins / spacings: the three floats each that ops.grid_points took for this grid; pose (V, 12) or
    (V, 3, 4): row-major [Rm | t], sensor to the grid's world; dirs (R, 3), or with per_view (V * R, 3) / (V, R, 3): directions in
    the sensor frame, NOT normalised on the device (the range is in units of their length); shape = (B, A).  attrs (n, d) with
    `channels`: the columns sampled at the hit, and with sem = (first column, number of classes): the class columns; labels (n,)
    int32 with k: an object per grid point, any values.  want: which arrays are made (the others are null in the call).
    -> dict of device tensors, each (V, R) unless said: range fp32 (`background` where nothing is hit), point (V, R, 3) fp32 (the
    hit position, or `background`), cell int32 (the hit cell's low corner, -1 = none), owner int32 (the cell's corner of greatest
    value, -1), cos fp32 (the incidence cosine, 0), sem int32 (the argmax of the class columns at owner, -1; only with sem), inst
    int32 (labels[owner] when in [0, k), else -1; only with labels), features (V, R, C) fp32 (`feature_background`, default
    `background`).  One launch, no host read."""
    nx, ny, nz, n = _grid(counts)
    v = _dev(values, name='values')
    assert v.dim() == 1 and v.shape[0] == n, 'values must be (%d,), got %s' % (n, tuple(v.shape))
    ps, dr = _dev(pose, name='pose'), _dev(dirs, name='dirs')
    V = ps.shape[0] if ps.dim() else -1
    assert ps.dim() in (2, 3) and ps.numel() == V * 12, 'pose must be (V, 12) or (V, 3, 4), got %s' % (tuple(ps.shape),)
    B, A = (int(s) for s in shape)
    R, per_view = B * A, bool(per_view)
    rows = V * R if per_view else R
    assert dr.dim() in (2, 3) and dr.shape[-1] == 3 and (B < 0 or A < 0 or dr.numel() == 3 * rows), \
        'dirs must hold %d rows of 3 (per_view = %r, V = %d, shape = %r), got %s' % (rows, per_view, V, (B, A), tuple(dr.shape))
    ps, dr = ps.contiguous(), dr.contiguous()
    cols = [int(c) for c in channels]
    n_ch = len(cols)
    sem_first, n_sem = (0, 0) if sem is None else (int(sem[0]), int(sem[1]))
    a, ld_attr, d = None, 0, 0
    if n_ch or n_sem:
        assert attrs is not None, 'channels and sem need attrs'
        a, ld_attr = _merge_rows(attrs, 'attrs')
        assert a.shape[0] == n, 'attrs must hold %d rows, got %d' % (n, a.shape[0])
        d = a.shape[1]
    lab = None
    if labels is not None:
        lab = _dev(labels, torch.int32, 'labels')
        assert lab.dim() == 1 and lab.shape[0] == n, 'labels must be (%d,), got %s' % (n, tuple(lab.shape))
        lab = _contiguous(lab)
    want = tuple(want)
    assert set(want) <= set(SWEEP_ARRAYS), 'want = %r: names of %r' % (want, SWEEP_ARRAYS)
    ok = B >= 0 and A >= 0                                        # (else the library's message; nothing is allocated)
    made = dict(range=((V, R), torch.float32), point=((V, R, 3), torch.float32), cell=((V, R), torch.int32), owner=((V, R), torch.int32),
                cos=((V, R), torch.float32), features=((V, R, n_ch), torch.float32))
    if n_sem:
        made['sem'] = ((V, R), torch.int32)
    if lab is not None:
        made['inst'] = ((V, R), torch.int32)
    out = {name: torch.empty(made[name][0] if ok else (0,), dtype=made[name][1], device=v.device)
           for name in SWEEP_ARRAYS if name in want and name in made}
    arr = (C.c_int32 * n_ch)(*cols) if n_ch else None
    fbg = background if feature_background is None else feature_background
    _lib.check(_lib.lib().occ4d_sweep_rays_f32(
        _ptr(v), v.stride(0) if n > 1 else 1, nx, ny, nz, float(mins[0]), float(spacings[0]), float(mins[1]), float(spacings[1]),
        float(mins[2]), float(spacings[2]), float(level), _ptr(ps), _ptr(dr), V, B, A, int(per_view), float(near), float(step),
        int(n_steps), _ptr(a), max(ld_attr, d), d, arr, n_ch, sem_first, n_sem, _ptr(lab), int(k), float(background), float(fbg),
        *(_ptr(out.get(name)) if name != 'features' or n_ch else None for name in SWEEP_ARRAYS), _stream()))
    return out


def grid_carve(returns, origins, counts, mins, spacings, sensor=None, counts_too=False):
    """Measured returns carved into the (nx, ny, nz) = `counts` grid (occ4d_evidence_carve_f32, the rules in include/ext/
    occ4d_evidence.h): returns (R, >= 3) float32 world points on the device, a row-strided view is read in place; origins (V, 3) int32
    lattice cells ON THE DEVICE, 1 <= V <= 4096, any values (the kernel checks what it reads); mins / spacings: the three floats each
    that ops.grid_points took for this grid; sensor (R,) int32 on the device or None = every return belongs to sensor 0;
    counts_too: also how many walks passed each cell.  -> (passed (ceil(n / 32),)
    int32, bit p % 32 of word p // 32 = a ray passed through cell p; hits (n,) int32; passes (n,) int32 or None; status (4,) int32 =
    [carved, dropped for the sensor, dropped as not finite / too far, dropped outside the grid]), on the device.  Two launches, no
    host read."""
    nx, ny, nz, n = _grid(counts)
    ret = _dev(returns, name='returns')
    assert ret.dim() == 2 and ret.shape[1] >= 3, 'returns must be (R, >= 3), got %s' % (tuple(ret.shape),)
    if ret.stride(1) != 1 or (ret.shape[0] > 1 and ret.stride(0) < 3):
        ret = ret.contiguous()
    R = int(ret.shape[0])
    ld = ret.stride(0) if R > 1 else max(int(ret.shape[1]), 3)
    org = _dev(origins, torch.int32, 'origins')
    assert org.dim() == 2 and org.shape[1] == 3, 'origins must be (V, 3), got %s' % (tuple(org.shape),)
    org = _contiguous(org)
    sen = None
    if sensor is not None:
        sen = _dev(sensor, torch.int32, 'sensor')
        assert tuple(sen.shape) == (R,), 'sensor must be (%d,), got %s' % (R, tuple(sen.shape))
        sen = _contiguous(sen)
    size = max(n, 0)
    passed = torch.empty(((size + 31) // 32,), dtype=torch.int32, device=ret.device)
    hits = torch.empty((size,), dtype=torch.int32, device=ret.device)
    passes = torch.empty((size,), dtype=torch.int32, device=ret.device) if counts_too else None
    status = torch.empty((4,), dtype=torch.int32, device=ret.device)
    _lib.check(_lib.lib().occ4d_evidence_carve_f32(
        _ptr(ret), ld, R, _ptr(sen), _ptr(org), int(org.shape[0]), nx, ny, nz, float(mins[0]), float(spacings[0]), float(mins[1]),
        float(spacings[1]), float(mins[2]), float(spacings[2]), _ptr(passed), _ptr(hits), _ptr(passes), _ptr(status), _stream()))
    return passed, hits, passes, status


def grid_evidence(values, level, hits, passed=None, passes=None, min_pass=1, mask=None, mask_level=0.0):
    """The six codes of prediction against evidence (occ4d_evidence_classify_f32, STATE, SOLID and CODE of include/ext/
    occ4d_evidence.h): values (n,), a strided column view is read in place, solid where values >= level (with mask (n,) also mask
    >= mask_level); hits (n,) int32 and passed (ceil(n / 32),) int32 from ops.grid_carve -- or passes (n,) int32, then a cell is FREE
    from min_pass walks on.  -> (code (n,) int32, totals (6,) int64: the histogram of code), on the device.  Two launches, no host
    read."""
    n = int(values.shape[0])
    v, ld = _inst_column(values, n, 'values')
    m, ld_mask = (None, 0) if mask is None else _inst_column(mask, n, 'mask')
    h = _dev(hits, torch.int32, 'hits')
    assert tuple(h.shape) == (n,) and h.is_contiguous(), 'hits must be a contiguous (%d,) tensor, got %s' % (n, tuple(h.shape))
    words = None if passed is None else _bit_words(passed, n, 'passed')
    ps = None
    if passes is not None:
        ps = _dev(passes, torch.int32, 'passes')
        assert tuple(ps.shape) == (n,) and ps.is_contiguous(), 'passes must be a contiguous (%d,) tensor, got %s' % (n, tuple(ps.shape))
    code = torch.empty((n,), dtype=torch.int32, device=v.device)
    totals = torch.empty((6,), dtype=torch.int64, device=v.device)
    _lib.check(_lib.lib().occ4d_evidence_classify_f32(_ptr(v), ld, float(level), _ptr(m), ld_mask, float(mask_level), n, _ptr(words),
                                                      _ptr(ps), int(min_pass), _ptr(h), _ptr(code), _ptr(totals), _stream()))
    return code, totals


def link_work_len(n, cap):
    """Elements of the int32 work array of occ4d_link_overlap_i32 for n grid points and `cap` pair rows (the formula of the
    header): 4 * slots + n + 2 * tiles with slots the smallest power of two >= max(2 * min(cap, n), MIN_SLOTS), at most 2^31."""
    k = _lib.LINK_CONSTANTS
    slots = k['MIN_SLOTS']
    while slots < 2 * min(cap, n) and slots < 2 ** 31:
        slots *= 2
    return 4 * slots + n + 2 * ((n + k['TILE'] - 1) // k['TILE'])


def components_overlap(labels_a, labels_b, k_a, k_b, cap=None, trim=False, pairs=None):
    """The overlaps of two label volumes of the same grid (occ4d_link_overlap_i32, the rules in include/ext/occ4d_link.h):
    labels_a, labels_b (n,) int32 as ops.grid_components returns them, k_a / k_b their numbers of components.  A point counts when
    0 <= labels_a[p] < k_a and 0 <= labels_b[p] < k_b.  -> (pairs (cap, 4) int64: a, b, count, root per distinct (a, b), numbered
    in the order of their lowest flat index, written below min(cap, totals[0]) only; totals (3,) int32: pairs, member points,
    1 if the work table overflowed), on the device.  cap=None: min(n, k_a * k_b), which holds every pair.  No host read unless
    trim=True: one 12-byte read, and pairs[:totals[0]] comes back.  `pairs`: a caller's contiguous int64 (>= cap, 4) buffer."""
    a = _dev(labels_a, torch.int32, 'labels_a')
    b = _dev(labels_b, torch.int32, 'labels_b')
    n = a.shape[0] if a.dim() == 1 else -1
    assert a.dim() == 1 and tuple(b.shape) == (n,) and a.is_contiguous() and b.is_contiguous(), \
        'labels_a and labels_b must be contiguous (n,) tensors of one length, got %s and %s' % (tuple(a.shape), tuple(b.shape))
    k_a, k_b = int(k_a), int(k_b)
    cap = min(n, k_a * k_b) if cap is None else int(cap)
    assert cap >= 0, 'cap = %d must be >= 0' % cap
    cols = _lib.LINK_CONSTANTS['PAIR_COLS']
    if pairs is None:
        pairs = torch.empty((cap, cols), dtype=torch.int64, device=a.device)
    else:
        pairs = _dev(pairs, torch.int64, 'pairs')
        assert pairs.dim() == 2 and pairs.shape[1] == cols and pairs.shape[0] >= cap and pairs.is_contiguous(), \
            'pairs must be a contiguous (>= %d, %d) tensor, got %s' % (cap, cols, tuple(pairs.shape))
    # (an empty grid is a no-op of the library: its totals are the zeros put here; the work array starts 16 bytes in: 8-byte aligned)
    scratch = (torch.empty if n else torch.zeros)(link_work_len(n, cap) + 4, dtype=torch.int32, device=a.device)
    totals, work = scratch[:3], scratch[4:]
    _lib.check(_lib.lib().occ4d_link_overlap_i32(_ptr(a), _ptr(b), k_a, k_b, n, _ptr(work), _ptr(pairs) if cap else None, cap,
                                                 _ptr(totals), _stream()))
    if trim:
        return pairs[:min(cap, int(totals.tolist()[0]))], totals
    return pairs[:cap], totals


def _min_iou_fraction(min_iou):
    if isinstance(min_iou, (tuple, list)):
        num, den = (int(v) for v in min_iou)
        return num, den
    from fractions import Fraction
    f = Fraction(min_iou).limit_denominator(2 ** 20)
    return f.numerator, f.denominator


def components_match(pairs, totals, table_a, table_b, track_a, next_id, min_iou=0.0):
    """The components of the later frame matched with those of the earlier one (occ4d_link_match_i32): pairs, totals as
    ops.components_overlap returns them (pairs at full cap), table_a (k_a, 12), table_b (k_b, 12) int64 the two component tables
    (column 0, the size, is read), track_a (k_a,) int32 the earlier frame's track ids, next_id (1,) int32 the first free track id,
    on the device.  b continues a when each is the other's best overlap by intersection over union and that is >= min_iou: a float,
    taken as Fraction(min_iou).limit_denominator(2 ** 20), or a (num, den) pair taken as it is.
    -> (link (k_b, 4) int32: track id, linked a or -1, best a or -1, its count; best_a (k_a, 2) int32: best b or -1, its count;
    next_out (1,) int32), on the device.  No host read."""
    num, den = _min_iou_fraction(min_iou)
    p = _dev(pairs, torch.int64, 'pairs')
    assert p.dim() == 2 and p.shape[1] == _lib.LINK_CONSTANTS['PAIR_COLS'] and p.is_contiguous(), \
        'pairs must be a contiguous (cap, 4) tensor, got %s' % (tuple(p.shape),)
    cap = p.shape[0]
    t = _dev(totals, torch.int32, 'totals')
    assert tuple(t.shape) == (3,) and t.is_contiguous(), 'totals must be a contiguous (3,) tensor, got %s' % (tuple(t.shape),)
    ta, lda = _rows(_dev(table_a, torch.int64, 'table_a'), 'table_a')
    tb, ldb = _rows(_dev(table_b, torch.int64, 'table_b'), 'table_b')
    assert ta.shape[1] >= 1 and tb.shape[1] >= 1, 'the tables need their size column'
    k_a, k_b = ta.shape[0], tb.shape[0]
    tr = _dev(track_a, torch.int32, 'track_a')
    assert tuple(tr.shape) == (k_a,) and tr.is_contiguous(), 'track_a must be a contiguous (%d,) tensor, got %s' % (k_a, tuple(tr.shape))
    nx = _dev(next_id, torch.int32, 'next_id')
    assert nx.numel() == 1, 'next_id must hold one element, got %s' % (tuple(nx.shape),)
    link = torch.empty((k_b, 4), dtype=torch.int32, device=p.device)
    best_a = torch.empty((k_a, 2), dtype=torch.int32, device=p.device)
    next_out = torch.empty((1,), dtype=torch.int32, device=p.device)
    used = k_a > 0 and k_b > 0 and cap > 0
    _lib.check(_lib.lib().occ4d_link_match_i32(_ptr(p) if used else None, _ptr(t), cap, _ptr(ta) if k_a else None, max(lda, 1),
                                               _ptr(tb) if k_b else None, max(ldb, 1), k_a, k_b, _ptr(tr) if k_a else None, num, den,
                                               _ptr(nx), _ptr(link) if k_b else None, _ptr(best_a) if k_a else None, _ptr(next_out),
                                               _stream()))
    return link, best_a, next_out
