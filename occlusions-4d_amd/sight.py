"""Line of sight through the decoded occupancy on the dense query grid, on the device (include/ext/occ4d_sight.h): of the predicted
scene, solid and free alike, which part lies in direct view of a sensor, which part is hidden behind predicted solid -- and behind
which cell --, and which part lies outside every frustum.  From ONE decode.

perform_inference(sight=Sight(origins=...)) adds result['sight'] = dict(seen (N,) int32[, framed (N,) int32][, blocker (V, N)
int32]): bit v of seen[q] says that the straight segment from query q to sensor v passes through free cells only; with cameras, bit v
of framed[q] says that q projects into the image of camera v at all (projection.visibility's OUTSIDE rule, bit for bit); with
blocker=True, blocker[v, q] is the flat index of the cell that hides q from sensor v, -1 where q is seen or not framed.

    res = perform_inference(..., point_sample_mode='grid', components=Components(), sight=Sight(origins=lidar_positions))
    s = res['sight']
    code = sight.codes(s['seen'])                                   # projection.VISIBLE / OCCLUDED / OUTSIDE per query
    share = sight.by_label(labels, k, seen)                         # per object: seen, hidden, unframed queries (device tensors)

THE ONE APPROXIMATION.  A sensor position becomes the grid cell that contains it, floor((position - mins) / spacings) in float64
on the host (grid_origin): a snap of at most one cell.  Everything after it is exact on the lattice: the walk visits the supercover
of the segment between the two cell centres, compares in 64-bit integers, and where the segment passes exactly through an edge or a
corner it passes only if a staircase of free cells leads around it (the header's SQUEEZE), so that a one-cell-thick wall, however it
is connected, hides what lies behind it.  A query is never tested itself: a solid query on the surface that faces the sensor is seen,
one inside an object is hidden.  Sensors may lie outside the grid (up to 2^20 cells away); the cells outside the grid are free.
Unlike the views= ray cast followed by projection.visibility this needs no image, no pixel and no float margin, so it serves a lidar as
well as a camera.  Everything is an integer, so every output is the same bit for bit under any scheduling.

THE NEXT BEST VIEW (include/ext/occ4d_viewplan.h).  From where should the sensor look next?  perform_inference(sight=Sight(...),
next_view=NextView(candidates, k)) adds result['next_view'] = dict(gain (C,), picks (k,), pick_gain (k,), status (2,)), all int32:
of the queries no current sensor sees (seen == 0), how many each candidate viewpoint would see on its own (gain), and a greedy
choice of up to k candidates that together see the most -- picks[r] is the lowest candidate that sees the most of what picks[:r]
leave unseen, -1 once nothing is left; status = [the unseen queries, those no pick sees].  The same walk, the same snap of a
candidate to its cell; a candidate inside a predicted solid cell sees nothing.  plan() is the stand-alone piece.

    res = perform_inference(..., sight=Sight(origins=lidar_positions), next_view=NextView(ring_of_positions, k=3, among='solid'))
    best = res['next_view']['picks']                                # indices into ring_of_positions, -1 behind the useful ones

NOT MEASURED: which share of a trained model's scene is hidden, and what a trained model's candidates gain.  There is no
checkpoint."""
import numpy as np
import torch

from . import _lib, ops, products, projection

MAX_ORIGINS = _lib.SIGHT_CONSTANTS['MAX_ORIGINS']
MAX_COORD = _lib.SIGHT_CONSTANTS['MAX_COORD']
MAX_CANDIDATES = _lib.VIEWPLAN_CONSTANTS['MAX_CANDIDATES']
MAX_PICKS = _lib.VIEWPLAN_CONSTANTS['MAX_PICKS']
MAX_WEIGHT = _lib.VIEWPLAN_CONSTANTS['MAX_WEIGHT']
AMONG = ('all', 'solid')


def _count(V, who):
    if not 1 <= V <= MAX_ORIGINS:
        raise ValueError('%s: V = %d origins, must be in [1, %d]' % (who, V, MAX_ORIGINS))


def grid_origin(points, mins, spacings):
    """World points (V, 3) -> (V, 3) int32 lattice points of the cell-centred grid of geometry.grid_frame: the cell that contains
    the point, floor((p - mins) / spacings) in float64 -- geodesic.grid_index's convention without its range error: a sensor may
    stand outside the grid.  ValueError for a point that is not finite or more than 2^20 cells from cell 0 (the header's limit)."""
    p = np.asarray(points, np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError('grid_origin: points must be (V, 3), got %s' % (p.shape,))
    with np.errstate(all='ignore'):
        g = np.floor((p - np.asarray(mins, np.float64)) / np.asarray(spacings, np.float64))
    bad = ~(np.isfinite(g) & (np.abs(g) <= MAX_COORD)).all(1)
    if bad.any():
        v = int(np.flatnonzero(bad)[0])
        raise ValueError('grid_origin: origin %d = %r lies beyond 2^20 cells (cell %r)' % (v, p[v].tolist(), g[v].tolist()))
    return g.astype(np.int32)


def _lattice(origins_ijk, who):
    """(V, 3) int32 numpy of integer lattice origins; ValueError unless 1 <= V <= 31 and every coordinate is within 2^20."""
    o = np.asarray(origins_ijk)
    if o.ndim != 2 or o.shape[1] != 3 or o.dtype.kind not in 'iu':
        raise ValueError('%s: origins must be (V, 3) integers, got %s %s' % (who, o.dtype, o.shape))
    _count(o.shape[0], who)
    if np.abs(o.astype(np.int64)).max() > MAX_COORD:
        raise ValueError('%s: an origin lies beyond 2^20 cells' % who)
    return np.ascontiguousarray(o, dtype=np.int32)


def _select(select, who):
    try:
        return None if select is None else (int(select[0]), float(select[1]))
    except (TypeError, IndexError) as e:
        raise ValueError('%s: select = %r must be (column, threshold) or None' % (who, select)) from e


class Sight(products.LevelProduct):
    """The option object of perform_inference(sight=...) / evaluate_clip(sight=..., sights=[]).  Exactly one of
    origins: (V, 3) world points, the sensors' positions (for CARLA the lidar's position per sweep), every query is framed; and
    cameras = (cam_RT (V, 3, 4), cam_K (3, 3) or (V, 3, 3), height, width): the origins are the camera centres, from
    projection.invert_cameras's float64 matrices on the host, and bit v of `framed` is projection.visibility(<the call's query
    points>, zeros (V, H, W), cam_RT, cam_K, 0.0) != OUTSIDE: the query lies in front of camera v and projects into its image.
    1 <= V <= 31.  level: the density from which a query is solid (density >= level), None = the call's density_threshold; select =
    (column, threshold) or None: solid queries also need implicit_output[:, column] >= threshold; blocker: also which cell hides.
    The product: dict(seen (N,) int32[, framed (N,) int32 with cameras][, blocker (V, N) int32 with blocker=True]) (the module's
    doc-string); no device value is read.  All host work happens in prepare(), before the encode: the origins snapped to cells of
    the call's grid (the only approximation, at most one cell), ValueError for V or for an origin beyond 2^20 cells.  In
    track_mode 'all' the solid set is that of the merged array, under `refine` that of the expanded one."""
    keyword, clip_list = 'sight', ('sights', 'one dict of seen[, framed][, blocker]')

    def __init__(self, origins=None, cameras=None, level=None, select=None, blocker=False):
        if (origins is None) == (cameras is None):
            raise ValueError('Sight: exactly one of origins and cameras must be given')
        self.level, self.select, self.blocker = self._level(level), _select(select, 'Sight'), bool(blocker)
        self.cameras = None
        if cameras is not None:
            try:
                cam_RT, cam_K, height, width = cameras
            except (TypeError, ValueError) as e:
                raise ValueError('Sight: cameras must be (cam_RT, cam_K, height, width)') from e
            rt64 = projection.invert_cameras(cam_RT, cam_K)[2]
            origins = np.linalg.inv(rt64)[:, :3, 3]                               # the camera centres, float64
            self.cameras = (cam_RT, cam_K, int(height), int(width))
            if self.cameras[2] < 0 or self.cameras[3] < 0:
                raise ValueError('Sight: height = %r, width = %r' % (height, width))
        self.origins = np.array(origins, np.float64)
        if self.origins.ndim != 2 or self.origins.shape[1] != 3:
            raise ValueError('Sight: origins must be (V, 3) world points, got %s' % (self.origins.shape,))
        _count(self.origins.shape[0], 'Sight')

    def prepare(self, grid):
        return self.resolve(grid.density_threshold), _lattice(grid_origin(self.origins, grid.mins, grid.spacings), 'Sight')

    def frame(self, points):
        """framed (N,) int32 of the points (N, >= 3) on their device: the OUTSIDE rule of projection.visibility; no host read."""
        cam_RT, cam_K, height, width = self.cameras
        V = self.origins.shape[0]
        device = projection._device(points)
        code = projection.visibility(points, torch.zeros((V, height, width), dtype=torch.float32, device=device), cam_RT, cam_K, 0.0)
        weight = torch.tensor([1 << v for v in range(V)], dtype=torch.int32, device=code.device)
        return ((code != projection.OUTSIDE).to(torch.int32) * weight[:, None]).sum(0, dtype=torch.int32)

    def run(self, grid, prepared, made):
        level, origins_ijk = prepared
        framed = None if self.cameras is None else self.frame(grid.points)
        seen, blocker = look(grid.output, grid.counts, origins_ijk, level, self.select, framed, self.blocker)
        out = dict(seen=seen)
        if framed is not None:
            out['framed'] = framed
        if blocker is not None:
            out['blocker'] = blocker
        return out

    def __repr__(self):
        return 'Sight(V=%d, %s, level=%r, select=%r, blocker=%r)' % (
            self.origins.shape[0], 'origins' if self.cameras is None else 'cameras %d x %d' % self.cameras[2:], self.level,
            self.select, self.blocker)


def look(implicit_output, counts, origins_ijk, level, select=None, framed=None, blocker=False, channel=0):
    """The stand-alone piece: line of sight through the set column `channel` >= level of a dense (N, G) output on the (nx, ny, nz) =
    `counts` grid, towards the lattice origins origins_ijk (V, 3) integers on the host (grid_origin).  select = (column,
    threshold): the mask column; framed (N,) int32 on the device or None.  ops.grid_solid_bits, then ops.grid_sight -> (seen (N,)
    int32, blocker (V, N) int32 or None) on the device; nothing is read back."""
    level = float(level)
    if level != level:
        raise ValueError('sight.look: level is NaN')
    origins_ijk = _lattice(origins_ijk, 'sight.look')
    values, mask, mask_level = products.columns(implicit_output, channel, _select(select, 'sight.look'))
    bits = ops.grid_solid_bits(values, level, mask, mask_level)
    return ops.grid_sight(bits, counts, origins_ijk, framed, blocker)


def codes(seen, framed=None, view=None):
    """int32 codes projection.VISIBLE / OCCLUDED / OUTSIDE of every query, from seen (N,) and framed (N,) or None = every origin
    frames every query (torch tensors on any device, or numpy -> the same kind).  view = v: under origin v -- VISIBLE where bit v
    of seen is set, else OCCLUDED where bit v of framed is set, else OUTSIDE.  view = None: under any origin -- VISIBLE if seen by
    one, OUTSIDE if framed by none, else OCCLUDED.  No host read."""
    if not isinstance(seen, torch.Tensor):
        out = codes(torch.from_numpy(np.ascontiguousarray(seen, dtype=np.int32)),
                    None if framed is None else torch.from_numpy(np.ascontiguousarray(framed, dtype=np.int32)), view)
        return out.numpy()
    if view is not None and not 0 <= int(view) < MAX_ORIGINS:
        raise ValueError('sight.codes: view = %r must be in [0, %d) or None' % (view, MAX_ORIGINS))
    pick = (lambda t: t != 0) if view is None else (lambda t: (t >> int(view)) & 1 != 0)
    is_seen = pick(seen)
    is_framed = torch.ones_like(is_seen) if framed is None else pick(framed)
    full = lambda c: torch.full_like(seen, c, dtype=torch.int32)
    return torch.where(is_seen & is_framed, full(projection.VISIBLE), torch.where(is_framed, full(projection.OCCLUDED), full(projection.OUTSIDE)))


def by_label(labels, k, seen, framed=None):
    """THE QUESTION THIS FEATURE EXISTS FOR: how much of each predicted object was never observed.  labels (N,) integers on the
    device: per query the number in [0, k) of its component or segment (components.label, watershed.split; anything else, like -1
    = air, is left out); -> (k, 3) int64 on the device: per number the queries seen by any origin, hidden from all origins that
    frame them, and framed by none.  row[1] / row.sum() is the hidden share of the object: the part completed amodally.  torch
    operations only; nothing is read back."""
    k = int(k)
    code = codes(seen, framed).to(torch.int64)                          # VISIBLE 0, OCCLUDED 1, OUTSIDE 2: the column
    lab = labels.to(torch.int64)
    slot = torch.where((lab >= 0) & (lab < k), lab * 3 + code, torch.full_like(lab, 3 * k))
    table = torch.zeros((3 * k + 1,), dtype=torch.int64, device=seen.device)
    table.scatter_add_(0, slot, torch.ones_like(slot))
    return table[:3 * k].view(k, 3)


# ---------------------------------------------------------------------------------------------------------------- the next best view
def _plan_options(k, among, max_dist2, weights, who):
    """(k, among, max_dist2 or None, (wx, wy, wz)) checked: ValueError."""
    try:
        k_int = int(k)
        weights = tuple(int(w) for w in weights)
        max_dist2 = None if max_dist2 is None else int(max_dist2)
    except (TypeError, ValueError) as e:
        raise ValueError('%s: k = %r, max_dist2 = %r and weights = %r must be integers' % (who, k, max_dist2, weights)) from e
    if k_int != k or not 0 <= k_int <= MAX_PICKS:
        raise ValueError('%s: k = %r must be an integer in [0, %d]' % (who, k, MAX_PICKS))
    if among not in AMONG:
        raise ValueError("%s: among = %r must be 'all' or 'solid'" % (who, among))
    if len(weights) != 3 or not all(1 <= w <= MAX_WEIGHT for w in weights):
        raise ValueError('%s: weights = %r must be three integers in [1, %d]' % (who, weights, MAX_WEIGHT))
    if max_dist2 is not None and not -2 ** 63 <= max_dist2 < 2 ** 63:
        raise ValueError('%s: max_dist2 = %r must fit int64' % (who, max_dist2))
    return k_int, among, max_dist2, weights


def _candidate_count(C, who):
    if not 1 <= C <= MAX_CANDIDATES:
        raise ValueError('%s: C = %d candidates, must be in [1, %d]' % (who, C, MAX_CANDIDATES))


def _candidates(candidates_ijk, who):
    """(C, 3) int32 numpy of integer lattice candidates; ValueError unless 1 <= C <= 4096 and every coordinate is within 2^20."""
    c = np.asarray(candidates_ijk)
    if c.ndim != 2 or c.shape[1] != 3 or c.dtype.kind not in 'iu':
        raise ValueError('%s: candidates must be (C, 3) integers, got %s %s' % (who, c.dtype, c.shape))
    _candidate_count(c.shape[0], who)
    if np.abs(c.astype(np.int64)).max() > MAX_COORD:
        raise ValueError('%s: a candidate lies beyond 2^20 cells' % who)
    return np.ascontiguousarray(c, dtype=np.int32)


def cells_to_world(ijk, mins, spacings):
    """Lattice points (..., 3) integers -> the centres of their cells, float64 world points: mins + (ijk + 0.5) * spacings, the
    inverse of grid_origin up to the snap.  candidates_world[picks] needs no such step; this one is for candidates that were cells
    from the start (the cells route= found reachable)."""
    c = np.asarray(ijk)
    if c.shape[-1:] != (3,) or c.dtype.kind not in 'iu':
        raise ValueError('cells_to_world: ijk must be (..., 3) integers, got %s %s' % (c.dtype, c.shape))
    return np.asarray(mins, np.float64) + (c.astype(np.float64) + 0.5) * np.asarray(spacings, np.float64)


def plan(implicit_output, counts, seen, candidates_ijk, k=1, level=0.5, select=None, among='all', max_dist2=None, weights=(1, 1, 1),
         channel=0, keep_vis=False):
    """The stand-alone piece of the next best view (include/ext/occ4d_viewplan.h): implicit_output (N, G) dense on the (nx, ny, nz)
    = `counts` grid, its solid set column `channel` >= level (select = (column, threshold): the mask column), as in look(); seen
    (N,) int32 of look() under the current sensors: THE TARGETS ARE THE QUERIES WITH seen == 0, with among='solid' only the solid
    ones of them (the amodally completed object parts), with among='all' free space too (exploration).  candidates_ijk: (C, 3)
    integers on the host, 1 <= C <= 4096, within 2^20 cells (ValueError) -- or an int32 (C, 3) tensor that is on the device already,
    taken as it is: the kernel checks its values, one out of range sees nothing.  A candidate in a solid cell sees nothing.  k in
    [0, 32]: the picks; max_dist2 (None: no limit) and weights (wx, wy, wz): a target counts for a candidate only within
    wx dx^2 + wy dy^2 + wz dz^2 <= max_dist2, in cells.  ops.grid_solid_bits, ops.grid_blocked_bits, ops.grid_visible,
    ops.viewplan_greedy -> dict(gain (C,), picks (k,), pick_gain (k,), status (2,)) int32 on the device (ops.viewplan_greedy
    describes them), with keep_vis=True also vis (C, ceil(N / 32)): bit q % 32 of word q // 32 of row c = candidate c sees target q.
    Nothing is read back."""
    level = float(level)
    if level != level:
        raise ValueError('sight.plan: level is NaN')
    k, among, max_dist2, weights = _plan_options(k, among, max_dist2, weights, 'sight.plan')
    values, mask, mask_level = products.columns(implicit_output, channel, _select(select, 'sight.plan'))
    if isinstance(candidates_ijk, torch.Tensor):
        cand = candidates_ijk
        if cand.dim() != 2 or cand.shape[1] != 3 or cand.dtype != torch.int32:
            raise ValueError('sight.plan: a candidates tensor must be (C, 3) int32, got %s %s' % (cand.dtype, tuple(cand.shape)))
        _candidate_count(cand.shape[0], 'sight.plan')
    else:
        cand = torch.from_numpy(_candidates(candidates_ijk, 'sight.plan')).to(values.device)
    bits = ops.grid_solid_bits(values, level, mask, mask_level)
    targets = ops.grid_blocked_bits(seen, 1)                          # !(seen >= 1): no sensor sees the query
    if among == 'solid':
        targets = targets & bits
    vis = ops.grid_visible(bits, counts, targets, cand, max_dist2, weights)
    gain, picks, pick_gain, status = ops.viewplan_greedy(vis, targets, k)
    out = dict(gain=gain, picks=picks, pick_gain=pick_gain, status=status)
    if keep_vis:
        out['vis'] = vis
    return out


class NextView(products.LevelProduct):
    """The option object of perform_inference(next_view=...) / evaluate_clip(next_view=..., next_views=[]); needs `sight`
    (ValueError): the targets are the queries that call's sensors do not see.  candidates: (C, 3) world points, 1 <= C <= 4096, the
    viewpoints to rank; k in [0, 32]: how many to pick; among: 'all' = every unseen query counts (exploration), 'solid' = the
    unseen solid ones (the amodally completed object parts); max_dist2, weights: the sensor's range in cells (plan()); level,
    select: the solid set the candidates look through -- THEY SHOULD BE THE Sight OPTION'S, so that both products walk the same
    scene; level None = the call's density_threshold.  The product: dict(gain (C,), picks (k,), pick_gain (k,), status (2,)), all
    int32 (plan()); picks index `candidates`.  No device value is read: the arrays come home under the call's one host wait.  All
    host work happens in prepare(), before the encode: the candidates snapped to cells of the call's grid with grid_origin (the
    same one approximation as the sensors', at most one cell), ValueError for one beyond 2^20 cells.
    NOT MEASURED: the gains of a trained model's scene.  There is no checkpoint."""
    keyword, clip_list = 'next_view', ('next_views', 'one dict of gain, picks, pick_gain, status')
    needs = ('sight', 'next_view needs sight: the targets are the queries its sensors do not see')

    def __init__(self, candidates, k=1, among='all', max_dist2=None, weights=(1, 1, 1), level=None, select=None):
        self.k, self.among, self.max_dist2, self.weights = _plan_options(k, among, max_dist2, weights, 'NextView')
        self.level, self.select = self._level(level), _select(select, 'NextView')
        self.candidates = np.array(candidates, np.float64)
        if self.candidates.ndim != 2 or self.candidates.shape[1] != 3:
            raise ValueError('NextView: candidates must be (C, 3) world points, got %s' % (self.candidates.shape,))
        _candidate_count(self.candidates.shape[0], 'NextView')

    def prepare(self, grid):
        return self.resolve(grid.density_threshold), _candidates(grid_origin(self.candidates, grid.mins, grid.spacings), 'NextView')

    def run(self, grid, prepared, made):
        level, candidates_ijk = prepared
        return plan(grid.output, grid.counts, made['sight']['seen'], torch.from_numpy(candidates_ijk).to(grid.device), self.k, level,
                    self.select, self.among, self.max_dist2, self.weights)

    def __repr__(self):
        return 'NextView(C=%d, k=%d, among=%r, max_dist2=%r, weights=%r, level=%r, select=%r)' % (
            self.candidates.shape[0], self.k, self.among, self.max_dist2, self.weights, self.level, self.select)
