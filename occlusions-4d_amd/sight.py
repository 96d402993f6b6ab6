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

NOT MEASURED: which share of a trained model's scene is hidden.  There is no checkpoint."""
import numpy as np
import torch

from . import _lib, ops, products, projection

MAX_ORIGINS = _lib.SIGHT_CONSTANTS['MAX_ORIGINS']
MAX_COORD = _lib.SIGHT_CONSTANTS['MAX_COORD']


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
