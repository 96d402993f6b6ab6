"""The connected components of the decoded occupancy on the dense query grid, on the device (include/ext/occ4d_components.h):
how many separate objects the predicted solid set holds and where each one is, from ONE decode.

perform_inference(components=Components()) adds result['components'] = dict(labels (N,) int32, table (K, 12) int64): per query
the number of its component (-1: air, or a component smaller than min_size), per component its size, root (lowest flat index),
class, and the sums, minima and maxima of its integer grid coordinates.  Components are numbered in the order of their roots; with
connectivity 6 / 18 / 26, min_size 1 and no classes that is scipy.ndimage.label's numbering minus one.

    res = perform_inference(..., point_sample_mode='grid', components=Components(min_size=20))
    frame = geometry.grid_frame(num_sample, min_z, cube_bounds, data_kind, cube_mode)        # counts, mins, spacings
    objects = boxes_and_centroids(res['components']['table'], frame[1], frame[2])

The table holds integers only, so it is the same bit for bit under any scheduling; world-space centroids and boxes are made from
it on the host in float64 (boxes_and_centroids).

perform_inference(components=Components(), boxes=Boxes()) also adds box (K, 8) int32 and dirs (A, 4) int32 to that dict: per object
the upright oriented box of least footprint area over a table of headings (include/ext/occ4d_boxes.h; yaw_directions,
oriented_boxes)."""
import numpy as np
import torch

from . import _lib, ops, products

CONNECTIVITIES = (6, 18, 26)


class Components(products.LevelProduct):
    """The option object of perform_inference(components=...) / evaluate_clip(components=..., objects=[]).  level: the density from
    which a query is solid (density >= level, the comparison of the solid split), None = the call's density_threshold; connectivity:
    6, 18 or 26; select = (column, threshold) or None: members also need implicit_output[:, column] >= threshold (with the track
    channel: the tracked object alone); by_class: neighbours must share their semantic class (the argmax of the semantic columns,
    first maximum wins; needs predict_segmentation); min_size: components of fewer points are dropped.  The product: dict(labels
    (N,) int32, table (K, 12) int64) (label); one 12-byte device->host read sizes the table."""
    keyword, clip_list = 'components', ('objects', 'one dict of labels and table')

    def __init__(self, level=None, connectivity=6, select=None, by_class=False, min_size=1):
        level = self._level(level)
        if isinstance(connectivity, bool) or connectivity not in CONNECTIVITIES:
            raise ValueError('Components: connectivity = %r must be 6, 18 or 26' % (connectivity,))
        if isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer)) or not 1 <= min_size <= 2 ** 31 - 1:
            raise ValueError('Components: min_size = %r must be an integer >= 1' % (min_size,))
        self.level, self.connectivity, self.min_size, self.by_class = level, int(connectivity), int(min_size), bool(by_class)
        self.select = None if select is None else (int(select[0]), float(select[1]))

    def prepare(self, grid):
        if self.by_class and not grid.predict_segmentation:
            raise ValueError('components with by_class=True needs predict_segmentation=True')
        return self.resolve(grid.density_threshold)

    def run(self, grid, level, made):
        out, klass = grid.output, None
        if self.by_class:
            klass = semantic_class(out, out.shape[1] - grid.semantic_classes, grid.semantic_classes)
        labels, table = label(out, grid.counts, level, self.connectivity, self.select, klass, self.min_size)
        return dict(labels=labels, table=table)

    def __repr__(self):
        return 'Components(level=%r, connectivity=%d, select=%r, by_class=%r, min_size=%d)' % (
            self.level, self.connectivity, self.select, self.by_class, self.min_size)


def label(implicit_output, counts, level, connectivity=6, select=None, klass=None, min_size=1, channel=0):
    """The components of column `channel` of a dense (N, G) output on the (nx, ny, nz) = `counts` grid at `level`.  select =
    (column, threshold): the mask column; klass (N,) int32 or None.  -> (labels (N,) int32, table (K, 12) int64) on the device; one
    12-byte device->host read (the totals) sizes the table."""
    level = float(level)
    if level != level:
        raise ValueError('components.label: level is NaN')
    values, mask, mask_level = products.columns(implicit_output, channel, select)
    labels, _, table = ops.grid_components(values, counts, level, connectivity, min_size, mask, mask_level, klass)
    return labels, table


def semantic_class(implicit_output, first, n_classes):
    """(N,) int32: the argmax of columns first .. first + n_classes - 1, the first maximum wins (the rule of compress_air)."""
    assert 0 <= first and first + n_classes <= implicit_output.shape[1] and n_classes >= 1, \
        'semantic columns %d .. %d of %d' % (first, first + n_classes - 1, implicit_output.shape[1])
    return torch.argmax(implicit_output[:, first:first + n_classes], dim=1).to(torch.int32)


class Tracker(products.GridProduct):
    """Links the components of consecutive output frames on the device (include/ext/occ4d_link.h): the option object of
    perform_inference(components=..., tracker=...) / evaluate_clip(..., tracker=...).  Component b of a frame continues component a
    of the frame before when each is the other's best overlap by intersection over union and that is >= min_iou (a float, or an
    exact (num, den) pair); it then keeps a's track id, and every other component takes the next free id, in order.  The product
    joins the components' dict: link (K, 4) int32 (add_frame), made from that call's labels and table.

    The previous frame's labels, table and track ids and the id counter stay on the device; add_frame reads nothing back."""
    keyword, into, reads_grid = 'tracker', 'components', False
    needs = ('components', 'tracker needs components=<a components.Components>: it links the components of consecutive frames')

    def __init__(self, min_iou=0.0):
        num, den = ops._min_iou_fraction(min_iou)
        if not (1 <= den <= 2 ** 20 and 0 <= num <= den):
            raise ValueError('Tracker: min_iou = %r must lie in [0, 1]' % (min_iou,))
        self.min_iou = (num, den)
        self.reset()

    def reset(self):
        """Forgets the previous frame and the ids: the next frame numbers its components 0, 1, ..."""
        self.labels = self.table = self.track = self.next = None

    def add_frame(self, labels, table):
        """labels (n,) int32, table (K, 12) int64: a frame's components (components.label).  -> link (K, 4) int32 on the device: per
        component its track id, the component of the previous frame it continues or -1, its best overlap there or -1, and that
        overlap's number of points."""
        if self.labels is not None and labels.shape[0] != self.labels.shape[0]:
            raise ValueError('Tracker.add_frame: labels of %d points after a frame of %d' % (labels.shape[0], self.labels.shape[0]))
        if self.labels is None:                                               # a first frame: nothing to continue
            self.labels, self.table = labels, table[:0]
            self.track = torch.empty((0,), dtype=torch.int32, device=labels.device)
        if self.next is None:
            self.next = torch.zeros((1,), dtype=torch.int32, device=labels.device)
        pairs, totals = ops.components_overlap(self.labels, labels, self.table.shape[0], table.shape[0])
        link, _, self.next = ops.components_match(pairs, totals, self.table, table, self.track, self.next, self.min_iou)
        self.labels, self.table, self.track = labels, table, link[:, 0].contiguous()
        return link

    def run(self, grid, prepared, made):
        return dict(link=self.add_frame(made['components']['labels'], made['components']['table']))

    def n_tracks(self):
        """The number of track ids handed out so far: the one host read."""
        return 0 if self.next is None else int(self.next.item())

    def __repr__(self):
        return 'Tracker(min_iou=(%d, %d))' % self.min_iou


BOXES_OF = ('components', 'segments')
YAW_SCALE = 2 ** 14                  # S: the integer length of a heading's unit vector along the coarser of the two axes


def yaw_directions(spacings, n=90, span_deg=90.0):
    """The table of headings of the yaw search (DIRECTIONS of include/ext/occ4d_boxes.h), on the host: for theta_a = a * span / n,
    a = 0 .. n - 1, with m = max(sx, sy) and S = 2^14 the row (ax, ay, bx, by) = rint(S sx / m cos, S sy / m sin, -S sx / m sin,
    S sy / m cos): u = ax ix + ay iy is the world coordinate along the heading in units of m / S, v the one across it, so the
    search is exact in world space on an anisotropic grid.  A rectangle's extents repeat after 90 degrees (length and width swap),
    hence the default span.  -> dict(table (n, 4) int32, yaw (n,) float64 radians, unit float64 = m / S)."""
    sx, sy = float(spacings[0]), float(spacings[1])
    n = int(n)
    if not (sx > 0.0 and sy > 0.0 and np.isfinite(sx) and np.isfinite(sy)):
        raise ValueError('yaw_directions: spacings = %r must be positive' % (tuple(spacings),))
    if not 1 <= n <= _lib.BOXES_CONSTANTS['MAX_DIRS']:
        raise ValueError('yaw_directions: n = %r must lie in [1, %d]' % (n, _lib.BOXES_CONSTANTS['MAX_DIRS']))
    m = max(sx, sy)
    yaw = np.deg2rad(np.arange(n, dtype=np.float64) * (float(span_deg) / n))
    c, s = np.cos(yaw), np.sin(yaw)
    table = np.rint(np.stack([YAW_SCALE * sx / m * c, YAW_SCALE * sy / m * s, -YAW_SCALE * sx / m * s, YAW_SCALE * sy / m * c], axis=1))
    return dict(table=table.astype(np.int32), yaw=yaw, unit=m / YAW_SCALE)


class Boxes(products.GridProduct):
    """The option object of perform_inference(components=..., boxes=...) / evaluate_clip(..., boxes=...): the upright oriented box
    of every object of the product `of` ('components' or 'segments'), by a search over n headings of a quarter turn
    (yaw_directions over the grid's spacings) for the footprint rectangle of least area (include/ext/occ4d_boxes.h).  The product
    joins that product's dict: box (K, 8) int32 = [a*, min u, max u, min v, max v, min iz, max iz, points], dirs (n, 4) int32,
    with extents=True also extent (K, n, 4) int32.  K is the length of that dict's table: no host read of its own.
    oriented_boxes(box, dirs, mins, spacings) makes centre, size and yaw of it on the host."""
    keyword, reads_grid = 'boxes', False

    def __init__(self, of='components', n=90, extents=False):
        if of not in BOXES_OF:
            raise ValueError("Boxes: of = %r must be 'components' or 'segments'" % (of,))
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= _lib.BOXES_CONSTANTS['MAX_DIRS']:
            raise ValueError('Boxes: n = %r must be an integer in [1, %d]' % (n, _lib.BOXES_CONSTANTS['MAX_DIRS']))
        self.of = self.into = of
        self.n, self.extents = int(n), bool(extents)

    @classmethod
    def check(cls, option, given, point_sample_mode='grid'):
        """As GridProduct.check; the product it builds on is the instance's `of` (`needs` is a class attribute)."""
        super().check(option, given, point_sample_mode)
        if option.of not in BOXES_OF:
            raise ValueError("Boxes: of = %r must be 'components' or 'segments'" % (option.of,))
        if option.of not in given:
            raise ValueError("boxes needs %s=<a %s>: it fits a box to each of that product's objects"
                             % (option.of, 'components.Components' if option.of == 'components' else 'watershed.Segments'))

    def prepare(self, grid):
        return yaw_directions(grid.spacings, self.n)['table']

    def run(self, grid, table, made):
        of = made[self.of]
        dirs = torch.from_numpy(table).to(of['labels'].device)
        extent, zr = ops.grid_box_extents(of['labels'], grid.counts, of['table'].shape[0], dirs)
        out = dict(box=ops.boxes_choose(extent, zr, dirs), dirs=dirs)
        if self.extents:
            out['extent'] = extent
        return out

    def __repr__(self):
        return 'Boxes(of=%r, n=%d, extents=%r)' % (self.of, self.n, self.extents)


def oriented_boxes(box, dirs, mins, spacings):
    """World-space boxes from the rows of a Boxes product, on the host in float64: box (K, 8), dirs (A, 4) made by yaw_directions
    over the same spacings.  -> dict(centre (K, 3), size (K, 3) = length, width, height with length >= width, yaw (K,) in
    [-pi/2, pi/2): the heading of the length, points (K,) int64, fill (K,) = points / the box's volume in cells).  Rows with
    a* = -1 are NaN (points: what the row holds).  A point (ix, iy) lies at origin + (i + 0.5) * spacing; with e1 = (ax / sx, ay / sy) /
    |.| and e2 = (bx / sx, by / sy) / |.| the world unit vectors of a* and unit = max(sx, sy) / 2^14 the centre is origin + 0.5 *
    spacing + unit * (mid u * e1 + mid v * e2), the sizes are W1 * unit, W2 * unit (W of the header's CHOICE) and (max iz - min iz
    + 1) * sz."""
    b = np.asarray(box.cpu() if hasattr(box, 'cpu') else box).astype(np.int64)
    d = np.asarray(dirs.cpu() if hasattr(dirs, 'cpu') else dirs).astype(np.int64)
    assert b.ndim == 2 and b.shape[1] == _lib.BOXES_CONSTANTS['COLS'], 'box must be (K, 8), got %s' % (b.shape,)
    assert d.ndim == 2 and d.shape[1] == 4, 'dirs must be (A, 4), got %s' % (d.shape,)
    origin, spacing = np.asarray(mins, np.float64).reshape(3), np.asarray(spacings, np.float64).reshape(3)
    unit = max(spacing[0], spacing[1]) / YAW_SCALE
    K = b.shape[0]
    ok = (b[:, 0] >= 0) & (b[:, 0] < d.shape[0])
    row = d[np.where(ok, b[:, 0], 0)].astype(np.float64)                       # (K, 4)
    e1 = row[:, 0:2] / spacing[None, :2]                                        # (ax, ay) = S / m * (sx cos, sy sin)
    e2 = row[:, 2:4] / spacing[None, :2]
    with np.errstate(invalid='ignore', divide='ignore'):
        e1, e2 = e1 / np.linalg.norm(e1, axis=1, keepdims=True), e2 / np.linalg.norm(e2, axis=1, keepdims=True)
    w1 = (b[:, 2] - b[:, 1] + np.abs(d[np.where(ok, b[:, 0], 0), 0:2]).sum(1)).astype(np.float64) * unit
    w2 = (b[:, 4] - b[:, 3] + np.abs(d[np.where(ok, b[:, 0], 0), 2:4]).sum(1)).astype(np.float64) * unit
    mid_u, mid_v = 0.5 * (b[:, 1] + b[:, 2]) * unit, 0.5 * (b[:, 3] + b[:, 4]) * unit
    centre = np.empty((K, 3), np.float64)
    centre[:, :2] = origin[None, :2] + 0.5 * spacing[None, :2] + mid_u[:, None] * e1 + mid_v[:, None] * e2
    centre[:, 2] = origin[2] + (0.5 * (b[:, 5] + b[:, 6]) + 0.5) * spacing[2]
    height = (b[:, 6] - b[:, 5] + 1).astype(np.float64) * spacing[2]
    swap = w2 > w1                                                              # the length is the longer side
    head = np.where(swap[:, None], e2, e1)
    yaw = np.arctan2(head[:, 1], head[:, 0])
    yaw = (yaw + 0.5 * np.pi) % np.pi - 0.5 * np.pi                             # a box has no front: [-pi/2, pi/2)
    size = np.stack([np.where(swap, w2, w1), np.where(swap, w1, w2), height], axis=1)
    cells = size.prod(axis=1) / spacing.prod()
    with np.errstate(invalid='ignore', divide='ignore'):
        fill = b[:, 7].astype(np.float64) / cells
    for arr in (centre, size, yaw, fill):
        arr[~ok] = np.nan
    return dict(centre=centre, size=size, yaw=yaw, points=b[:, 7].copy(), fill=fill)


def tracks(objects, mins, spacings):
    """The trajectories, on the host in float64: `objects` is the list evaluate_clip(components=..., objects=[], tracker=...)
    appended one dict(labels, table, link) per output frame to.  -> {track id: dict(frames (T,) int64, components (T,) int64: the
    component's number in its frame, size (T,) int64, centroid (T, 3), box_min (T, 3), box_max (T, 3))}, the T frames in order.
    When every frame dict also holds box and dirs (evaluate_clip(..., boxes=Boxes())) a trajectory carries obox_centre (T, 3),
    obox_size (T, 3) and obox_yaw (T,) as well (oriented_boxes); differencing obox_centre over the frames gives a velocity."""
    rows = {}
    oriented = len(objects) > 0 and all('box' in frame and 'dirs' in frame for frame in objects)
    for t, frame in enumerate(objects):
        summary = boxes_and_centroids(frame['table'], mins, spacings)
        obox = oriented_boxes(frame['box'], frame['dirs'], mins, spacings) if oriented else None
        link = np.asarray(frame['link'])
        assert link.ndim == 2 and link.shape == (len(summary['size']), 4), 'link must be (K, 4), got %s' % (link.shape,)
        for k, track in enumerate(link[:, 0].tolist()):
            rows.setdefault(track, []).append((t, k, summary['size'][k], summary['centroid'][k], summary['box_min'][k], summary['box_max'][k])
                                              + ((obox['centre'][k], obox['size'][k], obox['yaw'][k]) if oriented else ()))
    out = {}
    for track, items in sorted(rows.items()):
        out[track] = dict(frames=np.array([i[0] for i in items], np.int64), components=np.array([i[1] for i in items], np.int64),
                          size=np.array([i[2] for i in items], np.int64), centroid=np.array([i[3] for i in items], np.float64).reshape(-1, 3),
                          box_min=np.array([i[4] for i in items], np.float64).reshape(-1, 3),
                          box_max=np.array([i[5] for i in items], np.float64).reshape(-1, 3))
        if oriented:
            out[track].update(obox_centre=np.array([i[6] for i in items], np.float64).reshape(-1, 3),
                              obox_size=np.array([i[7] for i in items], np.float64).reshape(-1, 3),
                              obox_yaw=np.array([i[8] for i in items], np.float64).reshape(-1))
    return out


def boxes_and_centroids(table, mins, spacings):
    """World-space summary of a component table (K, 12), on the host in float64: dict(size (K,) int64, klass (K,) int64, centroid
    (K, 3), box_min (K, 3), box_max (K, 3): the centres of the box's corner points).  Point i of axis a lies at (i + 0.5) *
    spacing_a + origin_a, so the centroid is (sum_a / size + 0.5) * spacing_a + origin_a."""
    t = np.asarray(table.cpu() if hasattr(table, 'cpu') else table)
    assert t.ndim == 2 and t.shape[1] == _lib.COMPONENTS_CONSTANTS['COLS'], 'table must be (K, 12), got %s' % (t.shape,)
    t = t.astype(np.int64, copy=False)
    origin, spacing = np.asarray(mins, np.float64).reshape(3), np.asarray(spacings, np.float64).reshape(3)
    size = t[:, 0]

    def world(index):
        return (index + 0.5) * spacing + origin

    return dict(size=size.copy(), klass=t[:, 2].copy(), centroid=world(t[:, 3:6].astype(np.float64) / size[:, None].astype(np.float64)),
                box_min=world(t[:, 6:9].astype(np.float64)), box_max=world(t[:, 9:12].astype(np.float64)))
