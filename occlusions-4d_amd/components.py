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
it on the host in float64 (boxes_and_centroids)."""
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


def tracks(objects, mins, spacings):
    """The trajectories, on the host in float64: `objects` is the list evaluate_clip(components=..., objects=[], tracker=...)
    appended one dict(labels, table, link) per output frame to.  -> {track id: dict(frames (T,) int64, components (T,) int64: the
    component's number in its frame, size (T,) int64, centroid (T, 3), box_min (T, 3), box_max (T, 3))}, the T frames in order."""
    rows = {}
    for t, frame in enumerate(objects):
        summary = boxes_and_centroids(frame['table'], mins, spacings)
        link = np.asarray(frame['link'])
        assert link.ndim == 2 and link.shape == (len(summary['size']), 4), 'link must be (K, 4), got %s' % (link.shape,)
        for k, track in enumerate(link[:, 0].tolist()):
            rows.setdefault(track, []).append((t, k, summary['size'][k], summary['centroid'][k], summary['box_min'][k], summary['box_max'][k]))
    out = {}
    for track, items in sorted(rows.items()):
        out[track] = dict(frames=np.array([i[0] for i in items], np.int64), components=np.array([i[1] for i in items], np.int64),
                          size=np.array([i[2] for i in items], np.int64), centroid=np.array([i[3] for i in items], np.float64).reshape(-1, 3),
                          box_min=np.array([i[4] for i in items], np.float64).reshape(-1, 3),
                          box_max=np.array([i[5] for i in items], np.float64).reshape(-1, 3))
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
