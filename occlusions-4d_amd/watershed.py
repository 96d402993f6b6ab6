"""Touching objects of the decoded occupancy split at their necks, on the device (include/ext/occ4d_watershed.h): the watershed
segments of the depth map of the solid set, from ONE decode.

components.label calls two objects that touch one component.  The depth of the solid -- distance.Clearance(inside=True)'s inside2,
the exact squared distance of every solid query to the nearest query that is not solid -- is large in the middle of a thick part
and small in a neck: every solid query climbs to its deepest neighbour until a maximum, the queries of one maximum are a basin,
and two basins are one segment when the deepest point of the neck between them lies within `h` of the shallower maximum.

perform_inference(segments=Segments(h=...)) adds result['segments'] = dict(labels (N,) int32, table (K, 12) int64, peaks (K, 2)
int32): per query the number of its segment (-1: air, or a segment smaller than min_size); per segment the row of a components
table (size, root, -1, coordinate sums, minima, maxima) and the flat index and the depth of its deepest query.  Segments are
numbered in the order of their lowest flat index.  With h at or above the largest depth the segments are the components.

    res = perform_inference(..., point_sample_mode='grid', segments=Segments(h=4, min_size=20))
    s = res['segments']
    objects = components.boxes_and_centroids(s['table'], frame[1], frame[2])               # as for components
    region = distance.expand_labels(labels, nearest)                                       # the segments' Voronoi regions
    link = components.Tracker().add_frame(labels, table)                                   # frame after frame, by hand

Everything is an integer, so every output is the same bit for bit under any scheduling.

H.  `h` is in units of SQUARED weighted grid steps, the units of inside2, and has no default: which necks separate two objects
depends on the fields a trained model produces, and NO VALUE HAS BEEN MEASURED ON A TRAINED MODEL.  h = 0 splits at every neck,
however shallow (plateaus are still one segment); a large h merges everything that touches."""
import numpy as np

from . import components, distance, ops, products

H_MAX = 2 ** 31 - 1


def _h(h, who):
    if isinstance(h, bool) or not isinstance(h, (int, np.integer)) or not 0 <= h <= H_MAX:
        raise ValueError('%s: h = %r must be an integer in [0, 2^31 - 1]' % (who, h))
    return int(h)


def _connectivity(connectivity, who):
    if isinstance(connectivity, bool) or connectivity not in components.CONNECTIVITIES:
        raise ValueError('%s: connectivity = %r must be 6, 18 or 26' % (who, connectivity))
    return int(connectivity)


def _min_size(min_size, who):
    if isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer)) or not 1 <= min_size <= 2 ** 31 - 1:
        raise ValueError('%s: min_size = %r must be an integer >= 1' % (who, min_size))
    return int(min_size)


class Segments(products.LevelProduct):
    """The option object of perform_inference(segments=...) / evaluate_clip(segments=..., parts=[]).  h: the tolerance of the merge,
    an integer in [0, 2^31 - 1] in units of squared weighted grid steps; required: no value has been measured on a trained model
    (the module's doc-string).  level: the density from which a query is solid (density >= level, the comparison of the solid
    split), None = the call's density_threshold; select = (column, threshold) or None: solid queries also need
    implicit_output[:, column] >= threshold; weights: three integers >= 1, the metric of the depth (distance.py); connectivity: 6,
    18 or 26; min_size: segments of fewer points are dropped.  The product: dict(labels (N,) int32, table (K, 12) int64, peaks
    (K, 2) int32) (split); it computes its own inside2 and needs no other product; one 16-byte device->host read sizes table and
    peaks.  In track_mode 'all' the segments are those of the merged array, under `refine` those of the expanded one."""
    keyword, clip_list = 'segments', ('parts', 'one dict of labels, table and peaks')

    def __init__(self, h, level=None, select=None, weights=(1, 1, 1), connectivity=26, min_size=1):
        self.h, self.level = _h(h, 'Segments'), self._level(level)
        self.weights = distance._weights(weights, 'Segments')
        self.connectivity, self.min_size = _connectivity(connectivity, 'Segments'), _min_size(min_size, 'Segments')
        try:
            self.select = None if select is None else (int(select[0]), float(select[1]))
        except (TypeError, IndexError) as e:
            raise ValueError('Segments: select = %r must be (column, threshold) or None' % (select,)) from e

    def run(self, grid, level, made):
        labels, table, peaks = split(grid.output, grid.counts, level, self.h, self.select, self.weights, self.connectivity, self.min_size)
        return dict(labels=labels, table=table, peaks=peaks)

    def __repr__(self):
        return 'Segments(h=%d, level=%r, select=%r, weights=%r, connectivity=%d, min_size=%d)' % (
            self.h, self.level, self.select, self.weights, self.connectivity, self.min_size)


def split(implicit_output, counts, level, h, select=None, weights=(1, 1, 1), connectivity=26, min_size=1, channel=0):
    """The watershed segments of the set column `channel` >= level of a dense (N, G) output on the (nx, ny, nz) = `counts` grid:
    ops.grid_distance(..., target=1), the depth of every solid query, then ops.grid_watershed of it.  select = (column,
    threshold): the mask column.  -> (labels (N,) int32, table (K, 12) int64, peaks (K, 2) int32) on the device; one 16-byte
    device->host read (the totals) sizes table and peaks."""
    level = float(level)
    if level != level:
        raise ValueError('watershed.split: level is NaN')
    h, weights = _h(h, 'watershed.split'), distance._weights(weights, 'watershed.split')
    connectivity, min_size = _connectivity(connectivity, 'watershed.split'), _min_size(min_size, 'watershed.split')
    values, mask, mask_level = products.columns(implicit_output, channel, select)
    inside2 = ops.grid_distance(values, counts, level, weights, 1, mask, mask_level, False)[0]
    labels, _, table, peaks = ops.grid_watershed(inside2, counts, h, connectivity, min_size)
    return labels, table, peaks
