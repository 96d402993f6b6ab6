"""The distance transform of the decoded occupancy on the dense query grid, on the device (include/ext/occ4d_distance.h): how far
every query is from the nearest predicted solid -- the clearance --, from ONE decode.

perform_inference(clearance=Clearance()) adds result['clearance'] = dict(dist2 (N,) int32[, nearest (N,) int32][, inside2 (N,)
int32]): per query the exact squared distance to the nearest query whose density is >= level, in grid steps; with nearest=True the
flat index of that query; with inside=True also the squared distance to the nearest query that is NOT solid: the depth inside.

    res = perform_inference(..., point_sample_mode='grid', clearance=Clearance(nearest=True, inside=True), components=Components())
    c = res['clearance']
    sdf = signed(torch.from_numpy(c['dist2']), torch.from_numpy(c['inside2']), unit)      # < 0 inside the solid
    region = expand_labels(torch.from_numpy(res['components']['labels']), torch.from_numpy(c['nearest']))

WEIGHTS.  The cost of a step of d points along an axis is weight * d^2, an integer, so every result is the same bit for bit under
any scheduling.  The default (1, 1, 1) measures in voxels: metric(dist2, unit) with the grid's spacing as `unit` is the distance in
world units when the three spacings are equal.  The project's grids are anisotropic by under 1 % (geometry.grid_frame: each axis
divides its own extent by its own count); integer weights proportional to the SQUARED spacings -- (wx, wy, wz) = (sx^2, sy^2, sz^2)
/ u^2 rounded, for a small unit u -- make the metric exact in units of u, within the bound of the header (the largest cost must
stay below 2^31 - 1).  `nearest` gives the site itself: the float64 world-space vector to it is one subtraction of two rows of
points_query, whatever the weights."""
import numpy as np
import torch

from . import _lib, ops, products

NONE = _lib.DISTANCE_CONSTANTS['NONE']


def _weights(weights, who):
    try:
        w = tuple(weights)
    except TypeError:
        w = ()
    if len(w) != 3 or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 1 <= x <= 2 ** 31 - 1 for x in w):
        raise ValueError('%s: weights = %r must be three integers >= 1' % (who, weights))
    return tuple(int(x) for x in w)


class Clearance(products.LevelProduct):
    """The option object of perform_inference(clearance=...) / evaluate_clip(clearance=..., clearances=[]).  level: the density from
    which a query is solid (density >= level, the comparison of the solid split), None = the call's density_threshold; select =
    (column, threshold) or None: solid queries also need implicit_output[:, column] >= threshold (with the track channel: the
    tracked object alone); weights: three integers >= 1 (the module's doc-string); nearest: also the flat index of the nearest
    solid query; inside: also inside2, the squared distance to the nearest query that is not solid.  The product: dict(dist2 (N,)
    int32[, nearest (N,) int32][, inside2 (N,) int32]) (transform); no device value is read."""
    keyword, clip_list = 'clearance', ('clearances', 'one dict of distances')

    def __init__(self, level=None, select=None, weights=(1, 1, 1), nearest=False, inside=False):
        self.level, self.weights = self._level(level), _weights(weights, 'Clearance')
        self.select = None if select is None else (int(select[0]), float(select[1]))
        self.nearest, self.inside = bool(nearest), bool(inside)

    def run(self, grid, level, made):
        return transform(grid.output, grid.counts, level, self.select, self.weights, self.nearest, self.inside)

    def __repr__(self):
        return 'Clearance(level=%r, select=%r, weights=%r, nearest=%r, inside=%r)' % (
            self.level, self.select, self.weights, self.nearest, self.inside)


def transform(implicit_output, counts, level, select=None, weights=(1, 1, 1), nearest=False, inside=False, channel=0):
    """The distance transform of column `channel` of a dense (N, G) output on the (nx, ny, nz) = `counts` grid at `level`.  select =
    (column, threshold): the mask column.  -> dict(dist2 (N,) int32[, nearest (N,) int32][, inside2 (N,) int32]) on the device.  No
    host read."""
    level = float(level)
    if level != level:
        raise ValueError('distance.transform: level is NaN')
    weights = _weights(weights, 'distance.transform')
    values, mask, mask_level = products.columns(implicit_output, channel, select)
    dist2, site = ops.grid_distance(values, counts, level, weights, 0, mask, mask_level, nearest)
    result = dict(dist2=dist2)
    if nearest:
        result['nearest'] = site
    if inside:
        result['inside2'] = ops.grid_distance(values, counts, level, weights, 1, mask, mask_level, False)[0]
    return result


def metric(dist2, unit=1.0):
    """sqrt(dist2) * unit as float32 on dist2's device (the root in float64, rounded once); inf where dist2 is NONE."""
    assert dist2.dtype == torch.int32, 'dist2 must be torch.int32, got %s' % (dist2.dtype,)
    d = torch.sqrt(dist2.to(torch.float64)) * float(unit)
    return torch.where(dist2 == NONE, torch.full_like(d, float('inf')), d).to(torch.float32)


def signed(dist2, inside2, unit=1.0):
    """The signed distance, outside minus inside: metric(dist2) - metric(inside2), > 0 in free space and < 0 inside the solid
    (one of the two is 0 at every point); +inf / -inf where there is no solid / nothing but solid."""
    assert dist2.shape == inside2.shape, 'dist2 %s and inside2 %s differ in shape' % (tuple(dist2.shape), tuple(inside2.shape))
    return metric(dist2, unit) - metric(inside2, unit)


def expand_labels(labels, nearest):
    """labels (N,) int32 (components.label), nearest (N,) int32 -> (N,) int32: the component of each point's nearest solid, -1 where
    there is none: the Voronoi regions of the components.  One gather."""
    assert labels.dim() == 1 and nearest.shape == labels.shape and nearest.dtype == torch.int32, \
        'labels and nearest must be (N,) with nearest int32, got %s and %s' % (tuple(labels.shape), tuple(nearest.shape))
    if labels.shape[0] == 0:
        return labels.clone()
    has = nearest >= 0
    return torch.where(has, labels[nearest.clamp(min=0).to(torch.int64)], torch.full_like(labels, -1))
