"""The decoded occupancy scanned by a virtual lidar (include/ext/occ4d_sweep.h, ops.sweep_rays): the field of a
point_sample_mode='grid' call as a spinning lidar at a given pose would measure it.

    FieldSweep         the option object of perform_inference(sweep=...) / evaluate_clip(sweep=..., sweeps=[])
    cast               the stand-alone piece: a dense (N, G) array, poses and directions -> the sweep's arrays
    lidar_directions   the direction table of a spinning lidar: channels x azimuths unit vectors, beam-major
    directions_to      the directions and ranges of the returns of a measured sweep: the bundle that replays it
    poses              sensor-to-world matrices -> the (V, 12) rows the entry point takes
    march_range        near, step, n_steps of the march for a grid and a set of poses
    rows_of            the returns as rows (x, y, z, cosine_angle, instance_id, semantic_tag, R, G, B), frontend.carla_clip's format
    residual           predicted - measured range per ray of a replayed sweep

Three uses.  The PREDICTED SWEEP: a range image (B, A) with class, object and colour per return.  REPLAY: for every return of a
measured sweep the range the model predicts along the same ray -- a predicted surface in front of a measured return is a
hallucination in observed free space, a predicted range behind it a miss; both are measured in the sensor's space, without
ground-truth occupancy.  ROLLOUT: the predicted sweep as rows in the loader's format.

What it is NOT: the march takes uniform samples and refines the first crossing linearly (the rules of the ray cast,
include/ext/occ4d_raycast.h), it is no exact intersection with the surface; there is no beam divergence, no intensity and no
drop-off model; `cos` is the non-negative cosine of the incidence angle, it does not say from which side the surface is met.
Binning a measured sweep into a range image, a sharded decode with `sweep`, and a rollout driver that feeds rows_of back through
frontend.carla_clip are out of scope."""
import numpy as np
import torch

from . import _lib, ops, products
from .projection import _device, _tensor

MAX_STEPS = _lib.SWEEP_CONSTANTS['MAX_STEPS']
MAX_CHANNELS = _lib.SWEEP_CONSTANTS['MAX_CHANNELS']
SWEEP_OF = (None, 'components', 'segments')
NO_RETURN = -1.0                 # `range` and `point` of a ray without a return: below every range the march can give (min_range >= 0)
ROW_COLUMNS = ('x', 'y', 'z', 'cos', 'inst', 'sem', 'c0', 'c1', 'c2', 'view')


def lidar_directions(channels, azimuths, upper_fov, lower_fov, azimuth_range=(-180.0, 180.0)):
    """The direction table of a spinning lidar: (channels * azimuths, 3) float32 unit vectors in the sensor frame (x forward, z up),
    beam-major (row b * azimuths + a).  The elevations run linearly from upper_fov to lower_fov (degrees, both included), the
    azimuths from azimuth_range[0] towards azimuth_range[1] without the end point.  Computed in float64 as (cos el cos az, cos el
    sin az, sin el), then rounded."""
    B, A = int(channels), int(azimuths)
    if B < 0 or A < 0:
        raise ValueError('lidar_directions: channels = %r, azimuths = %r must be >= 0' % (channels, azimuths))
    el = np.deg2rad(np.linspace(float(upper_fov), float(lower_fov), B, dtype=np.float64))[:, None]
    az = np.deg2rad(np.linspace(float(azimuth_range[0]), float(azimuth_range[1]), A, endpoint=False, dtype=np.float64))[None, :]
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=-1)
    return np.ascontiguousarray(d.reshape(B * A, 3), dtype=np.float32)


def directions_to(points, origin=(0.0, 0.0, 0.0)):
    """The bundle that replays a measured sweep: points (M, >= 3), the returns in the sensor frame (numpy or a tensor, read on the
    host) -> (dirs (M', 3) float32 unit vectors, ranges (M',) float32), computed in float64; the rows AT the origin are dropped."""
    p = points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else np.asarray(points)
    v = p[:, :3].astype(np.float64) - np.asarray(origin, np.float64)
    r = np.sqrt((v * v).sum(axis=1))
    keep = r > 0.0
    return np.ascontiguousarray(v[keep] / r[keep, None], dtype=np.float32), r[keep].astype(np.float32)


def _pose64(sensor_RT):
    m = sensor_RT.detach().cpu().numpy() if isinstance(sensor_RT, torch.Tensor) else np.asarray(sensor_RT)
    m = m.astype(np.float64)
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3 or tuple(m.shape[1:]) not in ((4, 4), (3, 4)):
        raise ValueError('sensor_RT must be (V, 4, 4) or (V, 3, 4), got %s' % (m.shape,))
    return np.ascontiguousarray(m[:, :3, :])


def poses(sensor_RT):
    """Sensor-to-world matrices (V, 4, 4) or (V, 3, 4) -> (V, 12) float32: row-major [Rm | t], what occ4d_sweep_rays_f32 takes."""
    return np.ascontiguousarray(_pose64(sensor_RT).reshape(-1, 12), dtype=np.float32)


def march_range(counts, mins, spacings, pose64, min_range=0.0, max_range=None, step=None):
    """(near, step, n_steps) of a sweep of the (nx, ny, nz) grid from the poses pose64 (V, 3, 4) float64, on the host in float64:
    near = min_range (>= 0), step = half the smallest spacing unless given, far = the smaller of max_range and the distance from a
    sensor to the farthest of the eight corners of the hull of the grid's points, n_steps = ceil((far - near) / step) + 1.
    ValueError when that exceeds the header's limit (or a value is not finite)."""
    counts, mins, spacings = [int(c) for c in counts], [float(m) for m in mins], [float(s) for s in spacings]
    if step is None:
        step = 0.5 * min(spacings)
    step, near = float(step), float(min_range)
    if not (step > 0.0 and np.isfinite(step)):
        raise ValueError('sweep: step = %r must be finite and > 0' % (step,))
    if not (near >= 0.0 and np.isfinite(near)):
        raise ValueError('sweep: min_range = %r must be finite and >= 0' % (min_range,))
    lo = [m + 0.5 * s for m, s in zip(mins, spacings)]
    hi = [m + (c - 0.5) * s for m, s, c in zip(mins, spacings, counts)]
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    t = np.asarray(pose64, np.float64).reshape(-1, 3, 4)[:, :, 3]
    far = float(np.sqrt(((corners[None] - t[:, None]) ** 2).sum(axis=-1)).max()) if len(t) else near
    if max_range is not None:
        limit = float(max_range)
        far = min(far, limit) if limit == limit else limit
    if not np.isfinite(far):
        raise ValueError('sweep: far = %r must be finite' % (far,))
    n_steps = int(np.ceil(max(far - near, 0.0) / step)) + 1
    if n_steps > MAX_STEPS:
        raise ValueError('sweep: n_steps = %d exceeds %d: (far - near) / step = (%g - %g) / %g' % (n_steps, MAX_STEPS, far, near, step))
    return near, step, n_steps


class FieldSweep(products.LevelProduct):
    """The option object of perform_inference(sweep=...) / evaluate_clip(sweep=..., sweeps=[]): the decoded field scanned by a
    virtual lidar (include/ext/occ4d_sweep.h).  poses: V sensor-to-world matrices (V, 4, 4) or (V, 3, 4) in the grid's world; dirs:
    the directions in the sensor frame, (R, 3) shared by the views or, with per_view, (V * R, 3) / (V, R, 3) (lidar_directions,
    directions_to: unit vectors, so that a range is a distance); shape = (B, A) with B * A = R, the ray image, default (1, R).
    level: the density of the surface met, None = the call's density_threshold; channels: the output columns sampled at the hit;
    select = (column, threshold) or None, as FieldViews; min_range / max_range / step: the march (march_range).  of: None,
    'components' or 'segments': that product's labels give `inst` (the product has to be given too).  With the call's
    predict_segmentation `sem` is the argmax of the last semantic_classes columns.  rows = (c0, c1, c2): three colour columns; the
    product then also holds the returns as rows.
    The product: result['sweep'] = dict(range (V, R) float32, -1 = no return; point (V, R, 3) float32; cell, owner (V, R) int32, -1 =
    no return; cos (V, R) float32[; sem (V, R) int32][; inst (V, R) int32]; features (V, R, C) float32[; rows (V * R, 10) float32 =
    (x, y, z, cos, inst, sem, c0, c1, c2, view) of the returns in ray order, the colours those of the OWNER grid point, inst / sem -1
    where there is none, the rows behind n_rows uninitialised; n_rows (1,) int32]; march (2,) float32 = [near, step]).  No device
    value is read: the count comes home with the arrays and rows_of trims.  inst == -1 can occur at a return (the header says
    when)."""
    keyword, clip_list = 'sweep', ('sweeps', 'one dict of sweep arrays')

    def __init__(self, poses, dirs, shape=None, per_view=False, level=None, channels=(), select=None, min_range=0.0, max_range=None,
                 step=None, of=None, rows=None):
        level = self._level(level)
        self.pose64 = _pose64(poses)
        self.poses = np.ascontiguousarray(self.pose64.reshape(-1, 12), dtype=np.float32)
        V = len(self.poses)
        d = dirs.detach().cpu().numpy() if isinstance(dirs, torch.Tensor) else np.asarray(dirs)
        if d.ndim not in (2, 3) or d.shape[-1] != 3:
            raise ValueError('FieldSweep: dirs must be (R, 3), (V * R, 3) or (V, R, 3), got %s' % (d.shape,))
        self.dirs = np.ascontiguousarray(d.reshape(-1, 3), dtype=np.float32)
        self.per_view = bool(per_view)
        D = len(self.dirs)
        if self.per_view:
            if V == 0 or D % V:
                raise ValueError('FieldSweep: per_view needs dirs of V * R rows, got %d rows for V = %d' % (D, V))
            R = D // V
        else:
            if d.ndim != 2:
                raise ValueError('FieldSweep: dirs (V, R, 3) need per_view=True, got %s' % (d.shape,))
            R = D
        if shape is None:
            shape = (1, R)
        try:
            B, A = (int(s) for s in shape)
        except (TypeError, ValueError):
            raise ValueError('FieldSweep: shape = %r must be (B, A)' % (shape,))
        if B < 0 or A < 0:
            raise ValueError('FieldSweep: shape = %r must be (B, A) with B, A >= 0' % (shape,))
        if B * A != R:
            raise ValueError('FieldSweep: shape = %r holds %d rays, dirs hold %d%s' % (shape, B * A, R, ' per view' if self.per_view else ''))
        if of not in SWEEP_OF:
            raise ValueError("FieldSweep: of = %r must be None, 'components' or 'segments'" % (of,))
        self.shape, self.level, self.channels = (B, A), level, tuple(int(c) for c in channels)
        self.select = None if select is None else (int(select[0]), float(select[1]))
        self.min_range, self.max_range, self.step, self.of = min_range, max_range, step, of
        self.rows = None if rows is None else tuple(int(c) for c in rows)
        if self.rows is not None and len(self.rows) != 3:
            raise ValueError('FieldSweep: rows = %r must be three colour columns' % (rows,))

    @classmethod
    def check(cls, option, given, point_sample_mode='grid'):
        """As GridProduct.check; the product it builds on is the instance's `of` (`needs` is a class attribute)."""
        super().check(option, given, point_sample_mode)
        if option.of not in SWEEP_OF:
            raise ValueError("FieldSweep: of = %r must be None, 'components' or 'segments'" % (option.of,))
        if option.of is not None and option.of not in given:
            raise ValueError("sweep needs %s=<a %s>: its labels give the object of a return"
                             % (option.of, 'components.Components' if option.of == 'components' else 'watershed.Segments'))

    def prepare(self, grid):
        return (self.resolve(grid.density_threshold),
                march_range(grid.counts, grid.mins, grid.spacings, self.pose64, self.min_range, self.max_range, self.step))

    def run(self, grid, prepared, made):
        level, march = prepared
        labels, k = None, 0
        if self.of is not None:
            labels, k = made[self.of]['labels'], made[self.of]['table'].shape[0]
        sem = None
        if grid.predict_segmentation and grid.semantic_classes > 0:
            sem = (grid.output.shape[1] - grid.semantic_classes, grid.semantic_classes)
        return self.sweep(grid.output, grid.counts, grid.mins, grid.spacings, level, march, labels=labels, k=k, sem=sem)

    def sweep(self, implicit_output, counts, mins, spacings, level, march, channel=0, labels=None, k=0, sem=None):
        """-> the product's dict for implicit_output (N, G) on its device; march = (near, step, n_steps)."""
        out = implicit_output
        near, step, n_steps = march
        field, mask, threshold = products.columns(out, channel, self.select)
        if mask is not None:
            field = torch.where(mask >= threshold, field, torch.zeros((), dtype=out.dtype, device=out.device))
        pose, dirs = (torch.from_numpy(m).to(out.device) for m in (self.poses, self.dirs))
        res = ops.sweep_rays(field, counts, mins, spacings, level, pose, dirs, self.shape, near, step, n_steps, per_view=self.per_view,
                             attrs=out, channels=self.channels, sem=sem, labels=labels, k=k, background=NO_RETURN)
        if self.rows is not None:
            res['rows'], res['n_rows'] = self._rows(out, res)
        res['march'] = torch.tensor([near, step], dtype=torch.float32).to(out.device)
        return res

    def _rows(self, out, res):
        """The dense (V * R, 10) rows, compacted in ray order by the key `range` (>= 0: a return) -> (buffer, count (1,) int32)."""
        V, R = res['range'].shape
        n = V * R
        for c in self.rows:
            assert 0 <= c < out.shape[1], 'rows column = %r' % (c,)
        f32 = lambda t: t.reshape(n, 1).to(torch.float32)
        none = torch.full((n, 1), -1.0, dtype=torch.float32, device=out.device)
        hit = res['owner'].reshape(n) >= 0
        own = torch.where(hit, res['owner'].reshape(n), torch.zeros((), dtype=torch.int32, device=out.device)).to(torch.int64)
        colour = out.index_select(0, own)[:, list(self.rows)] if out.shape[0] else out.new_zeros((n, 3))
        view = torch.arange(V, dtype=torch.float32, device=out.device).repeat_interleave(R).reshape(n, 1)
        dense = torch.cat([res['point'].reshape(n, 3), f32(res['cos']), f32(res['inst']) if 'inst' in res else none,
                           f32(res['sem']) if 'sem' in res else none, colour, view], dim=1)
        return ops.compact_rows_nosync(dense, res['range'].reshape(n), 0.0, strict=False)

    def __repr__(self):
        return 'FieldSweep(V=%d, shape=%r, per_view=%r, level=%r, channels=%r, select=%r, min_range=%r, max_range=%r, step=%r, of=%r, rows=%r)' % (
            len(self.poses), self.shape, self.per_view, self.level, self.channels, self.select, self.min_range, self.max_range, self.step,
            self.of, self.rows)


def cast(implicit_output, counts, mins, spacings, poses, dirs, level, shape=None, per_view=False, channel=0, channels=(), select=None,
         min_range=0.0, max_range=None, step=None, sem=None, labels=None, k=0, rows=None):
    """The stand-alone piece of FieldSweep: implicit_output (N, G) on the (nx, ny, nz) = `counts` grid whose points ops.grid_points
    made from `mins` / `spacings` (geometry.grid_frame), scanned from `poses` along `dirs` (the arguments of FieldSweep).  sem =
    (first class column, number of classes) or None; labels (n,) int32 of k objects or None.  -> the dict of device tensors
    FieldSweep describes (the rules in include/ext/occ4d_sweep.h; the march's defaults in march_range).  Poses and directions are
    taken on the host; no device value is read."""
    level = float(level)
    if level != level:
        raise ValueError('sweep.cast: level is NaN')
    option = FieldSweep(poses, dirs, shape, per_view, level, channels, select, min_range, max_range, step, rows=rows)
    device = _device(implicit_output)
    out = _tensor(implicit_output, device, 'implicit_output')
    if labels is not None:
        lab = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32))
        labels = lab.to(device=device, dtype=torch.int32)
    march = march_range(counts, mins, spacings, option.pose64, min_range, max_range, step)
    return option.sweep(out, counts, mins, spacings, level, march, channel, labels=labels, k=k, sem=sem)


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def rows_of(result):
    """The returns of a sweep made with rows=(c0, c1, c2) -- a perform_inference result or its 'sweep' dict -- as the loader's rows:
    -> (rows (M, 9) float32 = (x, y, z, cosine_angle, instance_id, semantic_tag, c0, c1, c2), views (M,) int32), in ray order,
    trimmed to n_rows.  The points are in the grid's world; instance_id and semantic_tag are carried as floats, -1 where the sweep
    has none."""
    sw = result['sweep'] if 'sweep' in result else result
    if 'rows' not in sw:
        raise ValueError('rows_of needs a sweep made with rows=(c0, c1, c2)')
    rows, n = _host(sw['rows']), int(_host(sw['n_rows']).reshape(-1)[0])
    return np.ascontiguousarray(rows[:n, :9], dtype=np.float32), rows[:n, 9].astype(np.int32)


def residual(range, hit, measured):
    """predicted - measured per ray of a replayed sweep: range = the sweep's predicted ranges, hit = which rays have a predicted
    return (cell >= 0), measured = the ranges directions_to gave, of one shape.  NaN marks a ray with no predicted return; negative:
    the model puts a surface in front of the measured return, positive: behind it.  torch tensors give a tensor, numpy gives numpy."""
    if isinstance(range, torch.Tensor):
        m = measured if isinstance(measured, torch.Tensor) else torch.as_tensor(np.asarray(measured, np.float32))
        h = hit if isinstance(hit, torch.Tensor) else torch.as_tensor(np.asarray(hit, bool))
        return torch.where(h.to(range.device), range - m.to(device=range.device, dtype=range.dtype).reshape(range.shape),
                           torch.full((), float('nan'), dtype=range.dtype, device=range.device))
    r = np.asarray(range, np.float32)
    return np.where(np.asarray(hit, bool), r - np.asarray(measured, np.float32).reshape(r.shape), np.float32('nan')).astype(np.float32)
