"""Clouds into camera views on the device (include/occ4d_project.h): the projection of the reference's
``pixel_coords_from_point_cloud`` (utils/geometry.py:67-115, the exact inverse of the unprojection the clip front end restates),
a z-buffer over it, and the per-point visibility test against a depth image.

``render_views`` turns a cloud -- the decoded solid rows, an input or a target cloud -- into depth, index and feature images
under a clip's cameras, to be put beside the RGB-D frames the cloud came from.  ``visibility`` gives the partition of target
points the model is scored on: VISIBLE from a camera, OCCLUDED from it, or OUTSIDE its frustum; ``evaluation.evaluate_clip(
stats_occlusion=...)`` feeds it to ``EvalStats`` as the group of every target point.  Where a data set has no depth image (CARLA),
``render_views`` of the forward sweep gives one.

``render_field`` shows the decoded field itself instead of a cloud: the dense (N, G) output of a grid decode ray-cast into the
cameras (include/ext/occ4d_raycast.h, csrc/raycast.hip) -- the depth of the surface density == level, the mask of what was hit, and
output columns sampled at the hit; ``FieldViews`` is its option object for ``perform_inference(views=...)``.

The cloud functions run in the four kernels of csrc/project.hip; clouds, cameras and images stay on the device and none of them
reads a device value on the host (render_field inverts its cameras on the host: cameras given as device tensors are read once).
The arithmetic equals the reference's numpy results bit for bit (tests/golden/project_*.npz).
"""
import numpy as np
import torch

from . import _lib, ops, products

VISIBLE, OCCLUDED, OUTSIDE = 0, 1, 2


def _device(like=None):
    if _lib.is_twin():
        return torch.device('cpu')
    if isinstance(like, torch.Tensor) and like.is_cuda:
        return like.device
    return torch.device('cuda', torch.cuda.current_device())


def _tensor(a, device, name):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) if not isinstance(a, torch.Tensor) else a
    return t.to(device=device, dtype=torch.float32)


def expand_cameras(cam_RT, cam_K, device):
    """The reference's expanded matrices of V cameras, built with tensor operations only (no host read of a device value):
    cam_RT (V, 3, 4) or (3, 4), cam_K (3, 3) or (V, 3, 3) -> (rt, k), both (V, 4, 4) fp32 on `device`: eye(4) with the
    extrinsics in the first three rows / the intrinsics in the upper left corner."""
    RT, K = _tensor(cam_RT, device, 'cam_RT'), _tensor(cam_K, device, 'cam_K')
    if RT.dim() == 2:
        RT = RT[None]
    assert RT.dim() == 3 and tuple(RT.shape[1:]) == (3, 4), 'cam_RT must be (V, 3, 4) or (3, 4), got %s' % (tuple(RT.shape),)
    V = RT.shape[0]
    if K.dim() == 2:
        K = K[None].expand(V, 3, 3)
    assert tuple(K.shape) == (V, 3, 3), 'cam_K must be (3, 3) or (V = %d, 3, 3), got %s' % (V, tuple(K.shape))
    rt = torch.eye(4, dtype=torch.float32, device=device).repeat(V, 1, 1)
    k = rt.clone()
    rt[:, :3, :] = RT
    k[:, :3, :3] = K
    return rt, k


def pixel_coords_from_point_cloud(pcl, cam_RT, cam_K, flip_xy=False):
    """The reference's function of that name, arguments and result: pcl (N, D) world coordinates + features, cam_RT (3, 4), cam_K
    (3, 3) -> (N, D) float32 = pixel x, y (y, x with flip_xy), depth, then the features.  A tensor gives a tensor on its device,
    numpy gives numpy.  Points behind the camera are not filtered."""
    as_numpy = not isinstance(pcl, torch.Tensor)
    device = _device(pcl)
    rows = _tensor(pcl, device, 'pcl')
    assert rows.dim() == 2 and rows.shape[1] >= 3, 'pcl must be (N, D >= 3), got %s' % (tuple(rows.shape),)
    rt, k = expand_cameras(cam_RT, cam_K, device)
    assert rt.shape[0] == 1, 'pixel_coords_from_point_cloud takes one camera'
    out = torch.cat([ops.project_points(rows, rt, k, flip_xy)[0], rows[:, 3:]], dim=1)
    if as_numpy:
        return out.cpu().numpy()
    return out if pcl.device == out.device else out.to(pcl.device)


def render_views(pcl, cam_RT, cam_K, height, width, channels=(), radius=0, background=0.0):
    """Z-buffered images of the cloud pcl (N, D) under V cameras (cam_RT (V, 3, 4), cam_K (3, 3) or (V, 3, 3)): a dict of device
    tensors, 'depth' (V, H, W) fp32 (`background` where nothing projects: with the default 0, depth > 0 means valid, as in the
    front end's frames), 'index' (V, H, W) int32 (the row a pixel shows, -1 = none) and 'features' (V, H, W, C): the columns
    `channels` of that row (`background` where none).  Every point covers the (2 radius + 1)^2 pixels around its own; the nearest
    point wins a pixel, the lowest row among equal depths.  No host read."""
    device = _device(pcl)
    rows = _tensor(pcl, device, 'pcl')
    assert rows.dim() == 2 and rows.shape[1] >= 3, 'pcl must be (N, D >= 3), got %s' % (tuple(rows.shape),)
    rt, k = expand_cameras(cam_RT, cam_K, device)
    keys = ops.zbuffer_splat(rows, rt, k, height, width, radius)
    depth, index, feat = ops.zbuffer_resolve(keys, rows, channels, background)
    return dict(depth=depth, index=index, features=feat)


def visibility(points, depth, cam_RT, cam_K, margin):
    """(V, N) int32 codes of the points (N, >= 3) against the depth images (V, H, W) (or (H, W) with one camera) of the cameras
    cam_RT / cam_K: VISIBLE, OCCLUDED (the image holds a depth d > 0 at the point's pixel and the point lies more than `margin`
    behind it) or OUTSIDE (behind the camera or off the image).  On the device; no host read."""
    device = _device(points)
    rows = _tensor(points, device, 'points')
    assert rows.dim() == 2 and rows.shape[1] >= 3, 'points must be (N, >= 3), got %s' % (tuple(rows.shape),)
    rt, k = expand_cameras(cam_RT, cam_K, device)
    dep = _tensor(depth, device, 'depth')             # (a device tensor stays the view it is: strided images are read in place)
    if dep.dim() == 2:
        dep = dep[None]
    return ops.visibility(rows, rt, k, dep, margin)


# ---------------------------------------------------------------------------------------------------------------- the decoded field
MAX_STEPS = _lib.RAYCAST_CONSTANTS['MAX_STEPS']        # the header's limit on n_steps (include/ext/occ4d_raycast.h)


def invert_cameras(cam_RT, cam_K):
    """The inverses of the expanded 4 x 4 matrices of V cameras, (rt_inv, k_inv), both (V, 4, 4) float32 numpy: inverted on the
    HOST in float64 and rounded once -- 2 V 16 numbers that are known before any decode; nothing here depends on a device solver
    library.  Also returns the float64 expanded rt (V, 4, 4) (the depth of a world point is its row 2).  Device tensors are read
    to the host: one small read."""
    def host(a):
        return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    RT, K = host(cam_RT), host(cam_K)
    if RT.ndim == 2:
        RT = RT[None]
    assert RT.ndim == 3 and RT.shape[1:] == (3, 4), 'cam_RT must be (V, 3, 4) or (3, 4), got %s' % (RT.shape,)
    V = RT.shape[0]
    if K.ndim == 2:
        K = np.broadcast_to(K[None], (V, 3, 3))
    assert K.shape == (V, 3, 3), 'cam_K must be (3, 3) or (V = %d, 3, 3), got %s' % (V, K.shape)
    rt, k = np.tile(np.eye(4), (V, 1, 1)), np.tile(np.eye(4), (V, 1, 1))
    rt[:, :3, :], k[:, :3, :3] = RT, K
    return np.linalg.inv(rt).astype(np.float32), np.linalg.inv(k).astype(np.float32), rt


def march_range(counts, mins, spacings, rt64, near=None, far=None, step=None):
    """(near, step, n_steps) of a ray cast of the (nx, ny, nz) grid under the cameras rt64 (V, 4, 4) float64.  Defaults: step =
    half the smallest spacing; near / far = the smallest / largest depth of the eight corners of the hull of the grid's points
    under any of the cameras, near not below step; n_steps = ceil((far - near) / step) + 1.  ValueError when that exceeds the
    header's limit (or the range is not finite)."""
    counts, mins, spacings = [int(c) for c in counts], [float(m) for m in mins], [float(s) for s in spacings]
    if step is None:
        step = 0.5 * min(spacings)
    step = float(step)
    if not (step > 0.0 and np.isfinite(step)):
        raise ValueError('render_field: step = %r must be finite and > 0' % (step,))
    lo = [m + 0.5 * s for m, s in zip(mins, spacings)]
    hi = [m + (c - 0.5) * s for m, s, c in zip(mins, spacings, counts)]
    corners = np.array([[x, y, z, 1.0] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    depths = np.einsum('vj,cj->vc', rt64[:, 2, :], corners) if len(rt64) else np.zeros((1, 1))
    near = max(float(depths.min()), step) if near is None else float(near)
    far = float(depths.max()) if far is None else float(far)
    if not (np.isfinite(near) and np.isfinite(far)):
        raise ValueError('render_field: near = %r, far = %r must be finite' % (near, far))
    n_steps = int(np.ceil(max(far - near, 0.0) / step)) + 1
    if n_steps > MAX_STEPS:
        raise ValueError('render_field: n_steps = %d exceeds %d: (far - near) / step = (%g - %g) / %g' % (n_steps, MAX_STEPS, far, near, step))
    return near, step, n_steps


class FieldViews(products.LevelProduct):
    """The option object of perform_inference(views=...) / evaluate_clip(views=..., images=[]): the cameras cam_RT (V, 3, 4), cam_K
    (3, 3) or (V, 3, 3) and the image size the decoded field is ray-cast into (render_field).  level: the density of the surface
    shown, None = the call's density_threshold; channels: the output columns sampled at the hit; select = (column, threshold) or
    None; step: the march's step in depth, None = half the smallest grid spacing.  The cameras are inverted here, once, on the host.
    The product: dict(depth (V, H, W) float32, cell (V, H, W) int32, features (V, H, W, C) float32); no device value is read."""
    keyword, clip_list = 'views', ('images', 'one dict of images')

    def __init__(self, cam_RT, cam_K, height, width, level=None, channels=(), select=None, step=None):
        level = self._level(level)
        self.rt_inv, self.k_inv, self.rt64 = invert_cameras(cam_RT, cam_K)
        self.height, self.width = int(height), int(width)
        if self.height < 0 or self.width < 0:
            raise ValueError('FieldViews: height = %r, width = %r' % (height, width))
        self.level, self.channels, self.step = level, tuple(int(c) for c in channels), step
        self.select = None if select is None else (int(select[0]), float(select[1]))

    def run(self, grid, level, made):
        return dict(zip(('depth', 'cell', 'features'), self.render(grid.output, grid.counts, grid.mins, grid.spacings, level)))

    def render(self, implicit_output, counts, mins, spacings, level, channel=0, near=None, far=None, background=0.0):
        """-> (depth, cell, features) of implicit_output (N, G) on its device."""
        out = implicit_output
        field, mask, threshold = products.columns(out, channel, self.select)
        if mask is not None:
            field = torch.where(mask >= threshold, field, torch.zeros((), dtype=out.dtype, device=out.device))
        near, step, n_steps = march_range(counts, mins, spacings, self.rt64, near, far, self.step)
        rt_inv, k_inv = (torch.from_numpy(m).to(out.device) for m in (self.rt_inv, self.k_inv))
        return ops.raycast_grid(field, counts, mins, spacings, level, rt_inv, k_inv, self.height, self.width, near, step, n_steps,
                                attrs=out, channels=self.channels, background=background)

    def __repr__(self):
        return 'FieldViews(V=%d, height=%d, width=%d, level=%r, channels=%r, select=%r, step=%r)' % (
            len(self.rt_inv), self.height, self.width, self.level, self.channels, self.select, self.step)


def render_field(implicit_output, counts, mins, spacings, cam_RT, cam_K, height, width, level, channel=0, channels=(), select=None,
                 near=None, far=None, step=None, background=0.0):
    """The decoded field itself in V camera views (include/ext/occ4d_raycast.h): per pixel the first crossing of
    implicit_output[:, channel] == level along the pixel's ray through the (nx, ny, nz) = `counts` grid whose points
    ops.grid_points made from `mins` / `spacings` (geometry.grid_frame).  -> dict of device tensors: 'depth' (V, H, W) fp32
    (`background` where the ray meets no surface), 'cell' (V, H, W) int32 (the flat index of the hit cell's low corner, -1 =
    none: cell >= 0 is the mask) and 'features' (V, H, W, C): the columns `channels` of implicit_output, trilinear at the hit.
    select = (column, threshold): the field is where(implicit_output[:, column] >= threshold, implicit_output[:, channel], 0);
    with column = the track channel it shows the tracked object alone: its amodal depth and mask.
    The march: samples at depths near + i * step; defaults in march_range.  The cameras are inverted on the host in float64
    (invert_cameras); cameras given as device tensors cost one small device->host read, nothing else is read."""
    level = float(level)
    if level != level:
        raise ValueError('render_field: level is NaN')
    device = _device(implicit_output)
    views = FieldViews(cam_RT, cam_K, height, width, level, channels, select, step)
    depth, cell, feat = views.render(_tensor(implicit_output, device, 'implicit_output'), counts, mins, spacings, level, channel, near,
                                     far, background)
    return dict(depth=depth, cell=cell, features=feat)


# ---------------------------------------------------------------------------------------------------------------- object layers
LAYERS_OF = ('components', 'segments')
MAX_LAYERS = _lib.LAYERS_CONSTANTS['MAX']              # the header's limit on max_layers (include/ext/occ4d_layers.h)
LAYER_PIXEL_ARRAYS = ('label', 'first', 'samples', 'point', 'count')
# the columns of the table (not the visibility codes above)
LAYER_COLUMNS = {c: _lib.LAYERS_CONSTANTS[c] for c in ('AMODAL', 'VISIBLE', 'NEAR', 'XMIN', 'XMAX', 'YMIN', 'YMAX')}


class ObjectLayers(products.GridProduct):
    """The option object of perform_inference(components=..., layers=...) / evaluate_clip(..., layers=..., layer_images=[]): the
    objects of the product `of` ('components' or 'segments') as depth layers in the views of the cameras cam_RT (V, 3, 4), cam_K
    (3, 3) or (V, 3, 3) (include/ext/occ4d_layers.h).  Per pixel the objects its ray passes through in the order it first enters
    them, at most max_layers of them: layer 0 is the object seen there, the later ones are those behind it -- the amodal masks,
    the visible masks and who hides whom.  step: the march's step in depth, None = half the smallest grid spacing (march_range);
    arrays: which of the per-pixel arrays label, first, samples, point (V, H, W, L) and count (V, H, W) come back.  The cameras are
    inverted here, once, on the host.  The product: result['layers'] = dict(<those arrays>, table (V, K, 7) int32 = [amodal
    pixels, visible pixels, least first, xmin, xmax, ymin, ymax] per view and object, status (2,) int32 = [pixels that dropped an
    object, pixels with any object], march (2,) float32 = [near, step]).  K is the length of that product's table: no host read
    of its own.  With status[0] == 0 the table is exact, otherwise its counts are lower bounds.
    What it is NOT: the depth of a layer, near + first * step (layer_depth), is the first sample inside a labelled cell, quantised
    to the step -- not the refined surface crossing of FieldViews; and the masks are those of the label product, not of a density."""
    keyword, clip_list = 'layers', ('layer_images', 'one dict of layer images')

    def __init__(self, cam_RT, cam_K, height, width, of='components', max_layers=4, step=None, arrays=('label', 'first', 'count')):
        if of not in LAYERS_OF:
            raise ValueError("ObjectLayers: of = %r must be 'components' or 'segments'" % (of,))
        if isinstance(max_layers, bool) or not isinstance(max_layers, (int, np.integer)) or not 1 <= max_layers <= MAX_LAYERS:
            raise ValueError('ObjectLayers: max_layers = %r must be an integer in [1, %d]' % (max_layers, MAX_LAYERS))
        arrays = tuple(arrays)
        if not set(arrays) <= set(LAYER_PIXEL_ARRAYS):
            raise ValueError('ObjectLayers: arrays = %r: names of %r' % (arrays, LAYER_PIXEL_ARRAYS))
        self.rt_inv, self.k_inv, self.rt64 = invert_cameras(cam_RT, cam_K)
        self.height, self.width = int(height), int(width)
        if self.height < 0 or self.width < 0:
            raise ValueError('ObjectLayers: height = %r, width = %r' % (height, width))
        self.of, self.max_layers, self.step = of, int(max_layers), step
        self.arrays = tuple(a for a in LAYER_PIXEL_ARRAYS if a in arrays)

    @classmethod
    def check(cls, option, given, point_sample_mode='grid'):
        """As GridProduct.check; the product it builds on is the instance's `of` (`needs` is a class attribute)."""
        super().check(option, given, point_sample_mode)
        if option.of not in LAYERS_OF:
            raise ValueError("ObjectLayers: of = %r must be 'components' or 'segments'" % (option.of,))
        if option.of not in given:
            raise ValueError("layers needs %s=<a %s>: it shows that product's objects in the views"
                             % (option.of, 'components.Components' if option.of == 'components' else 'watershed.Segments'))

    def prepare(self, grid):
        return march_range(grid.counts, grid.mins, grid.spacings, self.rt64, step=self.step)

    def run(self, grid, march, made):
        of = made[self.of]
        return self.layers(of['labels'], of['table'].shape[0], grid.counts, grid.mins, grid.spacings, march)

    def layers(self, labels, k, counts, mins, spacings, march):
        """-> the product's dict for labels (n,) int32 on their device; march = (near, step, n_steps)."""
        near, step, n_steps = march
        rt_inv, k_inv = (torch.from_numpy(m).to(labels.device) for m in (self.rt_inv, self.k_inv))
        out = ops.grid_layers(labels, k, counts, mins, spacings, rt_inv, k_inv, self.height, self.width, near, step, n_steps,
                              self.max_layers, want=self.arrays + ('table', 'status'))
        out['march'] = torch.tensor([near, step], dtype=torch.float32).to(labels.device)
        return out

    def __repr__(self):
        return 'ObjectLayers(V=%d, height=%d, width=%d, of=%r, max_layers=%d, step=%r, arrays=%r)' % (
            len(self.rt_inv), self.height, self.width, self.of, self.max_layers, self.step, self.arrays)


def object_layers(labels, k, counts, mins, spacings, cam_RT, cam_K, height, width, max_layers=4, near=None, far=None, step=None):
    """The stand-alone piece of ObjectLayers: labels (n,) int32 of k objects on the (nx, ny, nz) = `counts` grid whose points
    ops.grid_points made from `mins` / `spacings`, in the views of the cameras cam_RT / cam_K.  -> dict of device tensors: label,
    first, samples, point (V, H, W, L) int32, count (V, H, W) int32, table (V, k, 7) int32, status (2,) int32, march (2,) float32
    = [near, step] (the rules in include/ext/occ4d_layers.h; the march's defaults in march_range).  The cameras are inverted on the
    host (invert_cameras); nothing else is read."""
    option = ObjectLayers(cam_RT, cam_K, height, width, max_layers=max_layers, step=step, arrays=LAYER_PIXEL_ARRAYS)
    lab = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32))
    lab = lab.to(device=_device(lab), dtype=torch.int32)
    return option.layers(lab, k, counts, mins, spacings, march_range(counts, mins, spacings, option.rt64, near, far, step))


def _is_torch(*arrays):
    return any(isinstance(a, torch.Tensor) for a in arrays)


def layer_depth(first, march):
    """The depth of every layer: near + first * step in float32 -- sample `first`'s own d_i bit for bit (the product and the sum
    rounded one after the other) --, NaN where first is -1.  first: the int32 array of the product, march: its (2,) float32 [near,
    step]; torch tensors give a tensor on their device, numpy gives numpy."""
    if _is_torch(first):
        m = march if isinstance(march, torch.Tensor) else torch.as_tensor(np.asarray(march, np.float32))
        m = m.to(device=first.device, dtype=torch.float32)
        travelled = first.to(torch.float32) * m[1]
        return torch.where(first >= 0, m[0] + travelled, torch.full((), float('nan'), dtype=torch.float32, device=first.device))
    first, m = np.asarray(first), np.asarray(march, np.float32)
    travelled = first.astype(np.float32) * m[1]
    return np.where(first >= 0, m[0] + travelled, np.float32('nan')).astype(np.float32)


def amodal_mask(label, k):
    """(V, H, W) bool: the pixels object k's full extent covers, in front or behind others -- k is one of the pixel's stored layers."""
    return (label == int(k)).any(-1) if _is_torch(label) else (np.asarray(label) == int(k)).any(-1)


def visible_mask(label, k):
    """(V, H, W) bool: the pixels in which object k is in front -- layer 0."""
    return label[..., 0] == int(k)


def occlusion_rate(table):
    """(V, K) float32: 1 - VISIBLE / AMODAL per view and object, NaN where the object covers no pixel of the view."""
    if _is_torch(table):
        amodal, visible = table[..., LAYER_COLUMNS['AMODAL']].to(torch.float32), table[..., LAYER_COLUMNS['VISIBLE']].to(torch.float32)
        return torch.where(amodal > 0, 1.0 - visible / amodal, torch.full((), float('nan'), dtype=torch.float32, device=table.device))
    table = np.asarray(table)
    amodal, visible = table[..., LAYER_COLUMNS['AMODAL']].astype(np.float32), table[..., LAYER_COLUMNS['VISIBLE']].astype(np.float32)
    with np.errstate(all='ignore'):
        return np.where(amodal > 0, np.float32(1) - visible / amodal, np.float32('nan')).astype(np.float32)


def occlusion_pairs(label, count=None):
    """Who hides whom: (P, 4) int64 rows (view, front = the label of layer 0, behind = the label of a later layer, pixels), unique
    and sorted, over the pixels of label (V, H, W, L).  count is not needed (unused layers hold -1); given, only the pixels with
    count >= 2 are looked at.  torch.unique / np.unique on packed keys; no kernel of the package."""
    as_torch = _is_torch(label)
    lab = label.to(torch.int64) if as_torch else torch.from_numpy(np.ascontiguousarray(label)).to(torch.int64)
    V, H, W, L = lab.shape
    front, behind = lab[..., :1].expand(V, H, W, max(L - 1, 0)), lab[..., 1:]
    view = torch.arange(V, dtype=torch.int64, device=lab.device).view(V, 1, 1, 1).expand_as(behind)
    keep = (front >= 0) & (behind >= 0)
    if count is not None:
        cnt = count if isinstance(count, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(count))
        keep = keep & (cnt.to(lab.device)[..., None] >= 2)
    base = int(lab.max().item()) + 2 if lab.numel() else 2                                 # (labels are below 2^31 / 7)
    keys, pixels = torch.unique((view[keep] * base + front[keep]) * base + behind[keep], return_counts=True)
    rows = torch.stack([keys // (base * base), (keys // base) % base, keys % base, pixels], dim=1)
    return rows if as_torch else rows.numpy()
