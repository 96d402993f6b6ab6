"""Clouds into camera views on the device (include/occ4d_project.h): the projection of the reference's
``pixel_coords_from_point_cloud`` (utils/geometry.py:67-115, the exact inverse of the unprojection the clip front end restates),
a z-buffer over it, and the per-point visibility test against a depth image.

``render_views`` turns a cloud -- the decoded solid rows, an input or a target cloud -- into depth, index and feature images
under a clip's cameras, to be put beside the RGB-D frames the cloud came from.  ``visibility`` gives the partition of target
points the model is scored on: VISIBLE from a camera, OCCLUDED from it, or OUTSIDE its frustum; ``evaluation.evaluate_clip(
stats_occlusion=...)`` feeds it to ``EvalStats`` as the group of every target point.  Where a data set has no depth image (CARLA),
``render_views`` of the forward sweep gives one.

Everything runs in the four kernels of csrc/project.hip; clouds, cameras and images stay on the device and no function here
reads a device value on the host.  The arithmetic equals the reference's numpy results bit for bit (tests/golden/project_*.npz).
"""
import numpy as np
import torch

from . import _lib, ops

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
