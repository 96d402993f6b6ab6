"""Times the camera projection, the z-buffer and the visibility test of include/occ4d_project.h at the published sizes against
the numpy path on host arrays.  Not a test: it asserts nothing.

    python profiles/project_timing.py [--repeats 10] [--warmup 3]

Sizes: 110 000 solid rows (a decoded GREATER frame) into 3 views of 240 x 320 at radius 0 and 1 (projection.render_views: fill,
splat, resolve with 3 feature channels); the visibility codes of a 14 336-point target against one depth image; the full
534 528-row grid into the 3 views and against one image as the upper end.  Device time by HIP events around the call and the
host-inclusive wall clock of the same call, median of the repeats after the warm-up, `x_ms_range` = [min, max]; run the command
three times to see the spread between processes.

The yardstick is numpy on the same box with the arrays already on the host (the thread count is whatever the environment
allows; it is printed): pixel_coords_from_point_cloud restated in numpy (two (4, 4) @ (4, N) float32 products and the division,
as utils/geometry.py:67-115 has them), the z-buffer as np.lexsort((index, depth, pixel)) over the clipped footprints, and the
depth test as array expressions."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import occlusions4d_amd as pk  # noqa: E402
from frontend_timing import _put, time_device, time_host  # noqa: E402

H, W, V = 240, 320, 3


def look_at(eye, target):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, np.cross(fwd, right), fwd, eye
    return np.linalg.inv(pose)[:3].astype(np.float32)


def numpy_project(pcl, cam_RT, cam_K):
    """(u, v, depth) as the reference computes them, columns of an (N, 3) float32 array."""
    rt, k = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    rt[:3], k[:3, :3] = cam_RT, cam_K
    pts = np.ones((4, pcl.shape[0]), np.float32)
    pts[:3] = pcl[:, :3].T
    cam = rt @ pts
    z = cam[2].copy()
    cam[:2] /= z[None]
    cam[2] = 1.0
    return np.concatenate([(k @ cam).T[:, :2], z[:, None]], axis=1)


def numpy_pixels(uvz):
    with np.errstate(invalid='ignore'):
        ru, rv = np.round(uvz[:, 0]), np.round(uvz[:, 1])
        on = (uvz[:, 2] > 0) & np.isfinite(uvz[:, 2]) & (ru >= 0) & (ru < W) & (rv >= 0) & (rv < H)
    return on, ru[on].astype(np.int64), rv[on].astype(np.int64)


def numpy_render(pcl, cam_RT, cam_K, radius, channels):
    depth, index = np.zeros((V, H * W), np.float32), np.full((V, H * W), -1, np.int32)
    feat = np.zeros((V, H * W, len(channels)), np.float32)
    for v in range(V):
        uvz = numpy_project(pcl, cam_RT[v], cam_K)
        on, px, py = numpy_pixels(uvz)
        rows = np.flatnonzero(on)
        pix, ind = [], []
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                x, y = px + dx, py + dy
                ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
                pix.append((y * W + x)[ok])
                ind.append(rows[ok])
        pix, ind = np.concatenate(pix), np.concatenate(ind)
        order = np.lexsort((ind, uvz[ind, 2], pix))
        first = np.ones(len(order), bool)
        first[1:] = pix[order][1:] != pix[order][:-1]
        win = order[first]
        depth[v, pix[win]], index[v, pix[win]] = uvz[ind[win], 2], ind[win]
        feat[v, pix[win]] = pcl[ind[win]][:, channels]
    return depth, index, feat


def numpy_visibility(points, depth, cam_RT, cam_K, margin):
    uvz = numpy_project(points, cam_RT, cam_K)
    on, px, py = numpy_pixels(uvz)
    code = np.full(points.shape[0], 2, np.int32)
    d = depth[py, px]
    code[on] = (d > 0) & (uvz[on, 2] - d > np.float32(margin))
    return code


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads(),
               omp_num_threads=os.environ.get('OMP_NUM_THREADS'))
    rng = np.random.default_rng(1)
    cam_RT = np.stack([look_at(eye, [0.0, 0.0, 1.0]) for eye in ([9.0, 0.5, 4.0], [-4.0, 8.0, 3.0], [-5.0, -7.0, 5.0])])
    cam_K = np.array([[280.0, 0.0, W / 2.0], [0.0, 280.0, H / 2.0], [0.0, 0.0, 1.0]], np.float32)
    channels = (4, 5, 6)
    equal = True
    for label, n in (('solid_110k', 110000), ('grid_534k', 534528)):
        pcl = np.concatenate([rng.uniform([-5, -5, -1], [5, 5, 5], size=(n, 3)), rng.uniform(size=(n, 5))], axis=1).astype(np.float32)
        rows = torch.from_numpy(pcl).to(dev)
        for radius in ((0, 1) if n < 200000 else (0,)):
            d, h = time_device(lambda: pk.projection.render_views(rows, cam_RT, cam_K, H, W, channels=channels, radius=radius),
                               a.warmup, a.repeats)
            _put(res, 'render_%s_r%d_device_ms' % (label, radius), d)
            _put(res, 'render_%s_r%d_host_inclusive_ms' % (label, radius), h)
            _put(res, 'numpy_render_%s_r%d_ms' % (label, radius), time_host(lambda: numpy_render(pcl, cam_RT, cam_K, radius, channels), 3))
            img = pk.projection.render_views(rows, cam_RT, cam_K, H, W, channels=channels, radius=radius)
            want = numpy_render(pcl, cam_RT, cam_K, radius, channels)
            res['covered_%s_r%d' % (label, radius)] = round(float((want[1] >= 0).mean()), 3)
            equal &= all(np.array_equal(img[key].cpu().numpy().reshape(w.shape), w) for key, w in zip(('depth', 'index', 'features'), want))
        rt, k = pk.projection.expand_cameras(cam_RT, cam_K, dev)
        for name, fn in (('project', lambda: pk.ops.project_points(rows, rt, k)),
                         ('splat_r0', lambda: pk.ops.zbuffer_splat(rows, rt, k, H, W, 0)),
                         ('splat_r1', lambda: pk.ops.zbuffer_splat(rows, rt, k, H, W, 1)),
                         ('splat_r4', lambda: pk.ops.zbuffer_splat(rows, rt, k, H, W, 4))):
            _put(res, 'entry_%s_%s_device_ms' % (name, label), time_device(fn, a.warmup, a.repeats)[0])
        keys = pk.ops.zbuffer_splat(rows, rt, k, H, W, 0)
        _put(res, 'entry_resolve_c3_%s_device_ms' % label, time_device(lambda: pk.ops.zbuffer_resolve(keys, rows, channels), a.warmup, a.repeats)[0])
    depth = pk.projection.render_views(rows, cam_RT[:1], cam_K, H, W, radius=1)['depth']
    depth_np = depth.cpu().numpy()[0]
    for label, n in (('target_14336', 14336), ('grid_534k', 534528)):
        pts_np = rng.uniform([-5, -5, -1], [5, 5, 5], size=(n, 3)).astype(np.float32)
        pts = torch.from_numpy(pts_np).to(dev)
        d, h = time_device(lambda: pk.projection.visibility(pts, depth, cam_RT[:1], cam_K, 0.05), a.warmup, a.repeats)
        _put(res, 'visibility_%s_device_ms' % label, d)
        _put(res, 'visibility_%s_host_inclusive_ms' % label, h)
        _put(res, 'numpy_visibility_%s_ms' % label, time_host(lambda: numpy_visibility(pts_np, depth_np, cam_RT[0], cam_K, 0.05), a.repeats))
        code = pk.projection.visibility(pts, depth, cam_RT[:1], cam_K, 0.05)[0].cpu().numpy()
        res['codes_%s' % label] = np.bincount(code, minlength=3).tolist()
        equal &= bool(np.array_equal(code, numpy_visibility(pts_np, depth_np, cam_RT[0], cam_K, 0.05)))
    res['equal_to_numpy'] = bool(equal)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
