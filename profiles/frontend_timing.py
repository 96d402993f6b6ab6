"""Times frontend.greater_clip / frontend.carla_clip at the published clip size (12 frames, ~172 K points in front of the
farthest-point sampling) against a from-scratch numpy restatement of the same steps on the same box.

    python profiles/frontend_timing.py [--repeats 10] [--warmup 3]

Per workload: device time (HIP events around the call, median of the repeats after the warm-up), host-inclusive time (wall
clock of the whole call with a device synchronisation at the end) and the numpy baseline (median of 3), each for the geometry
alone (frames -> shuffled clouds; n_fps_* chosen so that nothing is sampled) and, on the device, with the farthest-point
reduction to 14 336 points.  Every figure `x_ms` comes with `x_ms_range` = [min, max] of its repeats; run the command more
than once to see the spread between processes.  The baseline never runs the code under test; the box's core count is printed
with it.  The hue clusters are the test fixture's (tests/golden/frontend_greater_inputs.npz).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import occlusions4d_amd as pk  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUES = np.load(os.path.join(ROOT, 'tests', 'golden', 'frontend_greater_inputs.npz'))['hue_clusters'].astype(np.float64)


def look_at(eye, target):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, np.cross(fwd, right), fwd, eye
    return np.linalg.inv(pose)[:3].astype(np.float32)


def greater_frames(V=3, T=12, H=240, W=320, seed=0):
    rng = np.random.default_rng(seed)
    depth = rng.uniform(2.5, 12.0, size=(V, T, H, W)).astype(np.float32)
    depth[rng.uniform(size=depth.shape) < 0.1] = 0.0
    rgb = rng.uniform(size=(V, T, H, W, 3)).astype(np.float32)
    flat = rng.uniform(size=(V, T, H, W, 3)).astype(np.float32)
    flat[..., 2] = 0.0                                                  # saturated colours: most pixels get an id
    cam_RT = np.stack([np.stack([look_at([7 * np.cos(2.1 * v + 0.05 * t), 7 * np.sin(2.1 * v + 0.05 * t), 3.5], [0, 0, 0.5])
                                 for t in range(T)]) for v in range(V)])
    cam_K = np.zeros((V, T, 3, 3), dtype=np.float32)
    cam_K[..., 0, 0] = cam_K[..., 1, 1] = 1.1 * W
    cam_K[..., 0, 2], cam_K[..., 1, 2], cam_K[..., 2, 2] = W / 2.0, H / 2.0, 1.0
    return rgb, flat, depth, cam_RT, cam_K


def numpy_hue_ids(flat):
    mx, mn = flat.max(-1), flat.min(-1)
    delta = mx - mn
    safe = np.where(delta > 0, delta, 1).astype(np.float32)
    r, g, b = flat[..., 0], flat[..., 1], flat[..., 2]
    q = np.where(b == mx, 4 + (r - g) / safe, np.where(g == mx, 2 + (b - r) / safe, (g - b) / safe))
    h = np.where(delta > 0, (q / 6.0) % 1.0, 0).astype(np.float32)
    ids = np.abs(np.round(h * 360.0)[..., None] - HUES).argmin(-1).astype(np.float32)
    ids[np.where(mx > 0, delta / np.where(mx > 0, mx, 1), 0) < 0.9] = -1
    return ids


def numpy_greater(rgb, flat, depth, cam_RT, cam_K, n_points_rnd, src_view=0, ob=5.0, min_z=-1.0):
    """Frames -> shuffled input cloud + shuffled merged target frames, in numpy."""
    V, T, H, W = depth.shape
    py, px = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
    clouds = []
    for v in range(V):
        view = []
        for t in range(T):
            ids = numpy_hue_ids(flat[v, t])
            ok = depth[v, t] > 0
            k4, rt4 = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
            k4[:3, :3], rt4[:3] = cam_K[v, t], cam_RT[v, t]
            pts = np.ones((4, int(ok.sum())), dtype=np.float32)
            pts[0], pts[1] = px[ok], py[ok]
            pts = np.linalg.inv(k4) @ pts
            pts[:3] *= depth[v, t][ok]
            xyz = (np.linalg.inv(rt4) @ pts)[:3].T
            pcl = np.concatenate([xyz, ids[ok][:, None], rgb[v, t][ok]], axis=1)
            x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
            keep = (np.abs(x) <= ob) & (np.abs(y) <= ob) & (z >= min_z) & (z <= ob) & (z > (np.maximum(np.abs(x), np.abs(y)) - 4.5) / 3.5)
            pcl = pcl[keep]
            if 0 < n_points_rnd < pcl.shape[0]:
                pcl = pcl[np.sort(np.random.choice(pcl.shape[0], n_points_rnd, replace=False))]
            view.append(pcl)
        clouds.append(view)
    pcl_input = np.concatenate([np.concatenate([c, np.full((c.shape[0], 1), t, np.float32)], 1) for t, c in enumerate(clouds[src_view])])
    np.random.shuffle(pcl_input)
    target = np.concatenate([np.concatenate([c[-1][:, :4], np.full((c[-1].shape[0], 1), v, np.float32), c[-1][:, 4:]], 1)
                             for v, c in enumerate(clouds)])
    np.random.shuffle(target)
    return pcl_input, target


def carla_sweeps(V=4, T=12, N=40000, seed=1):
    rng = np.random.default_rng(seed)
    lidar = [[np.concatenate([rng.uniform([-20, -25, -2.5], [55, 25, 11], size=(N, 3)), rng.uniform(size=(N, 6))], 1).astype(np.float32)
              for _ in range(T)] for _ in range(V)]
    rt = np.tile(np.eye(4, dtype=np.float32), (T, V, 1, 1))
    for t in range(T):
        for v in range(V):
            a = 0.02 * t + 0.3 * v
            rt[t, v, :2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
            rt[t, v, :3, 3] = [2.0 * t, 0.5 * v, 1.0]
    return lidar, rt


def numpy_carla(lidar, rt, ob=20.0, min_z=-1.0):
    V, T = len(lidar), len(lidar[0])
    views = []
    for v in range(V):
        frames = []
        for t in range(T):
            pcl = lidar[v][t]
            if t != T - 1 or v != 0:
                pts = np.concatenate([pcl[:, :3].T, np.ones((1, pcl.shape[0]), np.float32)])
                pcl = pcl.copy()
                pcl[:, :3] = (np.linalg.inv(rt[T - 1, 0]) @ (rt[t, v] @ pts))[:3].T
            pcl[:, 2] += 1.0
            x, y, z = pcl[:, 0], pcl[:, 1], pcl[:, 2]
            frames.append(pcl[(x >= -ob * 0.7) & (x <= ob * 2.5) & (np.abs(y) <= ob) & (z >= min_z) & (z <= ob * 0.5)])
        views.append(frames)
    pcl_input = np.concatenate([np.concatenate([c, np.full((c.shape[0], 1), t, np.float32)], 1) for t, c in enumerate(views[0])])
    np.random.shuffle(pcl_input)
    target = np.concatenate([np.concatenate([c[-1][:, :6], np.full((c[-1].shape[0], 1), v, np.float32), c[-1][:, 6:]], 1)
                             for v, c in enumerate(views)])
    np.random.shuffle(target)
    return pcl_input, target


def time_device(fn, warmup, repeats):
    """((median, min, max) device ms by HIP events, (median, min, max) host-inclusive ms) of fn()."""
    dev, host = [], []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i >= warmup:
            dev.append(e0.elapsed_time(e1))
            host.append((t1 - t0) * 1e3)
    return _stats(dev), _stats(host)


def _stats(ms):
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def _put(res, name, stats):
    res[name] = round(stats[0], 3)
    res[name + '_range'] = [round(stats[1], 3), round(stats[2], 3)]


def time_host(fn, repeats=3):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return _stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads())

    rgb, flat, depth, cam_RT, cam_K = greater_frames()
    frames = [torch.from_numpy(x).to(dev) for x in (rgb, flat, depth)]
    kw = dict(cam_RT=cam_RT, cam_K=cam_K, hue_clusters=HUES, n_points_rnd=14336, pcl_target_frames=1)

    def greater(n_in, n_tg):
        np.random.seed(0)
        torch.manual_seed(0)
        return pk.frontend.greater_clip(frames[0], frames[1], frames[2], n_fps_input=n_in, n_fps_target=n_tg, **kw)
    probe = pk.frontend.greater_clip(frames[0], frames[1], frames[2], n_fps_input=14336, n_fps_target=14336, **kw)
    res['greater_points_before_fps'] = int(probe[3]['pcl_sizes'][0].sum())
    # "geometry": n_fps_input equal to the cloud's own size and n_fps_target 0 -> nothing is sampled or padded
    n_own = res['greater_points_before_fps']
    for tag, (n_in, n_tg) in (('geometry', (n_own, 0)), ('with_fps', (14336, 14336))):
        d, h = time_device(lambda: greater(n_in, n_tg), a.warmup, a.repeats)
        _put(res, 'greater_%s_device_ms' % tag, d)
        _put(res, 'greater_%s_host_inclusive_ms' % tag, h)
    _put(res, 'greater_geometry_numpy_ms', time_host(lambda: numpy_greater(rgb, flat, depth, cam_RT, cam_K, 14336)))
    _put(res, 'greater_upload_frames_ms',
         time_host(lambda: ([torch.from_numpy(x).to(dev) for x in (rgb, flat, depth)], torch.cuda.synchronize())))

    lidar, rt = carla_sweeps()
    sweeps = [[torch.from_numpy(s).to(dev) for s in view] for view in lidar]
    ckw = dict(reference_frame=-1, pcl_target_frames=1)
    probe = pk.frontend.carla_clip(sweeps, rt, n_fps_input=14336, n_fps_target=14336, **ckw)
    n_own = int(probe[3]['pcl_sizes'][0].sum())
    res['carla_points_before_fps'] = n_own

    def carla(n_in, n_tg):
        np.random.seed(0)
        torch.manual_seed(0)
        return pk.frontend.carla_clip(sweeps, rt, n_fps_input=n_in, n_fps_target=n_tg, **ckw)
    for tag, (n_in, n_tg) in (('geometry', (n_own, 0)), ('with_fps', (14336, 14336))):
        d, h = time_device(lambda: carla(n_in, n_tg), a.warmup, a.repeats)
        _put(res, 'carla_%s_device_ms' % tag, d)
        _put(res, 'carla_%s_host_inclusive_ms' % tag, h)
    _put(res, 'carla_geometry_numpy_ms', time_host(lambda: numpy_carla([[s.copy() for s in view] for view in lidar], rt)))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
