"""Times the virtual lidar sweep of the decoded field (ops.sweep_rays: occ4d_sweep_rays_f32) at the published grid -- the GREATER
configuration's geometry.grid_counts for 524 288 samples = 96 x 96 x 58 = 534 528 queries --, against the ray cast into camera
views at an equal number of rays and steps, and what perform_inference(sweep=FieldSweep()) adds to a call with components=.
Not a test: it sets no pass mark.  It needs a GPU and fails without one.

    python profiles/sweep_timing.py [--repeats 20] [--warmup 3] [--no-numpy] [--no-call]

Patterns: `lidar1`, a 64 x 1024 table (elevations +15 .. -25 degrees, the full circle) from one pose inside the grid, in free
space of the blob field; `lidar3`, the same table from three poses, one inside and two outside; `replay`, one (1, 65 536) bundle
with per_view=True that sweep.directions_to makes of random points of the hull.
Fields, each an (n, 5) array whose column 0 is the density: the six-blob synthetic field of profiles/surface_timing.py, the array
the untrained synthetic scene of profiles/refine_timing.py decodes to, all free and all solid.  The march is sweep.march_range's
default: step = half the smallest spacing.  Timed per field and pattern, device time by HIP events and the host-inclusive wall
clock, median of the repeats after the warm-up, `x_ms_range` = [min, max]:
  - `all`: every output (three feature columns, the components' labels as inst), and `range`: the range alone;
  - `raycast`: IN THE SAME RUN ops.raycast_grid, unchanged by this feature, on the same density at as many rays (256 x 256 pixels
    per pose, cameras at the sensors' places looking at the grid's centre) and the same n_steps, depth and cell: the yardstick.
    What the sweep costs beyond it is the gradient, the owner and the extra stores (and whatever the different rays meet);
  - `numpy`: the numpy float32 RESTATEMENT of the header (tests/sweep_cases.py: restate, which walks every sample) of lidar1 on this
    box's CPU, once, with the device's result asserted EQUAL.  A restatement, not a tuned baseline;
  - perform_inference on the synthetic scene with components=Components() and with sweep=FieldSweep(of='components', rows=...)
    beside it, the two calls ALTERNATING in one process.  The call without sweep is the code path from before this feature: its
    range is the spread to read the difference against.
Run the command three times to see the spread between processes.  A trained model's sweeps are not measured: there is no checkpoint."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'profiles'))
import occlusions4d_amd as pk  # noqa: E402
import raycast_cases as yc  # noqa: E402
import sweep_cases as sc  # noqa: E402
from frontend_timing import _put, _stats, time_host  # noqa: E402
from surface_timing import BATCH, N_POINTS, NUM_SAMPLE, SEED, VIDEO_LEN, blob_field  # noqa: E402

BEAMS, AZIMUTHS, SIDE = 64, 1024, 256
CHANNELS = (1, 2, 3)


def time_alternating(fns, warmup, repeats):
    """{name: ((median, min, max) device ms, (median, min, max) host-inclusive ms)} of the calls fns[name](), ALTERNATING."""
    dev, host = {k: [] for k in fns}, {k: [] for k in fns}
    for i in range(warmup + repeats):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= warmup:
                dev[name].append(e0.elapsed_time(e1))
                host[name].append((t1 - t0) * 1e3)
    return {k: (_stats(dev[k]), _stats(host[k])) for k in fns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-numpy', action='store_true', help='skip the numpy restatement')
    ap.add_argument('--no-call', action='store_true', help='skip the perform_inference comparison')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('profiles/sweep_timing.py needs a GPU: nothing is measured without one')
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads(),
               library=os.path.basename(pk._lib.LIB_PATH))
    pa, ia, inf = pk.configs.model_args('greater', N_POINTS)
    counts, mins, spacings = pk.geometry.grid_frame(NUM_SAMPLE, inf['min_z'], inf['cube_bounds'], 'greater', inf['cube_mode'])
    counts = tuple(int(c) for c in counts)
    n = counts[0] * counts[1] * counts[2]
    lo, hi = yc.hull(counts, mins, spacings)
    centre, ext = 0.5 * (lo + hi), hi - lo
    reach = float(np.linalg.norm(ext))
    blob_host = blob_field(counts, np.random.default_rng(SEED))
    # the sensor inside the grid stands in free space of the blob field: the candidate nearest the centre whose grid point is air
    density = blob_host[:, 0].reshape(counts)
    inside = None
    for off in sorted(((x, y, z) for x in np.linspace(-0.3, 0.3, 7) for y in np.linspace(-0.3, 0.3, 7) for z in (-0.2, 0.0, 0.2)),
                      key=lambda o: o[0] ** 2 + o[1] ** 2 + o[2] ** 2):
        at = centre + np.array(off) * ext
        idx = tuple(int(round((p - m) / s - 0.5)) for p, m, s in zip(at, mins, spacings))
        if density[idx] < 0.05:
            inside = at
            break
    assert inside is not None, 'no free place inside the blob field'
    origins = [inside, centre + np.array([-0.8, -0.5, 0.4]) * reach, centre + np.array([0.7, -0.6, 0.3]) * reach]
    poses = np.stack([np.concatenate([sc.facing(o, centre + np.array([1.0, 0.0, 0.0]) if i == 0 else centre), o[:, None]], axis=1)
                      for i, o in enumerate(origins)])
    table = pk.sweep.lidar_directions(BEAMS, AZIMUTHS, 15.0, -25.0)
    rng = np.random.default_rng(SEED)
    targets = lo + rng.uniform(size=(BEAMS * AZIMUTHS, 3)) * ext
    replay_dirs, _ = pk.sweep.directions_to((targets - origins[0]) @ poses[0][:, :3])
    patterns = dict(lidar1=(poses[:1], table, (BEAMS, AZIMUTHS), False), lidar3=(poses, table, (BEAMS, AZIMUTHS), False),
                    replay=(poses[:1], replay_dirs, (1, BEAMS * AZIMUTHS), True))
    near, step, n_steps = pk.sweep.march_range(counts, mins, spacings, poses)
    res.update(grid=list(counts), queries=n, beams=BEAMS, azimuths=AZIMUTHS, near=near, step=step, n_steps=n_steps, channels=len(CHANNELS))
    cam_K = np.array([[0.8 * SIDE, 0.0, (SIDE - 1) / 2.0], [0.0, 0.8 * SIDE, (SIDE - 1) / 2.0], [0.0, 0.0, 1.0]], np.float32)
    cam_RT = np.stack([yc.look_at(o, centre + np.array([1.0, 0.0, 0.0]) if i == 0 else centre) for i, o in enumerate(origins)]).astype(np.float32)
    rt_inv, k_inv, _ = pk.projection.invert_cameras(cam_RT, cam_K)

    esd, dsd = pk.configs.synthetic_weights(pa, ia, SEED)
    enc = pk.model.PointCompletionNetV3(**pa).to(dev).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).to(dev).eval()
    dec.load_state_dict(dsd)
    pcl = pk.configs.synthetic_pcl('greater', N_POINTS, VIDEO_LEN, SEED)

    def call(components, sweep):
        return pk.inference.perform_inference(
            pcl.clone(), None, None, [enc, dec], dev, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], 3, None,
            sample_implicit=True, num_sample=NUM_SAMPLE, point_sample_mode='grid', batch_size=BATCH,
            predict_segmentation=inf['predict_segmentation'], track_mode='none', semantic_classes=13, density_threshold=0.5,
            data_kind='greater', cube_mode=inf['cube_mode'], compress_air=True, components=components, sweep=sweep)

    scene = torch.from_numpy(call(None, None)['implicit_output'][:, :5].copy()).to(dev)
    blobs = torch.from_numpy(blob_host).to(dev)
    fields = dict(blobs=blobs, scene=scene, free=torch.zeros((n, 5), device=dev), solid=torch.ones((n, 5), device=dev))

    def sweep(field, labels, K, pattern, want):
        pose, dirs, shape, per_view = pattern
        everything = want == pk.ops.SWEEP_ARRAYS
        return pk.ops.sweep_rays(field[:, 0], counts, mins, spacings, 0.5, pose, dirs, shape, near, step, n_steps, per_view=per_view,
                                 attrs=field if everything else None, channels=CHANNELS if everything else (),
                                 labels=labels if everything else None, k=K, background=-1.0, want=want)

    for fname, field in fields.items():
        labels, tab = pk.components.label(field, counts, 0.5, 6)
        K = int(tab.shape[0])
        res[fname + '_objects'] = K
        for pname, (pose, dirs, shape, per_view) in patterns.items():
            pattern = (torch.from_numpy(np.ascontiguousarray(pose.reshape(-1, 12), np.float32)).to(dev), torch.from_numpy(dirs).to(dev), shape, per_view)
            V = pose.shape[0]
            key = '%s_%s' % (fname, pname)
            first = {k: t.cpu().numpy() for k, t in sweep(field, labels, K, pattern, pk.ops.SWEEP_ARRAYS).items()}
            res[key + '_returns'] = int((first['cell'] >= 0).sum())
            res[key + '_rays'] = int(first['cell'].size)
            rt_d, k_d = torch.from_numpy(rt_inv[:V]).to(dev), torch.from_numpy(k_inv[:V]).to(dev)
            column = field[:, 0].contiguous()
            fns = dict(all=lambda: sweep(field, labels, K, pattern, pk.ops.SWEEP_ARRAYS), range=lambda: sweep(field, labels, K, pattern, ('range',)))
            fns['raycast'] = lambda: pk.ops.raycast_grid(column, counts, mins, spacings, 0.5, rt_d, k_d, SIDE, SIDE, near, step, n_steps)
            for name, (d, h) in time_alternating(fns, a.warmup, a.repeats).items():
                _put(res, '%s_%s_device_ms' % (key, name), d)
                _put(res, '%s_%s_host_inclusive_ms' % (key, name), h)
            res[key + '_all_over_raycast'] = round(res[key + '_all_device_ms'] / max(res[key + '_raycast_device_ms'], 1e-6), 2)
            if pname == 'lidar1' and not a.no_numpy:
                host_field, host_labels = field.cpu().numpy(), labels.cpu().numpy()
                want = {}

                def numpy_call():
                    want.update(sc.restate(host_field[:, 0], counts, mins, spacings, 0.5, pose.reshape(-1, 12), dirs, shape, per_view, near,
                                           step, n_steps, host_field, CHANNELS, None, host_labels, K, -1.0))
                _put(res, key + '_numpy_restatement_ms', time_host(numpy_call, repeats=1))
                sc.same(first, want)                # EQUAL, or this script fails
                res[key + '_equal_to_restatement'] = True

    if not a.no_call:
        comp = pk.components.Components()
        option = pk.sweep.FieldSweep(poses, table, shape=(BEAMS, AZIMUTHS), channels=CHANNELS, of='components', rows=CHANNELS)
        times = {m: ([], []) for m in ('components', 'sweep')}
        out = {}
        for i in range(a.warmup + a.repeats):
            for mode in ('components', 'sweep'):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                out[mode] = call(comp, option if mode == 'sweep' else None)
                e1.record()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if i >= a.warmup:
                    times[mode][0].append(e0.elapsed_time(e1))
                    times[mode][1].append((t1 - t0) * 1e3)
        for mode in ('components', 'sweep'):
            _put(res, '%s_call_device_ms' % mode, _stats(times[mode][0]))
            _put(res, '%s_call_host_inclusive_ms' % mode, _stats(times[mode][1]))
        res['sweep_adds_ms'] = round(res['sweep_call_host_inclusive_ms'] - res['components_call_host_inclusive_ms'], 3)
        res['call_returns'] = int(out['sweep']['sweep']['n_rows'][0])
        res['call_rays'] = int(out['sweep']['sweep']['cell'].size)
        res['call_output_unchanged'] = bool(np.array_equal(out['components']['implicit_output'], out['sweep']['implicit_output'], equal_nan=True)
                                            and np.array_equal(out['components']['components']['labels'], out['sweep']['components']['labels']))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
