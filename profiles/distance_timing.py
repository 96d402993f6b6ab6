"""Times the distance transform of the solid set (ops.grid_distance: occ4d_distance_grid_f32) at the published grid -- the GREATER
configuration's geometry.grid_counts for 524 288 samples = 534 528 queries -- and what perform_inference(clearance=Clearance()) adds
to a call.  Not a test: it sets no pass mark.

    python profiles/distance_timing.py [--repeats 20] [--warmup 3]

Three fields at level 0.5, weights (1, 1, 1): the six-blob synthetic field of profiles/surface_timing.py, the density column the
untrained synthetic scene of profiles/refine_timing.py decodes to, and an all-air field but one site in the corner (0, 0, 0): the
largest costs, and the worst case for any visiting order that stops early.  Timed per field, with and without `nearest`:
  - ops.grid_distance (no host read): device time by HIP events and the host-inclusive wall clock, median of the repeats after the
    warm-up, `x_ms_range` = [min, max];
  - where scipy is importable, the same result on the same box's CPU: the array's copy to the host and
    scipy.ndimage.distance_transform_edt (return_indices where `nearest` is asked; scipy is single-threaded: the 16 CPUs of a
    command change nothing); rint of its squared distances is compared EQUAL with the device's dist2 (`equal_to_scipy`), and with
    indices the cost to scipy's site with dist2 (its tie rule is its own, so the sites themselves may differ);
  - perform_inference on the synthetic scene with and without clearance=Clearance(nearest=True), the two calls ALTERNATING in one
    process.  The call without `clearance` is the code path from before this feature, unchanged.
Run the command three times to see the spread between processes.  The g++ twin is not tuned and is not timed."""
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
from frontend_timing import _put, _stats, time_device, time_host  # noqa: E402
from surface_timing import BATCH, N_POINTS, NUM_SAMPLE, SEED, VIDEO_LEN, blob_field  # noqa: E402

try:
    from scipy import ndimage
except ImportError:
    ndimage = None


def scipy_edt(values, counts, indices):
    """(rint(edt^2) (n,) int64, the flat index of scipy's site (n,) or None) from the device column `values`."""
    air = ~(values.cpu().numpy().reshape(counts) >= np.float32(0.5))
    got = ndimage.distance_transform_edt(air, return_indices=indices)
    dist, where = got if indices else (got, None)
    flat = None if where is None else ((where[0].astype(np.int64) * counts[1] + where[1]) * counts[2] + where[2]).reshape(-1)
    return np.rint(dist.astype(np.float64) ** 2).astype(np.int64).reshape(-1), flat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads(),
               scipy=None if ndimage is None else __import__('scipy').__version__)
    pa, ia, inf = pk.configs.model_args('greater', N_POINTS)
    counts, mins, spacings = pk.geometry.grid_frame(NUM_SAMPLE, inf['min_z'], inf['cube_bounds'], 'greater', inf['cube_mode'])
    counts = tuple(int(c) for c in counts)
    n = counts[0] * counts[1] * counts[2]
    res.update(grid=list(counts), queries=n)

    esd, dsd = pk.configs.synthetic_weights(pa, ia, SEED)
    enc = pk.model.PointCompletionNetV3(**pa).to(dev).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).to(dev).eval()
    dec.load_state_dict(dsd)
    pcl = pk.configs.synthetic_pcl('greater', N_POINTS, VIDEO_LEN, SEED)

    def call(clearance):
        return pk.inference.perform_inference(
            pcl.clone(), None, None, [enc, dec], dev, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], 3, None,
            sample_implicit=True, num_sample=NUM_SAMPLE, point_sample_mode='grid', batch_size=BATCH,
            predict_segmentation=inf['predict_segmentation'], track_mode='none', semantic_classes=13, density_threshold=0.5,
            data_kind='greater', cube_mode=inf['cube_mode'], compress_air=True, clearance=clearance)

    scene = torch.from_numpy(call(None)['implicit_output']).to(dev)
    corner = torch.zeros((n, 1), device=dev)
    corner[0, 0] = 1.0
    fields = dict(blobs=torch.from_numpy(blob_field(counts, np.random.default_rng(SEED))).to(dev), scene=scene, corner=corner)
    xyz = np.stack(np.meshgrid(*(np.arange(c, dtype=np.int64) for c in counts), indexing='ij'), -1).reshape(-1, 3)
    for name, field in fields.items():
        column = field[:, 0]
        for nearest in (False, True):
            key = '%s_%s' % (name, 'nearest' if nearest else 'dist2')
            dist2, site = pk.ops.grid_distance(column, counts, 0.5, nearest=nearest)
            host = dist2.cpu().numpy().astype(np.int64)
            res[name + '_solid_share'] = round(float((dist2 == 0).float().mean()), 4)
            res[name + '_largest_dist2'] = int(host.max())
            d, h = time_device(lambda: pk.ops.grid_distance(column, counts, 0.5, nearest=nearest), a.warmup, a.repeats)
            _put(res, key + '_device_ms', d)
            _put(res, key + '_host_inclusive_ms', h)
            if ndimage is not None:
                got = {}
                _put(res, key + '_scipy_ms', time_host(lambda: got.update(r=scipy_edt(column, counts, nearest)), repeats=3))
                equal = bool(np.array_equal(got['r'][0], host))
                if nearest:
                    equal = equal and bool(np.array_equal(((xyz - xyz[got['r'][1]]) ** 2).sum(-1), host))
                res[key + '_equal_to_scipy'] = equal
                res[key + '_scipy_over_device'] = round(res[key + '_scipy_ms'] / res[key + '_host_inclusive_ms'], 1)

    # what clearance= adds to a call
    times = {m: ([], []) for m in ('plain', 'clearance')}
    out = {}
    for i in range(a.warmup + a.repeats):
        for mode in ('plain', 'clearance'):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out[mode] = call(pk.distance.Clearance(nearest=True) if mode == 'clearance' else None)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= a.warmup:
                times[mode][0].append(e0.elapsed_time(e1))
                times[mode][1].append((t1 - t0) * 1e3)
    for mode in ('plain', 'clearance'):
        _put(res, '%s_call_device_ms' % mode, _stats(times[mode][0]))
        _put(res, '%s_call_host_inclusive_ms' % mode, _stats(times[mode][1]))
    res['clearance_adds_ms'] = round(res['clearance_call_host_inclusive_ms'] - res['plain_call_host_inclusive_ms'], 3)
    res['call_output_unchanged'] = bool(np.array_equal(out['plain']['implicit_output'], out['clearance']['implicit_output'], equal_nan=True))
    res['call_dist2_is_the_pieces'] = bool(np.array_equal(
        out['clearance']['clearance']['dist2'], pk.ops.grid_distance(scene[:, 0], counts, 0.5)[0].cpu().numpy()))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
