"""Times the surface extraction (ops.surface_nets: occ4d_surface_count_f32 / occ4d_surface_write_f32) at the published grid -- the
GREATER configuration's geometry.grid_counts for 524 288 samples = 534 528 queries, five output columns as vertex attributes --
and what perform_inference(surface=Surface()) adds to a call.  Not a test: it sets no pass mark.

    python profiles/surface_timing.py [--repeats 20] [--warmup 3]

The field is synthetic: the sigmoid of a sum of a few smooth blobs (seeded), level 0.5; the attribute columns are the density and
four smooth functions of the position.  Timed:
  - the device call with its 8-byte count read (sync=True) and without it (sync=False, capacity-sized buffers): device time by
    HIP events and the host-inclusive wall clock, median of the repeats after the warm-up, `x_ms_range` = [min, max];
  - the vectorised numpy float32 restatement of the same rules (tests/surface_cases.py: restate) on the same box's CPU, whose
    result the device's is compared EQUAL with (`equal_to_restatement`);
  - perform_inference on the synthetic scene of profiles/refine_timing.py with and without surface=Surface(), the two calls
    ALTERNATING in one process.  The call without `surface` is the code path from before this feature, unchanged.  The synthetic
    scene's weights are untrained: its surface is whatever the untrained density field crosses 0.5 at (`call_vertices`).
Run the command three times to see the spread between processes."""
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
import occlusions4d_amd as pk  # noqa: E402
import surface_cases as sc  # noqa: E402
from frontend_timing import _put, _stats, time_device, time_host  # noqa: E402

N_POINTS, VIDEO_LEN, NUM_SAMPLE, BATCH, SEED = 14336, 12, 524288, 32768, 1830
N_BLOBS, N_ATTR = 6, 5


def blob_field(counts, rng):
    """(n, N_ATTR) float32: column 0 = sigmoid(sum of N_BLOBS gaussians - 0.5) on the grid, the others smooth in the position."""
    idx = [np.arange(c, dtype=np.float64) / c for c in counts]
    x, y, z = np.meshgrid(*idx, indexing='ij')
    total = np.zeros(counts)
    for _ in range(N_BLOBS):
        cx, cy, cz = rng.uniform(0.2, 0.8, size=3)
        r = rng.uniform(0.08, 0.2)
        total += np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (2 * r * r))
    density = 1.0 / (1.0 + np.exp(-8.0 * (total - 0.5)))
    cols = [density, x, y * z, np.sin(6 * x + 2 * y), np.cos(5 * z)]
    return np.stack([c.reshape(-1) for c in cols], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads())
    pa, ia, inf = pk.configs.model_args('greater', N_POINTS)
    counts, mins, spacings = pk.geometry.grid_frame(NUM_SAMPLE, inf['min_z'], inf['cube_bounds'], 'greater', inf['cube_mode'])
    counts = tuple(counts)
    field = blob_field(counts, np.random.default_rng(SEED))
    n = field.shape[0]
    field_dev = torch.from_numpy(field).to(dev)

    def device_call(sync=True):
        return pk.ops.surface_nets(field_dev[:, 0], counts, 0.5, mins, spacings, attrs=field_dev, sync=sync)

    v, f = device_call()
    res.update(grid=list(counts), queries=n, attributes=N_ATTR, vertices=int(v.shape[0]), faces=int(f.shape[0]),
               inside_share=round(float((field[:, 0] >= 0.5).mean()), 4))
    for name, sync in (('device_call', True), ('device_call_nosync', False)):
        d, h = time_device(lambda: device_call(sync), a.warmup, a.repeats)
        _put(res, name + '_device_ms', d)
        _put(res, name + '_host_inclusive_ms', h)
    want = {}

    def numpy_call():
        want.update(sc.restate(field[:, 0], counts, 0.5, mins, spacings, field))
    _put(res, 'numpy_restatement_ms', time_host(numpy_call, repeats=3))
    res['equal_to_restatement'] = bool(sc.same_mesh(v.cpu().numpy(), f.cpu().numpy(), want))
    res['numpy_over_device'] = round(res['numpy_restatement_ms'] / res['device_call_host_inclusive_ms'], 1)

    # what surface= adds to a call
    esd, dsd = pk.configs.synthetic_weights(pa, ia, SEED)
    enc = pk.model.PointCompletionNetV3(**pa).to(dev).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).to(dev).eval()
    dec.load_state_dict(dsd)
    pcl = pk.configs.synthetic_pcl('greater', N_POINTS, VIDEO_LEN, SEED)

    def call(surface):
        return pk.inference.perform_inference(
            pcl.clone(), None, None, [enc, dec], dev, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], 3, None,
            sample_implicit=True, num_sample=NUM_SAMPLE, point_sample_mode='grid', batch_size=BATCH,
            predict_segmentation=inf['predict_segmentation'], track_mode='none', semantic_classes=13, density_threshold=0.5,
            data_kind='greater', cube_mode=inf['cube_mode'], compress_air=True, surface=surface)

    times = {m: ([], []) for m in ('plain', 'surface')}
    out = {}
    for i in range(a.warmup + a.repeats):
        for mode in ('plain', 'surface'):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out[mode] = call(pk.surface.Surface() if mode == 'surface' else None)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= a.warmup:
                times[mode][0].append(e0.elapsed_time(e1))
                times[mode][1].append((t1 - t0) * 1e3)
    for mode in ('plain', 'surface'):
        _put(res, '%s_call_device_ms' % mode, _stats(times[mode][0]))
        _put(res, '%s_call_host_inclusive_ms' % mode, _stats(times[mode][1]))
    res['surface_adds_ms'] = round(res['surface_call_host_inclusive_ms'] - res['plain_call_host_inclusive_ms'], 3)
    res['call_vertices'], res['call_faces'] = (int(out['surface']['surface'][k].shape[0]) for k in ('vertices', 'faces'))
    res['call_output_unchanged'] = bool(np.array_equal(out['plain']['implicit_output'], out['surface']['implicit_output'], equal_nan=True))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
