"""Times the connected-component labelling (components.label: occ4d_components_label_f32 / occ4d_components_table_i64) at the published
grid -- the GREATER configuration's geometry.grid_counts for 524 288 samples = 534 528 queries -- and what
perform_inference(components=Components()) adds to a call.  Not a test: it sets no pass mark.

    python profiles/components_timing.py [--repeats 20] [--warmup 3]

Three fields, each at connectivity 6 and 26, level 0.5: the six-blob synthetic field of profiles/surface_timing.py, the density
column the untrained synthetic scene of profiles/refine_timing.py decodes to, and an all-solid grid (one component: the worst case
for contention on a table row and on a size counter).  Timed per field:
  - components.label with its 12-byte totals read: device time by HIP events and the host-inclusive wall clock, median of the
    repeats after the warm-up, `x_ms_range` = [min, max];
  - where scipy is importable, the same table on the same box's CPU: the array's copy to the host, scipy.ndimage.label, np.bincount
    and ndimage.find_objects / ndimage.sum for the sizes, boxes and coordinate sums (scipy is single-threaded: the 16 CPUs of a
    command change nothing); its labels are compared EQUAL with the device's (`equal_to_scipy`);
  - perform_inference on the synthetic scene with and without components=Components(), the two calls ALTERNATING in one process.
    The call without `components` is the code path from before this feature, unchanged.
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


def scipy_table(values, counts, rank):
    """(labels - 1, table without the root and class columns' device rules: size, sums, minima, maxima) with scipy / numpy."""
    solid = values.cpu().numpy().reshape(counts) >= np.float32(0.5)
    lab, count = ndimage.label(solid, structure=ndimage.generate_binary_structure(3, rank))
    size = np.bincount(lab.reshape(-1), minlength=count + 1)[1:]
    boxes = ndimage.find_objects(lab)
    index = np.arange(1, count + 1)
    sums = [ndimage.sum(np.broadcast_to(np.arange(c).reshape([-1 if a == b else 1 for b in range(3)]), counts), lab, index)
            for a, c in enumerate(counts)]
    return lab.reshape(-1).astype(np.int32) - 1, size, boxes, sums


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

    def call(components):
        return pk.inference.perform_inference(
            pcl.clone(), None, None, [enc, dec], dev, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], 3, None,
            sample_implicit=True, num_sample=NUM_SAMPLE, point_sample_mode='grid', batch_size=BATCH,
            predict_segmentation=inf['predict_segmentation'], track_mode='none', semantic_classes=13, density_threshold=0.5,
            data_kind='greater', cube_mode=inf['cube_mode'], compress_air=True, components=components)

    scene = torch.from_numpy(call(None)['implicit_output']).to(dev)
    fields = dict(blobs=torch.from_numpy(blob_field(counts, np.random.default_rng(SEED))).to(dev), scene=scene,
                  solid=torch.ones((n, 1), device=dev))
    for name, field in fields.items():
        for connectivity in (6, 26):
            key = '%s_%d' % (name, connectivity)
            labels, table = pk.components.label(field, counts, 0.5, connectivity)
            res[key + '_components'] = int(table.shape[0])
            res[key + '_solid_share'] = round(float((labels >= 0).float().mean()), 4)
            res[key + '_largest'] = int(table[:, 0].max()) if table.shape[0] else 0
            d, h = time_device(lambda: pk.components.label(field, counts, 0.5, connectivity), a.warmup, a.repeats)
            _put(res, key + '_device_ms', d)
            _put(res, key + '_host_inclusive_ms', h)
            if ndimage is not None:
                got = {}
                _put(res, key + '_scipy_ms', time_host(lambda: got.update(r=scipy_table(field[:, 0], counts, 1 if connectivity == 6 else 3)),
                                                       repeats=3))
                res[key + '_equal_to_scipy'] = bool(np.array_equal(got['r'][0], labels.cpu().numpy())
                                                    and np.array_equal(got['r'][1], table[:, 0].cpu().numpy()))
                res[key + '_scipy_over_device'] = round(res[key + '_scipy_ms'] / res[key + '_host_inclusive_ms'], 1)

    # what components= adds to a call
    times = {m: ([], []) for m in ('plain', 'components')}
    out = {}
    for i in range(a.warmup + a.repeats):
        for mode in ('plain', 'components'):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out[mode] = call(pk.components.Components() if mode == 'components' else None)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= a.warmup:
                times[mode][0].append(e0.elapsed_time(e1))
                times[mode][1].append((t1 - t0) * 1e3)
    for mode in ('plain', 'components'):
        _put(res, '%s_call_device_ms' % mode, _stats(times[mode][0]))
        _put(res, '%s_call_host_inclusive_ms' % mode, _stats(times[mode][1]))
    res['components_adds_ms'] = round(res['components_call_host_inclusive_ms'] - res['plain_call_host_inclusive_ms'], 3)
    res['call_components'] = int(out['components']['components']['table'].shape[0])
    res['call_output_unchanged'] = bool(np.array_equal(out['plain']['implicit_output'], out['components']['implicit_output'], equal_nan=True))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
