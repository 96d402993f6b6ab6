"""Times the watershed segments (ops.grid_watershed: occ4d_watershed_label_i32 / occ4d_components_table_i64 /
occ4d_watershed_peaks_i32) at the published grid -- the GREATER configuration's geometry.grid_counts for 524 288 samples = 534 528
queries -- and what perform_inference(segments=Segments(h)) adds to a call.  Not a test: it sets no pass mark.

    python profiles/watershed_timing.py [--repeats 20] [--warmup 3] [--no-host]

Three fields, level 0.5: the six-blob synthetic field of profiles/surface_timing.py, the density column the untrained synthetic
scene of profiles/refine_timing.py decodes to, and an all-solid grid (every height INT32_MAX: one plateau, the worst case for the
union-find and for one size counter).  The heights are each field's inside2 (ops.grid_distance, target 1), made once, outside the
timed call.  Timed per field, at h = 0 and h = 4 and connectivity 6 and 26:
  - ops.grid_watershed with its 16-byte totals read: device time by HIP events and the host-inclusive wall clock, median of the
    repeats after the warm-up, `x_ms_range` = [min, max]; the segments and the basins it finds;
  - THE YARDSTICK, in the same run on the same build: components.label on the same field (the same union-find, numbering and table,
    without the ascent, the doubling rounds and the peaks);
  - watershed.split (the distance transform and the watershed) once per field;
  - the host path, once per field (h = 4, connectivity 26): the copy of inside2 to the host and the numpy / Python RESTATEMENT of
    tests/watershed_cases.py -- a restatement of the rules written for the tests, not a tuned baseline --, compared EQUAL;
  - perform_inference on the synthetic scene with and without segments=Segments(4), the two calls ALTERNATING in one process.  The
    call without `segments` is the code path from before this feature, unchanged.
Run the command three times to see the spread between processes.  A trained model's fields are not measured: there is no checkpoint.
The g++ twin is not tuned and is not timed."""
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

H_MID = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-host', action='store_true', help='skip the host restatement (seconds per field)')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads())
    pa, ia, inf = pk.configs.model_args('greater', N_POINTS)
    counts, mins, spacings = pk.geometry.grid_frame(NUM_SAMPLE, inf['min_z'], inf['cube_bounds'], 'greater', inf['cube_mode'])
    counts = tuple(int(c) for c in counts)
    n = counts[0] * counts[1] * counts[2]
    res.update(grid=list(counts), queries=n, h_mid=H_MID)

    esd, dsd = pk.configs.synthetic_weights(pa, ia, SEED)
    enc = pk.model.PointCompletionNetV3(**pa).to(dev).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).to(dev).eval()
    dec.load_state_dict(dsd)
    pcl = pk.configs.synthetic_pcl('greater', N_POINTS, VIDEO_LEN, SEED)

    def call(segments):
        return pk.inference.perform_inference(
            pcl.clone(), None, None, [enc, dec], dev, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], 3, None,
            sample_implicit=True, num_sample=NUM_SAMPLE, point_sample_mode='grid', batch_size=BATCH,
            predict_segmentation=inf['predict_segmentation'], track_mode='none', semantic_classes=13, density_threshold=0.5,
            data_kind='greater', cube_mode=inf['cube_mode'], compress_air=True, segments=segments)

    scene = torch.from_numpy(call(None)['implicit_output']).to(dev)
    fields = dict(blobs=torch.from_numpy(blob_field(counts, np.random.default_rng(SEED))).to(dev), scene=scene,
                  solid=torch.ones((n, 1), device=dev))
    for name, field in fields.items():
        inside2 = pk.ops.grid_distance(field[:, 0], counts, 0.5, target=1)[0]
        res[name + '_solid_share'] = round(float((inside2 >= 1).float().mean()), 4)
        res[name + '_deepest'] = int(inside2.max())
        _put(res, name + '_split_host_inclusive_ms', time_device(lambda: pk.watershed.split(field, counts, 0.5, H_MID), a.warmup, a.repeats)[1])
        for connectivity in (6, 26):
            key = '%s_%d' % (name, connectivity)
            d, h = time_device(lambda: pk.components.label(field, counts, 0.5, connectivity), a.warmup, a.repeats)
            _put(res, key + '_components_label_device_ms', d)
            _put(res, key + '_components_label_host_inclusive_ms', h)
            res[key + '_components'] = int(pk.components.label(field, counts, 0.5, connectivity)[1].shape[0])
            for hh in (0, H_MID):
                k2 = '%s_h%d' % (key, hh)
                totals = pk.ops.grid_watershed(inside2, counts, hh, connectivity)[1].cpu().tolist()
                res[k2 + '_segments'], res[k2 + '_basins'] = totals[0], totals[3]
                d, h = time_device(lambda: pk.ops.grid_watershed(inside2, counts, hh, connectivity), a.warmup, a.repeats)
                _put(res, k2 + '_device_ms', d)
                _put(res, k2 + '_host_inclusive_ms', h)
                res[k2 + '_over_components_label'] = round(res[k2 + '_host_inclusive_ms'] / res[key + '_components_label_host_inclusive_ms'], 2)
        if not a.no_host:
            import watershed_cases as wc
            got = {}
            _put(res, name + '_host_restatement_ms',
                 time_host(lambda: got.update(r=wc.restate(inside2.cpu().numpy(), counts, 26, H_MID)), repeats=1))
            out = pk.ops.grid_watershed(inside2, counts, H_MID, 26)
            res[name + '_equal_to_restatement'] = bool(all(np.array_equal(got['r'][k], t.cpu().numpy())
                                                           for k, t in zip(('labels', 'totals', 'table', 'peaks'), out)))

    # what segments= adds to a call
    times = {m: ([], []) for m in ('plain', 'segments')}
    out = {}
    for i in range(a.warmup + a.repeats):
        for mode in ('plain', 'segments'):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out[mode] = call(pk.watershed.Segments(H_MID) if mode == 'segments' else None)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= a.warmup:
                times[mode][0].append(e0.elapsed_time(e1))
                times[mode][1].append((t1 - t0) * 1e3)
    for mode in ('plain', 'segments'):
        _put(res, '%s_call_device_ms' % mode, _stats(times[mode][0]))
        _put(res, '%s_call_host_inclusive_ms' % mode, _stats(times[mode][1]))
    res['segments_adds_ms'] = round(res['segments_call_host_inclusive_ms'] - res['plain_call_host_inclusive_ms'], 3)
    res['call_segments'] = int(out['segments']['segments']['table'].shape[0])
    res['call_output_unchanged'] = bool(np.array_equal(out['plain']['implicit_output'], out['segments']['implicit_output'], equal_nan=True))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
