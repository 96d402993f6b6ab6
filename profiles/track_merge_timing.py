"""Times perform_inference(track_mode='all') with the reruns merged on the device against the merge on the host, at the
published size: the GREATER configuration, 14 336 input points, the 534 528-query grid, a synthetic clip with 5 tracked
instances, compress_air=True.  Not a test: it asserts nothing.

    python profiles/track_merge_timing.py [--repeats 10] [--warmup 3] [--instances 5]

The two modes ALTERNATE in one process (host, device, host, device, ...): device time by HIP events around the call and the
host-inclusive wall clock of the same call, median of the repeats after the warm-up, `x_ms_range` = [min, max]; run the
command three times to see the spread between processes.  track_merge='host' is the code path from before the device merge,
unchanged.  Also timed alone: the two merge entry points (K adds with the squash codes + the finish, on the three accumulators
of a call) and numpy's multi_track_merge on host arrays of the same sizes."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import occlusions4d_amd as pk  # noqa: E402
from frontend_timing import _put, _stats, time_device, time_host  # noqa: E402

N_POINTS, VIDEO_LEN, NUM_SAMPLE, BATCH, SEED = 14336, 12, 524288, 32768, 1830


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--instances', type=int, default=5)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    K = a.instances
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads(),
               instances=K)
    pa, ia, inf = pk.configs.model_args('greater', N_POINTS)
    esd, dsd = pk.configs.synthetic_weights(pa, ia, SEED)
    enc = pk.model.PointCompletionNetV3(**pa).to(dev).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).to(dev).eval()
    dec.load_state_dict(dsd)
    pcl = pk.configs.synthetic_pcl('greater', N_POINTS, VIDEO_LEN, SEED)
    sem = np.random.default_rng(SEED).integers(-1, K, size=(N_POINTS, 1)).astype(np.float32)

    def call(mode):
        return pk.inference.perform_inference(
            pcl.clone(), sem.copy(), None, [enc, dec], dev, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], 3, None,
            sample_implicit=True, num_sample=NUM_SAMPLE, point_sample_mode='grid', batch_size=BATCH,
            predict_segmentation=inf['predict_segmentation'], track_mode='all', semantic_classes=13, density_threshold=0.5,
            data_kind='greater', cube_mode=inf['cube_mode'], compress_air=True, track_merge=mode)

    # the two modes in alternation, timed as frontend_timing.time_device times one call
    times = {m: ([], []) for m in ('host', 'device')}
    out = {}
    for i in range(a.warmup + a.repeats):
        for mode in ('host', 'device'):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out[mode] = call(mode)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= a.warmup:
                times[mode][0].append(e0.elapsed_time(e1))
                times[mode][1].append((t1 - t0) * 1e3)
    for mode in ('host', 'device'):
        _put(res, 'all_mode_%s_merge_device_ms' % mode, _stats(times[mode][0]))
        _put(res, 'all_mode_%s_merge_host_inclusive_ms' % mode, _stats(times[mode][1]))
    res['queries'], res['channels'] = [int(v) for v in out['host']['implicit_output'].shape]
    res['modes_equal'] = bool(all(np.array_equal(out['host'][k], out['device'][k], equal_nan=True) for k in out['host']))

    # the merge alone: K adds + finish on the three accumulators of a call / numpy on host arrays of the same sizes
    n, g = res['queries'], res['channels']
    track_col = pk.inference.get_track_idx(inf['color_mode'])
    rng = np.random.default_rng(1)
    raw = [torch.from_numpy(rng.normal(size=(n, g)).astype(np.float32)).to(dev) for _ in range(K)]
    abstract = [torch.from_numpy(rng.normal(size=out['host']['pcl_abstract'].shape).astype(np.float32)).to(dev) for _ in range(K)]
    feats = [torch.from_numpy(rng.normal(size=out['host']['features_global'].shape).astype(np.float32)).to(dev) for _ in range(K)]

    post_ops = (inf['color_mode'], inf['predict_segmentation'], 'all', 13)
    no_copies = types.SimpleNamespace(fetch=lambda t: None)          # (the merged arrays' way to the host is not timed here)

    def merge_alone():
        m = pk.inference._DeviceMerge(no_copies, list(range(K)), track_col, post_ops)
        for k in range(K):
            m.add(dict(implicit_output=raw[k], pcl_abstract=abstract[k], features_global=feats[k]), k)
        return m.finish()
    d, h = time_device(merge_alone, a.warmup, a.repeats)
    _put(res, 'merge_entry_points_device_ms', d)
    _put(res, 'merge_entry_points_host_inclusive_ms', h)
    host = [[t.cpu().numpy() for t in part] for part in (abstract, feats, raw)]
    _put(res, 'numpy_multi_track_merge_ms', time_host(lambda: pk.inference.multi_track_merge(list(range(K)), *host, track_col),
                                                      a.repeats))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
