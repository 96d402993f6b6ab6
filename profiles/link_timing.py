"""Times the linking of the components of two consecutive output frames (ops.components_overlap + ops.components_match:
occ4d_link_overlap_i32 / occ4d_link_match_i32, eleven launches) at the published grid -- the GREATER configuration's
geometry.grid_counts for 524 288 samples = 534 528 queries -- and what perform_inference(components=..., tracker=Tracker()) adds to
a perform_inference(components=...) call.  Not a test: it sets no pass mark.

    python profiles/link_timing.py [--repeats 20] [--warmup 3]

Three pairs of frames, labelled at connectivity 6, level 0.5: the six-blob synthetic field of profiles/surface_timing.py and the same
field shifted by two voxels along x; the density columns the untrained synthetic scene of profiles/refine_timing.py decodes to at
two consecutive output times (thousands of components); an all-solid grid twice (ONE pair of n points: the worst case for
contention on a table slot).  Timed per pair of frames:
  - overlap + match with no host read: device time by HIP events and the host-inclusive wall clock, median of the repeats after
    the warm-up, `x_ms_range` = [min, max];
  - the host path on the same box: the numpy / Python-integer restatement of tests/link_cases.py (a packed-key np.unique, then the
    order relation in Python integers) on the labels and tables already on the host, as a perform_inference call returns them;
    its pairs and links are compared EQUAL with the device's (`equal_to_host`) in every run;
  - perform_inference on the synthetic scene with components=Components() and with tracker=Tracker() on top, the two calls
    ALTERNATING in one process.  The call without `tracker` is the code path from before this feature, unchanged.
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
import link_cases as lc  # noqa: E402

MIN_IOU = (1, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads(),
               launches=11)
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

    def call(time_idx, components=None, tracker=None):
        return pk.inference.perform_inference(
            pcl.clone(), None, None, [enc, dec], dev, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], time_idx, None,
            sample_implicit=True, num_sample=NUM_SAMPLE, point_sample_mode='grid', batch_size=BATCH,
            predict_segmentation=inf['predict_segmentation'], track_mode='none', semantic_classes=13, density_threshold=0.5,
            data_kind='greater', cube_mode=inf['cube_mode'], compress_air=True, components=components, tracker=tracker)

    blobs = blob_field(counts, np.random.default_rng(SEED))[:, :1]
    moved = np.roll(blobs.reshape(counts), 2, axis=0).reshape(-1, 1)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    fields = dict(blobs=(to(blobs), to(moved)), scene=(to(call(2)['implicit_output'][:, :1]), to(call(3)['implicit_output'][:, :1])),
                  solid=(torch.ones((n, 1), device=dev), torch.ones((n, 1), device=dev)))
    next_id = torch.full((1,), 1000, dtype=torch.int32, device=dev)
    for name, (first, second) in fields.items():
        (la, ta), (lb, tb) = (pk.components.label(f, counts, 0.5, 6) for f in (first, second))
        k_a, k_b = ta.shape[0], tb.shape[0]
        track_a = torch.arange(k_a, dtype=torch.int32, device=dev)

        def link():
            pairs, totals = pk.ops.components_overlap(la, lb, k_a, k_b)
            return pairs, totals, pk.ops.components_match(pairs, totals, ta, tb, track_a, next_id, MIN_IOU)

        pairs, totals, (links, best_a, next_out) = link()
        totals_h = totals.tolist()
        res.update({name + '_components': [k_a, k_b], name + '_pairs': totals_h[0], name + '_member_points': totals_h[1],
                    name + '_overflow': totals_h[2], name + '_cap': int(pairs.shape[0]),
                    name + '_work_MiB': round(pk.ops.link_work_len(n, pairs.shape[0]) * 4 / 2 ** 20, 1),
                    name + '_linked': int((links[:, 1] >= 0).sum())})
        d, h = time_device(link, a.warmup, a.repeats)
        _put(res, name + '_device_ms', d)
        _put(res, name + '_host_inclusive_ms', h)
        la_h, lb_h, ta_h, tb_h, track_h = (t.cpu().numpy() for t in (la, lb, ta, tb, track_a))
        got = {}

        def host_overlap():
            got['pairs'] = lc.restate_overlap(la_h, lb_h, k_a, k_b)[0]

        def host_match():
            got['match'] = lc.restate_match(got['pairs'], ta_h[:, 0], tb_h[:, 0], track_h, 1000, *MIN_IOU)

        _put(res, name + '_host_unique_ms', time_host(host_overlap, repeats=3))
        _put(res, name + '_host_match_ms', time_host(host_match, repeats=3))
        res[name + '_host_ms'] = round(res[name + '_host_unique_ms'] + res[name + '_host_match_ms'], 3)
        res[name + '_equal_to_host'] = bool(
            np.array_equal(pairs[:totals_h[0]].cpu().numpy(), got['pairs']) and np.array_equal(links.cpu().numpy(), got['match'][0])
            and np.array_equal(best_a.cpu().numpy(), got['match'][1]) and int(next_out.item()) == got['match'][2])
        res[name + '_host_over_device'] = round(res[name + '_host_ms'] / res[name + '_host_inclusive_ms'], 1)

    # what tracker= adds to a call with components=: consecutive output times, alternating
    times = {m: ([], []) for m in ('components', 'tracker')}
    out = {}
    tracker = pk.components.Tracker(min_iou=MIN_IOU)
    for i in range(a.warmup + a.repeats):
        for mode in ('components', 'tracker'):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out[mode] = call(2 + i % 2, pk.components.Components(), tracker if mode == 'tracker' else None)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= a.warmup:
                times[mode][0].append(e0.elapsed_time(e1))
                times[mode][1].append((t1 - t0) * 1e3)
    for mode in ('components', 'tracker'):
        _put(res, '%s_call_device_ms' % mode, _stats(times[mode][0]))
        _put(res, '%s_call_host_inclusive_ms' % mode, _stats(times[mode][1]))
    res['tracker_adds_ms'] = round(res['tracker_call_host_inclusive_ms'] - res['components_call_host_inclusive_ms'], 3)
    res['call_tracks'] = tracker.n_tracks()
    res['call_linked'] = int((out['tracker']['components']['link'][:, 1] >= 0).sum())
    res['call_output_unchanged'] = bool(np.array_equal(out['components']['components']['labels'], out['tracker']['components']['labels']))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
