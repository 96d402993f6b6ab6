"""Times the oriented boxes (ops.grid_box_extents / ops.boxes_choose: occ4d_boxes_extents_i32 / occ4d_boxes_choose_i32) at the
published grid -- the GREATER configuration's geometry.grid_counts for 524 288 samples = 96 x 96 x 58 = 534 528 queries -- with the
90 headings of components.yaw_directions, against the host path on the same box, and what perform_inference(boxes=Boxes()) adds
to a call with components=.  Not a test: it sets no pass mark but one: both paths must give EQUAL boxes.

    python profiles/boxes_timing.py [--repeats 20] [--warmup 3] [--no-call] [--no-host]

Three fields, level 0.5, labelled by components.label with connectivity 6: the six-blob synthetic field of
profiles/surface_timing.py (one component), the density column the untrained synthetic scene of profiles/refine_timing.py decodes
to (thousands of components), and an all-solid grid (one component, every point a member).  Timed per field, device time by HIP
events and the host-inclusive wall clock, median of the repeats after the warm-up, `x_ms_range` = [min, max]:
  - extents: ops.grid_box_extents on labels made before;  choose: ops.boxes_choose on those extents;  both: the two in a row;
  - the host path, ONE run per process: the labels copied to the host plus the numpy int64 restatement of the tests
    (tests/boxes_cases.py: a restatement, not a tuned baseline), box asserted EQUAL;
  - objects, runs: the number of objects and of runs of equal object labels along z (what the reduce kernel steps through);
  - perform_inference on the synthetic scene with components=Components() and with boxes=Boxes() beside it, the two calls
    ALTERNATING in one process.  The call without boxes is the code path from before this feature, unchanged: its range is the
    spread to read the difference against.
Run the command three times to see the spread between processes.  A trained model's boxes are not measured: there is no checkpoint.
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
from frontend_timing import _put, _stats, time_device  # noqa: E402
from surface_timing import BATCH, N_POINTS, NUM_SAMPLE, SEED, VIDEO_LEN, blob_field  # noqa: E402

N_DIRS = 90


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-call', action='store_true', help='skip the perform_inference comparison')
    ap.add_argument('--no-host', action='store_true', help='skip the host path')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads(),
               constants=pk._lib.BOXES_CONSTANTS, library=os.path.basename(pk._lib.LIB_PATH))
    pa, ia, inf = pk.configs.model_args('greater', N_POINTS)
    counts, mins, spacings = pk.geometry.grid_frame(NUM_SAMPLE, inf['min_z'], inf['cube_bounds'], 'greater', inf['cube_mode'])
    counts = tuple(int(c) for c in counts)
    n = counts[0] * counts[1] * counts[2]
    table = pk.components.yaw_directions(spacings, N_DIRS)['table']
    dirs = torch.from_numpy(table).to(dev)
    res.update(grid=list(counts), queries=n, directions=N_DIRS, spacings=[float(s) for s in spacings])

    esd, dsd = pk.configs.synthetic_weights(pa, ia, SEED)
    enc = pk.model.PointCompletionNetV3(**pa).to(dev).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).to(dev).eval()
    dec.load_state_dict(dsd)
    pcl = pk.configs.synthetic_pcl('greater', N_POINTS, VIDEO_LEN, SEED)

    def call(components, boxes):
        return pk.inference.perform_inference(
            pcl.clone(), None, None, [enc, dec], dev, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], 3, None,
            sample_implicit=True, num_sample=NUM_SAMPLE, point_sample_mode='grid', batch_size=BATCH,
            predict_segmentation=inf['predict_segmentation'], track_mode='none', semantic_classes=13, density_threshold=0.5,
            data_kind='greater', cube_mode=inf['cube_mode'], compress_air=True, components=components, boxes=boxes)

    scene = torch.from_numpy(call(None, None)['implicit_output']).to(dev)
    blobs = torch.from_numpy(blob_field(counts, np.random.default_rng(SEED))).to(dev)
    fields = dict(blobs=blobs, scene=scene, solid=torch.ones((n, 1), device=dev))
    if not a.no_host:
        import boxes_cases as bc
    for name, field in fields.items():
        labels, tab = pk.components.label(field, counts, 0.5, 6)
        K = int(tab.shape[0])
        lab = labels.view(counts)
        member = lab >= 0
        heads = member.clone()
        heads[:, :, 1:] &= lab[:, :, 1:] != lab[:, :, :-1]
        res[name + '_objects'], res[name + '_points'], res[name + '_runs'] = K, int(member.sum()), int(heads.sum())
        extent = torch.empty((K * N_DIRS * 4,), dtype=torch.int32, device=dev)
        zr = torch.empty((K * 3,), dtype=torch.int32, device=dev)
        box = torch.empty((K * 8,), dtype=torch.int32, device=dev)
        ext = lambda: pk.ops.grid_box_extents(labels, counts, K, dirs, out=(extent, zr))
        e, z = ext()

        def both():
            e, z = ext()
            return pk.ops.boxes_choose(e, z, dirs, out=box)
        for what, fn in (('extents', ext), ('choose', lambda: pk.ops.boxes_choose(e, z, dirs, out=box)), ('both', both)):
            d, h = time_device(fn, a.warmup, a.repeats)
            _put(res, '%s_%s_device_ms' % (name, what), d)
            _put(res, '%s_%s_host_inclusive_ms' % (name, what), h)
        got = both().cpu().numpy()
        res[name + '_first_boxes'] = got[:3].tolist()
        if not a.no_host:
            t0 = time.perf_counter()
            host_labels = labels.cpu().numpy()
            t1 = time.perf_counter()
            want_e, want_z = bc.restate_extents(host_labels, counts, K, table)
            want = bc.restate_choose(want_e, want_z, table)
            t2 = time.perf_counter()
            assert np.array_equal(got, want), name + ': the device and the host path differ'
            res[name + '_host_copy_ms'], res[name + '_host_path_ms'] = round((t1 - t0) * 1e3, 3), round((t2 - t0) * 1e3, 1)
            res[name + '_host_over_both_host_inclusive'] = round(res[name + '_host_path_ms'] / max(res[name + '_both_host_inclusive_ms'], 1e-6), 1)
            res[name + '_box_equal_to_host'] = True

    if not a.no_call:
        comp, option = pk.components.Components(), pk.components.Boxes(n=N_DIRS)
        times = {m: ([], []) for m in ('components', 'boxes')}
        out = {}
        for i in range(a.warmup + a.repeats):
            for mode in ('components', 'boxes'):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                out[mode] = call(comp, option if mode == 'boxes' else None)
                e1.record()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if i >= a.warmup:
                    times[mode][0].append(e0.elapsed_time(e1))
                    times[mode][1].append((t1 - t0) * 1e3)
        for mode in ('components', 'boxes'):
            _put(res, '%s_call_device_ms' % mode, _stats(times[mode][0]))
            _put(res, '%s_call_host_inclusive_ms' % mode, _stats(times[mode][1]))
        res['boxes_adds_ms'] = round(res['boxes_call_host_inclusive_ms'] - res['components_call_host_inclusive_ms'], 3)
        res['call_objects'] = int(out['boxes']['components']['box'].shape[0])
        res['call_output_unchanged'] = bool(np.array_equal(out['components']['implicit_output'], out['boxes']['implicit_output'], equal_nan=True)
                                            and np.array_equal(out['components']['components']['labels'], out['boxes']['components']['labels']))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
