"""Times the next best view (ops.grid_visible / ops.viewplan_greedy: occ4d_viewplan_visible_u32 / occ4d_viewplan_greedy_u32) at the
published grid -- the GREATER configuration's geometry.grid_counts for 524 288 samples = 96 x 96 x 58 = 534 528 queries -- against THE
EXISTING WAY to the same numbers, and what perform_inference(next_view=NextView(...)) adds to a call with sight=.  Not a test: it sets
no pass mark but one: both ways must give EQUAL gain.

    python profiles/viewplan_timing.py [--repeats 20] [--warmup 3] [--no-call]

Three fields, level 0.5: the six-blob synthetic field of profiles/surface_timing.py, the density column the untrained synthetic scene
of profiles/refine_timing.py decodes to, and an all-free grid.  The targets are the queries with seen == 0 under the three origins
inside the grid of profiles/sight_timing.py (on the all-free grid there are none: every wave skips).  C = 16 and 256 candidates on a
ring round the scene, outside the grid, at two thirds of its height; k = 8; no range limit.  Timed per field and C, device time by HIP
events and the host-inclusive wall clock, median of the repeats after the warm-up, `x_ms_range` = [min, max]:
  - vis: ops.grid_visible on bits and targets made before;  greedy: ops.viewplan_greedy on that vis;  both: the two in a row;
    plan: sight.plan, which also packs the solid set and the targets;
  - THE EXISTING WAY, in the same run on the same build: ceil(C / 31) calls of sight.look, each followed by the torch operations
    that pick the bits of `seen` apart and count, per candidate, the unseen queries it sees -- the same `gain`, asserted EQUAL.  It
    keeps no per-candidate visibility, so a greedy choice would cost it more; that is not added.
  - targets_share: the share of the queries that are targets = the share of the (candidate, query) pairs that are walked;
    waves_share: the share of the 64-query runs that hold a target = the share of the waves that walk at all.
  - perform_inference on the synthetic scene with sight=Sight(three origins) and with next_view=NextView(256 candidates, k = 8)
    beside it, the two calls ALTERNATING in one process.  The call without next_view is the code path from before this feature,
    unchanged: its range is the spread to read the difference against.
Run the command three times to see the spread between processes.  A trained model's gains are not measured: there is no checkpoint.
The g++ twin is not tuned and is not timed."""
import argparse
import json
import math
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
from sight_timing import origin_sets  # noqa: E402
from surface_timing import BATCH, N_POINTS, NUM_SAMPLE, SEED, VIDEO_LEN, blob_field  # noqa: E402

K = 8
MAX_ORIGINS = pk.sight.MAX_ORIGINS


def ring(counts, C):
    """C lattice points on a circle round the grid's axis, outside the grid, at two thirds of its height."""
    nx, ny, nz = counts
    radius = 0.75 * math.hypot(nx, ny)
    angle = 2 * np.pi * np.arange(C) / C
    return np.stack([np.floor(nx / 2 + radius * np.cos(angle)), np.floor(ny / 2 + radius * np.sin(angle)), np.full(C, 2 * nz // 3)], 1).astype(np.int32)


def existing_gain(field, counts, seen, cand):
    """The existing way to `gain`: sight.look 31 candidates at a time, then per candidate the count of the unseen queries whose bit
    is set."""
    unseen = seen == 0
    parts = []
    for start in range(0, len(cand), MAX_ORIGINS):
        chunk = cand[start:start + MAX_ORIGINS]
        seen_c = pk.sight.look(field, counts, chunk, 0.5)[0]
        shifts = torch.arange(len(chunk), dtype=torch.int32, device=seen_c.device)
        parts.append((((seen_c[None, :] >> shifts[:, None]) & 1).bool() & unseen[None, :]).sum(1, dtype=torch.int32))
    return torch.cat(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-call', action='store_true', help='skip the perform_inference comparison')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads(),
               chunk=pk._lib.VIEWPLAN_CONSTANTS['CHUNK'])
    pa, ia, inf = pk.configs.model_args('greater', N_POINTS)
    counts, mins, spacings = pk.geometry.grid_frame(NUM_SAMPLE, inf['min_z'], inf['cube_bounds'], 'greater', inf['cube_mode'])
    counts = tuple(int(c) for c in counts)
    n = counts[0] * counts[1] * counts[2]
    res.update(grid=list(counts), queries=n, k=K)

    esd, dsd = pk.configs.synthetic_weights(pa, ia, SEED)
    enc = pk.model.PointCompletionNetV3(**pa).to(dev).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).to(dev).eval()
    dec.load_state_dict(dsd)
    pcl = pk.configs.synthetic_pcl('greater', N_POINTS, VIDEO_LEN, SEED)

    def call(sight, next_view):
        return pk.inference.perform_inference(
            pcl.clone(), None, None, [enc, dec], dev, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], 3, None,
            sample_implicit=True, num_sample=NUM_SAMPLE, point_sample_mode='grid', batch_size=BATCH,
            predict_segmentation=inf['predict_segmentation'], track_mode='none', semantic_classes=13, density_threshold=0.5,
            data_kind='greater', cube_mode=inf['cube_mode'], compress_air=True, sight=sight, next_view=next_view)

    scene = torch.from_numpy(call(None, None)['implicit_output']).to(dev)
    blobs = torch.from_numpy(blob_field(counts, np.random.default_rng(SEED))).to(dev)
    fields = dict(blobs=blobs, scene=scene, free=torch.zeros((n, 1), device=dev))
    origins = np.array(origin_sets(counts)['3_inside'], np.int32)
    for name, field in fields.items():
        bits = pk.ops.grid_solid_bits(field[:, 0], 0.5)
        seen = pk.sight.look(field, counts, origins, 0.5)[0]
        targets = pk.ops.grid_blocked_bits(seen, 1)
        unseen = seen == 0
        res[name + '_solid_share'] = round(float((field[:, 0] >= 0.5).float().mean()), 4)
        res[name + '_targets_share'] = round(float(unseen.float().mean()), 4)
        runs = torch.nn.functional.pad(unseen.to(torch.uint8), (0, -n % 64)).view(-1, 64).any(1)
        res[name + '_waves_share'] = round(float(runs.float().mean()), 4)
        for C in (16, 256):
            cand_np = ring(counts, C)
            cand = torch.from_numpy(cand_np).to(dev)
            key = '%s_C%d' % (name, C)
            vis = pk.ops.grid_visible(bits, counts, targets, cand)
            work = torch.empty(pk.ops.viewplan_work_len(C, vis.shape[1]), dtype=torch.int32, device=dev)

            def both():
                return pk.ops.viewplan_greedy(pk.ops.grid_visible(bits, counts, targets, cand, out=vis.view(-1)), targets, K, work=work)
            for what, fn in (('vis', lambda: pk.ops.grid_visible(bits, counts, targets, cand, out=vis.view(-1))),
                             ('greedy', lambda: pk.ops.viewplan_greedy(vis, targets, K, work=work)), ('both', both),
                             ('plan', lambda: pk.sight.plan(field, counts, seen, cand, K, 0.5)),
                             ('existing', lambda: existing_gain(field, counts, seen, cand_np))):
                d, h = time_device(fn, a.warmup, a.repeats)
                _put(res, '%s_%s_device_ms' % (key, what), d)
                _put(res, '%s_%s_host_inclusive_ms' % (key, what), h)
            gain, picks, pick_gain, status = both()
            equal = bool(torch.equal(gain, existing_gain(field, counts, seen, cand_np)))
            assert equal, key + ': the new path and the existing way differ in gain'
            res[key + '_gain_equal_to_existing'] = equal
            res[key + '_existing_over_plan_device'] = round(res[key + '_existing_device_ms'] / max(res[key + '_plan_device_ms'], 1e-6), 2)
            res[key + '_existing_over_plan_host_inclusive'] = round(
                res[key + '_existing_host_inclusive_ms'] / max(res[key + '_plan_host_inclusive_ms'], 1e-6), 2)
            res[key + '_picks'] = picks.cpu().tolist()
            res[key + '_status'] = status.cpu().tolist()

    if not a.no_call:
        mins64, sp64 = np.asarray(mins, np.float64), np.asarray(spacings, np.float64)
        to_world = lambda cells: mins64 + (np.asarray(cells, np.float64) + 0.5) * sp64
        look = pk.sight.Sight(origins=to_world(origins))
        option = pk.sight.NextView(to_world(ring(counts, 256)), k=K)
        times = {m: ([], []) for m in ('sight', 'next_view')}
        out = {}
        for i in range(a.warmup + a.repeats):
            for mode in ('sight', 'next_view'):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                out[mode] = call(look, option if mode == 'next_view' else None)
                e1.record()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if i >= a.warmup:
                    times[mode][0].append(e0.elapsed_time(e1))
                    times[mode][1].append((t1 - t0) * 1e3)
        for mode in ('sight', 'next_view'):
            _put(res, '%s_call_device_ms' % mode, _stats(times[mode][0]))
            _put(res, '%s_call_host_inclusive_ms' % mode, _stats(times[mode][1]))
        res['next_view_adds_ms'] = round(res['next_view_call_host_inclusive_ms'] - res['sight_call_host_inclusive_ms'], 3)
        res['call_picks'] = out['next_view']['next_view']['picks'].tolist()
        res['call_output_unchanged'] = bool(np.array_equal(out['sight']['implicit_output'], out['next_view']['implicit_output'], equal_nan=True)
                                            and np.array_equal(out['sight']['sight']['seen'], out['next_view']['sight']['seen']))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
