"""Times the pull of traced paths into waypoints (ops.grid_blocked_bits + ops.geodesic_pull: occ4d_pull_bits_i32, occ4d_pull_paths_i32)
and pairwise line of sight (ops.grid_segments: occ4d_pull_pairs_u32) at the published grid -- the GREATER configuration's
geometry.grid_counts for 524 288 samples = 534 528 queries -- and what Route(..., pull=True) adds to a perform_inference call with a
route.  Not a test: it sets no pass mark.

    python profiles/pull_timing.py [--repeats 20] [--warmup 3] [--restate-goals 2]

The three fields of profiles/geodesic_timing.py (six blobs, the untrained synthetic scene, all free), blocked = dist2 < 1 of
ops.grid_distance at level 0.5, the same seeds; 1, 16 and 256 goals: the reached query farthest from the seed by cost, then seeded
random reached ones.  Recorded per field and goal count:
  - the mean number of points and of waypoints per path, and the mean of polyline_length(waypoints) / polyline_length(paths) over
    the paths of more than one point (spacings of the grid);
  - ops.grid_blocked_bits + ops.geodesic_pull (no host read): device time by HIP events and the host-inclusive wall clock, median of
    the repeats after the warm-up, `x_ms_range` = [min, max].  The kernel walks a copy of the bits in LDS at this grid; while it was
    being decided, a build that chose between that copy and global memory by an environment variable ran both in this loop, in
    the same runs -- DESIGN 7c rank 20 has both sets of figures;
  - beside it, in the same run, ops.grid_geodesic(parent=True) + ops.geodesic_trace, which make the paths;
  - the restatement of tests/pull_cases.py on the host for the first --restate-goals goals -- dist2's copy, then plain Python loops
    over sight_cases.walk_scalar: A RESTATEMENT OF THE RULES, NOT A TUNED BASELINE -- with its results compared EQUAL with the
    device's (`equal_to_restatement`);
and once per field ops.grid_segments at 534 528 seeded random pairs.  Then perform_inference on the synthetic scene with
route=Route(seed, goals) and with pull=True as well, the two calls ALTERNATING in one process; the call with pull=False is the code
path from before this feature, unchanged.  Run the command three times to see the spread between processes.  An untrained network's
field says nothing about a trained one's.  The g++ twin is not tuned and is not timed."""
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

NONE = pk.geodesic.NONE
GOAL_COUNTS = (1, 16, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--restate-goals', type=int, default=2)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads())
    pa, ia, inf = pk.configs.model_args('greater', N_POINTS)
    counts, mins, spacings = pk.geometry.grid_frame(NUM_SAMPLE, inf['min_z'], inf['cube_bounds'], 'greater', inf['cube_mode'])
    counts = tuple(int(c) for c in counts)
    n = counts[0] * counts[1] * counts[2]
    cap = 4 * max(counts)
    res.update(grid=list(counts), queries=n, path_cap=cap, round=pk._lib.PULL_CONSTANTS['ROUND'])

    esd, dsd = pk.configs.synthetic_weights(pa, ia, SEED)
    enc = pk.model.PointCompletionNetV3(**pa).to(dev).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).to(dev).eval()
    dec.load_state_dict(dsd)
    pcl = pk.configs.synthetic_pcl('greater', N_POINTS, VIDEO_LEN, SEED)

    def call(route):
        return pk.inference.perform_inference(
            pcl.clone(), None, None, [enc, dec], dev, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], 3, None,
            sample_implicit=True, num_sample=NUM_SAMPLE, point_sample_mode='grid', batch_size=BATCH,
            predict_segmentation=inf['predict_segmentation'], track_mode='none', semantic_classes=13, density_threshold=0.5,
            data_kind='greater', cube_mode=inf['cube_mode'], compress_air=True, clearance=pk.distance.Clearance(), route=route)

    scene = torch.from_numpy(call(None)['implicit_output']).to(dev)
    fields = dict(blobs=torch.from_numpy(blob_field(counts, np.random.default_rng(SEED))).to(dev)[:, 0], scene=scene[:, 0],
                  free=torch.zeros(n, device=dev))
    middle = ((counts[0] // 2) * counts[1] + counts[1] // 2) * counts[2] + counts[2] // 2
    xyz = np.stack(np.meshgrid(*(np.arange(c, dtype=np.int64) for c in counts), indexing='ij'), -1).reshape(-1, 3)
    scene_points = None
    for name, column in fields.items():
        dist2 = pk.ops.grid_distance(column, counts, 0.5)[0]
        host_dist2 = dist2.cpu().numpy()
        free = np.flatnonzero(host_dist2 >= 1)
        seed = int(free[np.argmin(((xyz[free] - xyz[middle]) ** 2).sum(-1))]) if name == 'scene' else int(free[0])
        seeds = torch.tensor([seed], dtype=torch.int32, device=dev)
        cost, status, up = pk.ops.grid_geodesic(dist2, counts, seeds, parent=True)
        host_cost = cost.cpu().numpy()
        reached = np.flatnonzero((host_cost != NONE) & (host_cost > 0))
        order = np.concatenate([[reached[np.argmax(host_cost[reached])]], np.random.default_rng(SEED).permutation(reached)])
        res.update({name + '_converged': int(status.cpu()[0]), name + '_blocked_share': round(1 - len(free) / n, 4)})
        if name == 'scene':
            scene_points = seed, order
        for G in GOAL_COUNTS:
            key = '%s_g%d' % (name, G)
            goals = torch.from_numpy(order[:G].astype(np.int32)).to(dev)
            paths, path_len = pk.ops.geodesic_trace(cost, up, goals, cap)
            d, h = time_device(lambda: pk.ops.geodesic_trace(*pk.ops.grid_geodesic(dist2, counts, seeds, parent=True)[::2], goals, cap),
                               a.warmup, a.repeats)
            _put(res, key + '_geodesic_trace_device_ms', d)
            _put(res, key + '_geodesic_trace_host_inclusive_ms', h)
            pull = lambda: pk.ops.geodesic_pull(pk.ops.grid_blocked_bits(dist2, 1), counts, paths, path_len)
            way, way_len = (t.cpu().numpy() for t in pull())
            d, h = time_device(pull, a.warmup, a.repeats)
            _put(res, key + '_pull_device_ms', d)
            _put(res, key + '_pull_host_inclusive_ms', h)
            host_paths, host_len = paths.cpu().numpy(), path_len.cpu().numpy()
            long = pk.geodesic.polyline_length(host_paths, host_len, spacings, counts)
            short = pk.geodesic.polyline_length(way, way_len, spacings, counts)
            several = host_len > 1
            res.update({key + '_mean_points': round(float(host_len.mean()), 2), key + '_mean_waypoints': round(float(way_len.mean()), 2),
                        key + '_length_ratio': round(float((short[several] / long[several]).mean()), 4) if several.any() else None})
            if G == GOAL_COUNTS[0] and a.restate_goals > 0:
                import pull_cases as pc
                k = min(a.restate_goals, G)
                t0 = time.perf_counter()
                want = pc.pull_all(pc.blocked_of(dist2.cpu().numpy(), 1), counts, host_paths[:k], host_len[:k])
                res[key + '_restatement_goals'] = k
                res[key + '_restatement_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
                res[key + '_equal_to_restatement'] = bool(np.array_equal(want[0], way[:k]) and np.array_equal(want[1], way_len[:k]))
                assert res[key + '_equal_to_restatement'], key
        # pairwise line of sight: as many pairs as the grid has points
        rng = np.random.default_rng(SEED + 1)
        pa_, pb_ = (torch.from_numpy(rng.integers(0, n, size=n).astype(np.int32)).to(dev) for _ in range(2))
        blocked = pk.ops.grid_blocked_bits(dist2, 1)
        hit = pk.ops.grid_segments(blocked, counts, pa_, pb_).cpu().numpy()
        res[name + '_pairs'] = n
        res[name + '_pairs_free_share'] = round(float((hit == -1).mean()), 4)
        d, h = time_device(lambda: pk.ops.grid_segments(blocked, counts, pa_, pb_), a.warmup, a.repeats)
        _put(res, name + '_pairs_device_ms', d)
        _put(res, name + '_pairs_host_inclusive_ms', h)

    # what pull=True adds to a call that has a route with goals
    seed, order = scene_points
    for G in (1, 16):
        routes = {mode: pk.geodesic.Route([seed], order[:G].astype(np.int64), pull=mode == 'pull') for mode in ('route', 'pull')}
        times = {m: ([], []) for m in routes}
        out = {}
        for i in range(a.warmup + a.repeats):
            for mode in routes:
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                out[mode] = call(routes[mode])
                e1.record()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if i >= a.warmup:
                    times[mode][0].append(e0.elapsed_time(e1))
                    times[mode][1].append((t1 - t0) * 1e3)
        for mode in routes:
            _put(res, 'call_g%d_%s_device_ms' % (G, mode), _stats(times[mode][0]))
            _put(res, 'call_g%d_%s_host_inclusive_ms' % (G, mode), _stats(times[mode][1]))
        res['call_g%d_pull_adds_ms' % G] = round(res['call_g%d_pull_host_inclusive_ms' % G] - res['call_g%d_route_host_inclusive_ms' % G], 3)
        res['call_g%d_rest_unchanged' % G] = bool(all(np.array_equal(out['route']['route'][k], out['pull']['route'][k]) for k in out['route']['route'])
                                                  and np.array_equal(out['route']['implicit_output'], out['pull']['implicit_output'], equal_nan=True))
        res['call_g%d_waypoint_len' % G] = out['pull']['route']['waypoint_len'].tolist()
        res['call_g%d_path_len' % G] = out['pull']['route']['path_len'].tolist()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
