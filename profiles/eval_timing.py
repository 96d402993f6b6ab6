"""Times evaluation.EvalStats.add_frame at the published size (534 528 queries of one output frame; a 14 336-point GREATER target,
a 57 000-point CARLA target with 13 classes) against a numpy restatement of the same statistics on the same box.

    python profiles/eval_timing.py [--repeats 10] [--warmup 3]

Per workload, device time by HIP events (median of the repeats after the warm-up, `x_ms_range` = [min, max]): `add_frame` (both
1-NN searches, the solid split with its 4-byte read, the two statistics passes), `searches` (the two ops.knn calls alone),
`stats_pass` (occ4d_eval_target_stats_f32 + occ4d_eval_query_stats_f32 alone, search results given) and `numpy_stats` (the
restatement of tests/eval_cases.py on the host, search results given, median of 3: what a caller would write over the arrays
perform_inference hands back; it never runs the code under test).  Run the command more than once to see the spread between
processes.  The clouds are seeded uniform samples of the scene cuboid, about a fifth of the queries predicted solid."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import occlusions4d_amd as pk  # noqa: E402
import eval_cases as ec  # noqa: E402
from frontend_timing import _put, time_device, time_host  # noqa: E402

N_QUERY = 534528


def workload(kind, seed):
    rng = np.random.default_rng(seed)
    m, dt, C, half = (14336, 9, 0, 5.0) if kind == 'greater' else (57000, 11, 13, 20.0)
    q = rng.uniform(-half, half, size=(N_QUERY, 4)).astype(np.float32)
    out = rng.uniform(0, 1, size=(N_QUERY, 5 + C)).astype(np.float32)
    out[:, 0] = out[:, 0] ** 3                                    # P(density >= 0.5) = 0.21
    target = rng.uniform(0, 1, size=(m, dt)).astype(np.float32)
    target[:, :3] = rng.uniform(-half, half, size=(m, 3))
    if kind == 'carla':
        target[:, 5] = rng.integers(0, C, size=m)
    group = (rng.uniform(size=m) < 0.5).astype(np.int32)
    return q, out, target, group, C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), queries=N_QUERY)
    for kind in ('greater', 'carla'):
        q, out, target, group, C = workload(kind, 1 if kind == 'greater' else 2)
        qd, od, td, gd = (torch.from_numpy(x).to(dev) for x in (q, out, target, group))
        kw = dict(density_threshold=0.5, point_occupancy_radius=0.2, color_mode='rgb', predict_segmentation=C > 0, track_mode='one',
                  data_kind=kind, target_group=gd)
        stats = pk.evaluation.EvalStats(2, C, dev)
        res[kind + '_target_points'] = target.shape[0]
        _put(res, kind + '_add_frame_ms', time_device(lambda: stats.add_frame(qd, od, td, **kw), a.warmup, a.repeats)[0])
        solid = pk.ops.split_solid_air(qd, od, 0.5)[0]
        res[kind + '_solid_queries'] = solid.shape[0]

        def searches():
            return (pk.ops.knn(qd[:, :3], td[:, :3], 1, metric=1, return_dist=True), pk.ops.knn(td[:, :3], solid[:, :3], 1, metric=1, return_dist=True))
        (idx, dist), (_, back) = searches()
        _put(res, kind + '_searches_ms', time_device(searches, a.warmup, a.repeats)[0])
        cols = pk.evaluation.TARGET_COLUMNS[kind]
        flags = ec.FLAG_COLOR | ec.FLAG_TRACK | (ec.FLAG_SEG if C else 0)

        def passes():
            pk.ops.eval_target_stats(back[:, 0], stats.counts, stats.sums, n_groups=2, n_classes=C, target_group=gd)
            pk.ops.eval_query_stats(od, idx[:, 0], dist[:, 0], td, stats.counts, stats.sums, n_groups=2, n_classes=C, density_threshold=0.5,
                                    radius=0.2, flags=flags, out_track=4, target_group=gd, **cols)
        _put(res, kind + '_stats_pass_ms', time_device(passes, a.warmup, a.repeats)[0])
        stats.summary()                                            # (no bad rows)
        idx_h, dist_h, back_h = idx[:, 0].cpu().numpy(), dist[:, 0].cpu().numpy(), back[:, 0].cpu().numpy()
        _put(res, kind + '_numpy_stats_ms',
             time_host(lambda: ec.restate(out, idx_h, dist_h, target, radius=0.2, threshold=0.5, target_group=group, comp_dist=back_h,
                                          n_groups=2, n_classes=C, flags=flags, out_track=4, **cols)))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
