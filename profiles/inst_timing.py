"""Times evaluation.InstanceStats.add_frame at the published size (534 528 queries of one output frame, a 14 336-point GREATER
target, 12 instance ids, about 110 K predicted-solid rows; inputs on the device) against a numpy restatement of the same tables
and fold on the same box.

    python profiles/inst_timing.py [--repeats 10] [--warmup 3]

Device time by HIP events (median of the repeats after the warm-up, `x_ms_range` = [min, max]; `x_host_ms`: the wall time of the
same calls, launches included): `add_frame` (the query -> target 1-NN search, the solid split with its 4-byte read, the zero-fill
and the four library calls), `add_frame_shared` (search result and solid rows given, as perform_inference calls it: the zero-fill
and the four library calls plus the Python around them), `library_calls` (occ4d_inst_confusion_f32, occ4d_inst_points_f32 twice
and occ4d_inst_fold alone, through ops), `searches` (ops.knn and ops.split_solid_air alone) and `numpy_tables` (the restatement
of tests/inst_cases.py on the host with the arrays on the host, search results given, median of 3: what a caller would write over
the arrays perform_inference hands back; it never runs the code under test).  Run the command more than once to see the spread
between processes.  The clouds are seeded uniform samples of the scene cuboid, about a fifth of the queries predicted solid."""
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
import inst_cases as ic  # noqa: E402
from frontend_timing import _put, time_device, time_host  # noqa: E402

N_QUERY, N_TARGET, N_IDS, N_GROUPS, RADIUS = 534528, 14336, 12, 3, 0.2


def workload(seed):
    rng = np.random.default_rng(seed)
    q = rng.uniform(-5.0, 5.0, size=(N_QUERY, 4)).astype(np.float32)
    out = rng.uniform(0, 1, size=(N_QUERY, 5)).astype(np.float32)
    out[:, 0] = out[:, 0] ** 3                                    # P(density >= 0.5) = 0.21
    out[:, 4] = rng.integers(-1, N_IDS, size=N_QUERY)             # the merged mark_track channel: a winner id or -1
    target = rng.uniform(0, 1, size=(N_TARGET, 9)).astype(np.float32)
    target[:, :3] = rng.uniform(-5.0, 5.0, size=(N_TARGET, 3))
    target[:, 3] = rng.integers(-1, N_IDS, size=N_TARGET)
    group = rng.integers(0, N_GROUPS, size=N_IDS).astype(np.int32)
    return q, out, target, group


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), queries=N_QUERY, target_points=N_TARGET,
               ids=N_IDS)
    q, out, target, group = workload(1)
    qd, od, td, gd = (torch.from_numpy(x).to(dev) for x in (q, out, target, group))
    kw = dict(density_threshold=0.5, point_occupancy_radius=RADIUS, color_mode='rgb', data_kind='greater', inst_group=gd)
    stats = pk.evaluation.InstanceStats(N_IDS, N_GROUPS, dev)

    def put(name, both):
        _put(res, name + '_ms', both[0])
        res[name + '_host_ms'] = round(both[1][0], 3)
    put('add_frame', time_device(lambda: stats.add_frame(qd, od, td, **kw), a.warmup, a.repeats))

    def searches():
        idx, dist = pk.ops.knn(qd[:, :3], td[:, :3], 1, metric=1, return_dist=True)
        return (idx[:, 0], dist[:, 0]), pk.ops.split_solid_air(qd, od, 0.5)[0]
    nn, solid = searches()
    res['solid_queries'] = solid.shape[0]
    put('searches', time_device(searches, a.warmup, a.repeats))
    put('add_frame_shared', time_device(lambda: stats.add_frame(qd, od, td, nn=nn, solid=solid, **kw), a.warmup, a.repeats))
    frame = torch.zeros_like(stats.frame)

    def calls():
        pk.ops.inst_confusion(od[:, 0], od[:, 4], nn[0], nn[1], td[:, 3], frame, n_ids=N_IDS, density_threshold=0.5, radius=RADIUS)
        pk.ops.inst_points(solid, solid[:, 8], frame, n_ids=N_IDS, side=ic.SIDE_PRED)
        pk.ops.inst_points(td, td[:, 3], frame, n_ids=N_IDS, side=ic.SIDE_GT)
        pk.ops.inst_fold(frame, stats.counts, stats.sums, n_ids=N_IDS, n_groups=N_GROUPS, inst_group=gd)
    put('library_calls', time_device(calls, a.warmup, a.repeats))
    summary = stats.summary()                                      # (no bad rows)
    res['instance_miou'] = [round(float(v), 6) for v in summary['instance_miou']]
    idx_h, dist_h, solid_h = nn[0].cpu().numpy(), nn[1].cpu().numpy(), solid.cpu().numpy()

    def restatement():
        f = np.zeros(ic.frame_len(N_IDS), np.int64)
        ic.restate_confusion(f, out[:, 0], out[:, 4], idx_h, dist_h, target[:, 3], N_IDS, threshold=0.5, radius=RADIUS)
        ic.restate_points(f, solid_h[:, :3], solid_h[:, 8], N_IDS, ic.SIDE_PRED)
        ic.restate_points(f, target[:, :3], target[:, 3], N_IDS, ic.SIDE_GT)
        return f, ic.restate_fold(f, N_IDS, group, N_GROUPS)
    _put(res, 'numpy_tables_ms', time_host(restatement))
    f, _ = restatement()
    stats.add_frame(qd, od, td, nn=nn, solid=solid, **kw)
    res['frame_equals_numpy'] = bool(np.array_equal(stats.frame.cpu().numpy(), f))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
