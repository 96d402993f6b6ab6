"""Times the shortest free-space paths over the clearance (ops.grid_geodesic: occ4d_geodesic_grid_i32) at the published grid -- the
GREATER configuration's geometry.grid_counts for 524 288 samples = 534 528 queries -- and what perform_inference(route=Route())
adds to a call with a clearance.  Not a test: it sets no pass mark.

    python profiles/geodesic_timing.py [--repeats 20] [--warmup 3] [--no-scipy]

Three fields, passable = dist2 >= 1 of ops.grid_distance at level 0.5, connectivity 26, steps (3, 4, 5), the default rounds: the
six-blob synthetic field of profiles/surface_timing.py with the seed in the first free corner, the density column the untrained
synthetic scene of profiles/refine_timing.py decodes to with the seed at the free query nearest the middle, and an all-free grid
with the seed in the corner (0, 0, 0).  Recorded per field:
  - whether the default rounds converged (status[0]) and how many rounds changed a value (status[1]), the reached share and the
    largest cost;
  - ops.grid_geodesic (no host read) without and with `parent`: device time by HIP events and the host-inclusive wall clock, median
    of the repeats after the warm-up, `x_ms_range` = [min, max];
  - the same call with NO seed: round 1 finds nothing to lower and every later launch returns on its flag -- the cost of the
    launches alone;
  - where scipy is importable, the host path on the same box: dist2's copy to the host, the explicit grid graph (26 shifted index
    arrays into a CSR matrix) and scipy.sparse.csgraph.dijkstra from the seed; its costs are compared EQUAL with the device's
    (`equal_to_scipy`), in every run; `scipy_dijkstra_ms` is the search alone;
  - perform_inference on the synthetic scene with clearance=Clearance() alone and with route=Route(seed, goal) as well, the two
    calls ALTERNATING in one process.  The call without `route` is the code path from before this feature, unchanged.
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
from frontend_timing import _put, _stats, time_device  # noqa: E402
from surface_timing import BATCH, N_POINTS, NUM_SAMPLE, SEED, VIDEO_LEN, blob_field  # noqa: E402

try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
except ImportError:
    dijkstra = None

STEPS = (3, 4, 5)
NONE = pk.geodesic.NONE


def shifted(a, d, fill):
    out = np.full_like(a, fill)
    src = tuple(slice(max(x, 0), a.shape[k] + min(x, 0)) for k, x in enumerate(d))
    dst = tuple(slice(max(-x, 0), a.shape[k] + min(-x, 0)) for k, x in enumerate(d))
    out[dst] = a[src]
    return out


def scipy_costs(dist2, counts, seed, timing):
    """The host path: dist2 (device) -> costs (n,) int64 by scipy's Dijkstra on the explicit graph; timing['dijkstra'] = the search."""
    n = counts[0] * counts[1] * counts[2]
    open_ = (dist2.cpu().numpy() >= 1).reshape(counts)
    index = np.arange(n, dtype=np.int32).reshape(counts)
    rows, cols, vals = [], [], []
    for c in range(27):
        d = (c // 9 - 1, (c // 3) % 3 - 1, c % 3 - 1)
        kind = sum(x != 0 for x in d)
        if kind == 0:
            continue
        ok = open_ & shifted(open_, d, False)
        rows.append(index[ok])
        cols.append(shifted(index, d, -1)[ok])
        vals.append(np.full(len(rows[-1]), float(STEPS[kind - 1]), np.float32))
    graph = coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    t0 = time.perf_counter()
    d = dijkstra(graph, directed=True, indices=[seed], min_only=True)
    timing['dijkstra'] = (time.perf_counter() - t0) * 1e3
    return np.where(np.isinf(d), float(NONE), d).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-scipy', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    use_scipy = dijkstra is not None and not a.no_scipy
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads(),
               scipy=__import__('scipy').__version__ if use_scipy else None)
    pa, ia, inf = pk.configs.model_args('greater', N_POINTS)
    counts, mins, spacings = pk.geometry.grid_frame(NUM_SAMPLE, inf['min_z'], inf['cube_bounds'], 'greater', inf['cube_mode'])
    counts = tuple(int(c) for c in counts)
    n = counts[0] * counts[1] * counts[2]
    rounds = pk.ops.geodesic_default_rounds(counts)
    res.update(grid=list(counts), queries=n, rounds=rounds, tile=[pk._lib.GEODESIC_CONSTANTS[k] for k in ('TILE_X', 'TILE_Y', 'TILE_Z')])

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
    no_seed = torch.zeros(0, dtype=torch.int32, device=dev)
    scene_seed = None
    for name, column in fields.items():
        dist2 = pk.ops.grid_distance(column, counts, 0.5)[0]
        free = np.flatnonzero(dist2.cpu().numpy() >= 1)
        seed = int(free[np.argmin(((xyz[free] - xyz[middle]) ** 2).sum(-1))]) if name == 'scene' else int(free[0])
        scene_seed = seed if name == 'scene' else scene_seed
        seeds = torch.tensor([seed], dtype=torch.int32, device=dev)
        cost, status, _ = pk.ops.grid_geodesic(dist2, counts, seeds, steps=STEPS)
        host = cost.cpu().numpy().astype(np.int64)
        status = status.cpu().tolist()
        res.update({name + '_seed': seed, name + '_free_share': round(len(free) / n, 4), name + '_converged': status[0],
                    name + '_changing_rounds': status[1], name + '_reached_share': round(float((host != NONE).mean()), 4),
                    name + '_largest_cost': int(host[host != NONE].max())})
        for parent in (False, True):
            key = '%s_%s' % (name, 'parent' if parent else 'cost')
            d, h = time_device(lambda: pk.ops.grid_geodesic(dist2, counts, seeds, steps=STEPS, parent=parent), a.warmup, a.repeats)
            _put(res, key + '_device_ms', d)
            _put(res, key + '_host_inclusive_ms', h)
        d, h = time_device(lambda: pk.ops.grid_geodesic(dist2, counts, no_seed, steps=STEPS), a.warmup, a.repeats)
        _put(res, name + '_no_seed_device_ms', d)
        _put(res, name + '_no_seed_host_inclusive_ms', h)
        if use_scipy:
            timing = {}
            t0 = time.perf_counter()
            want = scipy_costs(dist2, counts, seed, timing)
            res[name + '_scipy_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
            res[name + '_scipy_dijkstra_ms'] = round(timing['dijkstra'], 1)
            res[name + '_equal_to_scipy'] = bool(np.array_equal(want, host))
            res[name + '_scipy_over_device'] = round(res[name + '_scipy_ms'] / res[name + '_cost_host_inclusive_ms'], 1)

    # what route= adds to a call that has a clearance
    far = int(np.argmax(np.where(pk.ops.grid_distance(scene[:, 0], counts, 0.5)[0].cpu().numpy() >= 1, ((xyz - xyz[scene_seed]) ** 2).sum(-1), -1)))
    route = pk.geodesic.Route([scene_seed], [far])
    times = {m: ([], []) for m in ('clearance', 'route')}
    out = {}
    for i in range(a.warmup + a.repeats):
        for mode in ('clearance', 'route'):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out[mode] = call(route if mode == 'route' else None)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= a.warmup:
                times[mode][0].append(e0.elapsed_time(e1))
                times[mode][1].append((t1 - t0) * 1e3)
    for mode in ('clearance', 'route'):
        _put(res, '%s_call_device_ms' % mode, _stats(times[mode][0]))
        _put(res, '%s_call_host_inclusive_ms' % mode, _stats(times[mode][1]))
    res['route_adds_ms'] = round(res['route_call_host_inclusive_ms'] - res['clearance_call_host_inclusive_ms'], 3)
    res['call_output_unchanged'] = bool(np.array_equal(out['clearance']['implicit_output'], out['route']['implicit_output'], equal_nan=True))
    r = out['route']['route']
    res['call_route_status'] = r['status'].tolist()
    res['call_path_len'] = int(r['path_len'][0])
    res['call_cost_is_the_pieces'] = bool(np.array_equal(r['cost'], pk.ops.grid_geodesic(
        pk.ops.grid_distance(scene[:, 0], counts, 0.5)[0], counts, torch.tensor([scene_seed], dtype=torch.int32, device=dev))[0].cpu().numpy()))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
