"""Times the line of sight through the decoded occupancy (ops.grid_solid_bits / ops.grid_sight: occ4d_sight_bits_f32 /
occ4d_sight_grid_u32) at the published grid -- the GREATER configuration's geometry.grid_counts for 524 288 samples = 96 x 96 x 58 =
534 528 queries -- and what perform_inference(sight=Sight(...)) adds to a call.  Not a test: it sets no pass mark.

    python profiles/sight_timing.py [--repeats 20] [--warmup 3] [--no-host]

Four fields, level 0.5: the six-blob synthetic field of profiles/surface_timing.py, the density column the untrained synthetic scene
of profiles/refine_timing.py decodes to, an all-free grid (every walk runs to the origin or to the grid's hull: the longest walks) and
an all-solid grid (every walk ends at its first step: the shortest).  Timed per field, with 1 and 3 origins, inside and outside the
grid, with and without `blocker` (the variant of the walk kernel that kept the bits in LDS was timed by an earlier version of this
script, lost on every field and is gone: DESIGN 7c rank 19):
  - ops.grid_sight on bits made before (the walk alone) and sight.look (the bits and the walk): device time by HIP events and the
    host-inclusive wall clock, median of the repeats after the warm-up, `x_ms_range` = [min, max]; the share of (origin, query)
    pairs that are hidden;
  - THE EXISTING WAY, in the same run on the same build, on the blob field: projection.FieldViews at 3 x 240 x 320 ray-casts the
    field, the query points are generated again and projection.visibility compares every query with its pixel;
  - the host path, once per field (one origin inside the grid): the copy of the field to the host and the vectorised numpy
    RESTATEMENT of tests/sight_cases.py -- a restatement of the rules written for the tests, not a tuned baseline --, with EQUAL
    bits asserted;
  - perform_inference on the synthetic scene with and without sight=Sight(three origins, blocker=True), the two calls ALTERNATING
    in one process.  The call without `sight` is the code path from before this feature, unchanged.
Run the command three times to see the spread between processes.  A trained model's fields are not measured: there is no checkpoint,
so the share of a trained scene that is hidden is unknown.  The g++ twin is not tuned and is not timed."""
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
from raycast_timing import HEIGHT, WIDTH, cameras  # noqa: E402
from surface_timing import BATCH, N_POINTS, NUM_SAMPLE, SEED, VIDEO_LEN, blob_field  # noqa: E402

def origin_sets(counts):
    nx, ny, nz = counts
    inside = [(nx // 10, 5 * ny // 6, 2 * nz // 3), (nx // 2, ny // 2, nz // 2), (5 * nx // 6, ny // 10, nz // 6)]
    outside = [(-20, ny // 2, nz + 40), (nx // 2, -30, nz + 20), (nx + 44, ny + 24, nz // 2)]
    return {'1_inside': inside[:1], '3_inside': inside, '1_outside': outside[:1], '3_outside': outside}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-host', action='store_true', help='skip the host restatement (tens of seconds per field)')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads())
    pa, ia, inf = pk.configs.model_args('greater', N_POINTS)
    counts, mins, spacings = pk.geometry.grid_frame(NUM_SAMPLE, inf['min_z'], inf['cube_bounds'], 'greater', inf['cube_mode'])
    counts = tuple(int(c) for c in counts)
    n = counts[0] * counts[1] * counts[2]
    res.update(grid=list(counts), queries=n, bits_bytes=4 * ((n + 31) // 32))

    esd, dsd = pk.configs.synthetic_weights(pa, ia, SEED)
    enc = pk.model.PointCompletionNetV3(**pa).to(dev).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).to(dev).eval()
    dec.load_state_dict(dsd)
    pcl = pk.configs.synthetic_pcl('greater', N_POINTS, VIDEO_LEN, SEED)

    def call(sight):
        return pk.inference.perform_inference(
            pcl.clone(), None, None, [enc, dec], dev, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], 3, None,
            sample_implicit=True, num_sample=NUM_SAMPLE, point_sample_mode='grid', batch_size=BATCH,
            predict_segmentation=inf['predict_segmentation'], track_mode='none', semantic_classes=13, density_threshold=0.5,
            data_kind='greater', cube_mode=inf['cube_mode'], compress_air=True, sight=sight)

    scene = torch.from_numpy(call(None)['implicit_output']).to(dev)
    blobs = torch.from_numpy(blob_field(counts, np.random.default_rng(SEED))).to(dev)
    fields = dict(blobs=blobs, scene=scene, free=torch.zeros((n, 1), device=dev), solid=torch.ones((n, 1), device=dev))
    sets = origin_sets(counts)
    for name, field in fields.items():
        bits = pk.ops.grid_solid_bits(field[:, 0], 0.5)
        res[name + '_solid_share'] = round(float((field[:, 0] >= 0.5).float().mean()), 4)
        _put(res, name + '_bits_device_ms', time_device(lambda: pk.ops.grid_solid_bits(field[:, 0], 0.5), a.warmup, a.repeats)[0])
        for oname, origins in sets.items():
            org = np.array(origins, np.int32)
            key = '%s_%s' % (name, oname)
            for bname, blocker in (('', False), ('_blocker', True)):
                d, h = time_device(lambda: pk.ops.grid_sight(bits, counts, org, None, blocker), a.warmup, a.repeats)
                _put(res, key + bname + '_walk_device_ms', d)
                _put(res, key + bname + '_walk_host_inclusive_ms', h)
                d, h = time_device(lambda: pk.sight.look(field, counts, org, 0.5, blocker=blocker), a.warmup, a.repeats)
                _put(res, key + bname + '_look_device_ms', d)
                _put(res, key + bname + '_look_host_inclusive_ms', h)
            res[key + '_hidden_share'] = round(float((pk.ops.grid_sight(bits, counts, org, None, True)[1] >= 0).float().mean()), 4)
        if not a.no_host:
            import sight_cases as sc
            origin = sets['1_inside'][0]
            got = {}

            def host():
                values = field[:, 0].cpu().numpy()
                solid = sc.member_of(values, 0.5)
                got.update(bits=sc.pack(solid), block=sc.blockers_lockstep(solid.reshape(counts), counts, origin))
            _put(res, name + '_host_restatement_ms', time_host(host, repeats=1))
            seen, block = pk.ops.grid_sight(bits, counts, [origin], None, True)
            equal = np.array_equal(got['bits'], bits.cpu().numpy()) and np.array_equal(got['block'].astype(np.int32), block.cpu().numpy()[0]) \
                and np.array_equal((got['block'] < 0).astype(np.int32), seen.cpu().numpy())
            assert equal, name + ': the device and the numpy restatement differ'
            res[name + '_equal_to_restatement'] = bool(equal)

    # the existing way: the ray cast of the field, the query points again, projection.visibility against the depth images
    cam_RT, cam_K = cameras(counts, mins, spacings)
    views = pk.projection.FieldViews(cam_RT, cam_K, HEIGHT, WIDTH)
    margin = float(max(spacings))

    def existing():
        depth = views.render(blobs, counts, mins, spacings, 0.5)[0]
        points = pk.ops.grid_points(counts, mins, spacings, 3, dev)
        return pk.projection.visibility(points[:, :3], depth, cam_RT, cam_K, margin)
    d, h = time_device(existing, a.warmup, a.repeats)
    _put(res, 'blobs_views_plus_visibility_device_ms', d)
    _put(res, 'blobs_views_plus_visibility_host_inclusive_ms', h)
    option = pk.sight.Sight(cameras=(cam_RT, cam_K, HEIGHT, WIDTH))
    grid = pk.products.Grid((counts, mins, spacings), 0.5, False, 13, dev)
    grid.output, grid.points = blobs, pk.ops.grid_points(counts, mins, spacings, 3, dev)[:, :3]
    prepared = option.prepare(grid)
    d, h = time_device(lambda: option.run(grid, prepared, {}), a.warmup, a.repeats)
    _put(res, 'blobs_sight_cameras_device_ms', d)                      # framed by the same three cameras, then the walk
    _put(res, 'blobs_sight_cameras_host_inclusive_ms', h)
    code = existing().cpu().numpy()
    mine = option.run(grid, prepared, {})
    mine = np.stack([pk.sight.codes(mine['seen'], mine['framed'], v).cpu().numpy() for v in range(3)])
    res['blobs_codes_agreeing_with_the_existing_way'] = round(float((code == mine).mean()), 4)       # (pixels and a margin against cells)

    # what sight= adds to a call
    mins64, sp64 = np.asarray(mins, np.float64), np.asarray(spacings, np.float64)
    world = mins64 + (np.array(sets['3_outside'], np.float64) + 0.5) * sp64
    times = {m: ([], []) for m in ('plain', 'sight')}
    out = {}
    for i in range(a.warmup + a.repeats):
        for mode in ('plain', 'sight'):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out[mode] = call(pk.sight.Sight(origins=world, blocker=True) if mode == 'sight' else None)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= a.warmup:
                times[mode][0].append(e0.elapsed_time(e1))
                times[mode][1].append((t1 - t0) * 1e3)
    for mode in ('plain', 'sight'):
        _put(res, '%s_call_device_ms' % mode, _stats(times[mode][0]))
        _put(res, '%s_call_host_inclusive_ms' % mode, _stats(times[mode][1]))
    res['sight_adds_ms'] = round(res['sight_call_host_inclusive_ms'] - res['plain_call_host_inclusive_ms'], 3)
    res['call_hidden_share'] = round(float((out['sight']['sight']['blocker'] >= 0).mean()), 4)
    res['call_output_unchanged'] = bool(np.array_equal(out['plain']['implicit_output'], out['sight']['implicit_output'], equal_nan=True))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
