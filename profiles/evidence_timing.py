"""Times the carve of measured returns into the query grid and the six codes (ops.grid_carve: occ4d_evidence_carve_f32,
ops.grid_evidence: occ4d_evidence_classify_f32) at the published grid -- the GREATER configuration's geometry.grid_counts for
524 288 samples = 96 x 96 x 58 = 534 528 queries --, and what perform_inference(evidence=Evidence()) adds to a call.
Not a test: it sets no pass mark.  It needs a GPU and fails without one.

    python profiles/evidence_timing.py [--repeats 20] [--warmup 3] [--no-numpy] [--no-call] [--other NAME=LIBRARY ...]

--other times the carve of a second library beside the first, the two ALTERNATING call by call, outputs asserted EQUAL, under
`NAME_bits` / `NAME_counts`: a build of csrc/evidence.hip with one of its experiment defines, which is how the variants that
were NOT kept stay reproducible from the tree.  From occlusions-4d_amd/, with <D> = -DOCC4D_EVIDENCE_MATCH=0 (plain adds for the
counts), =1 (a wave match per step of the walk), =3 (per step and of the last cells; the library's own is 2, the last cells alone)
or -DOCC4D_EVIDENCE_GLOBAL_BITS (the passed bits ORed into global memory at every grid):
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -I../include -Icsrc <D> -shared csrc/evidence.hip \
        csrc/error.hip csrc/memops.hip -o libevidence_NAME.so

Fields, each an (n, 5) array whose column 0 is the density: the six-blob synthetic field of profiles/surface_timing.py, the array
the untrained synthetic scene of profiles/refine_timing.py decodes to, and all free.
Returns: `lidar1` / `lidar3`, sweep.cast's own returns of the field for the 64 x 1024 lidar table of profiles/sweep_timing.py from one
pose inside the grid and from three poses (one inside, two outside), in ray order: realistic bundles, neighbouring rays in
neighbouring threads (the all-free field has none: R = 0 times the clear alone); `lidar1_shuffled` / `lidar3_shuffled`, the same rows in a
random order; `clip`, 172 000 random points of the hull over 36 sensors on a ring round the grid, the size of a GREATER clip.
Timed per field and pattern, device time by HIP events and the host-inclusive wall clock, the variants ALTERNATING call by call,
median of the repeats after the warm-up, `x_ms_range` = [min, max]:
  - `bits`: the carve with the passed bits only, as the library places them (staged in LDS at this grid);
  - `counts`: the carve with the per-cell counts as well (one more global integer add per passed cell);
  - `classify`: the six codes and their histogram alone, from the bits;
  - `numpy`: the numpy int64 RESTATEMENT of the header (tests/evidence_cases.py: restate_carve) of lidar1 on this box's CPU, once.  A
    restatement, not a tuned baseline.  The device's output is asserted EQUAL to it;
  - perform_inference on the synthetic scene without and with evidence=Evidence(<the scene's lidar3 returns>), the two calls
    ALTERNATING in one process.  The call without it is the code path from before this feature: its range is the spread to read
    the difference against.
Run the command three times to see the spread between processes.  A trained model's shares are not measured: there is no checkpoint."""
import argparse
import ctypes
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
import evidence_cases as ec  # noqa: E402
import raycast_cases as yc  # noqa: E402
import sweep_cases as sc  # noqa: E402
from frontend_timing import _put, _stats, time_host  # noqa: E402
from surface_timing import BATCH, N_POINTS, NUM_SAMPLE, SEED, VIDEO_LEN, blob_field  # noqa: E402
from sweep_timing import AZIMUTHS, BEAMS, time_alternating  # noqa: E402

CLIP_RETURNS, CLIP_SENSORS = 172000, 36


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-numpy', action='store_true', help='skip the numpy restatement')
    ap.add_argument('--no-call', action='store_true', help='skip the perform_inference comparison')
    ap.add_argument('--other', action='append', default=[], metavar='NAME=LIBRARY', help='a second library whose carve is timed beside')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('profiles/evidence_timing.py needs a GPU: nothing is measured without one')
    dev = torch.device('cuda:0')
    others = {}
    for item in a.other:
        name, _, path = item.partition('=')
        others[name] = pk._lib.bind(ctypes.CDLL(os.path.abspath(path)), missing=lambda symbol: None)

    def through(handle, fn):
        """fn() with `handle` as the package's library for the length of the call."""
        def call():
            keep, pk._lib._lib = pk._lib._lib, handle
            try:
                return fn()
            finally:
                pk._lib._lib = keep
        return call
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads(),
               library=os.path.basename(pk._lib.LIB_PATH), others=sorted(others))
    pa, ia, inf = pk.configs.model_args('greater', N_POINTS)
    counts, mins, spacings = pk.geometry.grid_frame(NUM_SAMPLE, inf['min_z'], inf['cube_bounds'], 'greater', inf['cube_mode'])
    counts = tuple(int(c) for c in counts)
    n = counts[0] * counts[1] * counts[2]
    lo, hi = yc.hull(counts, mins, spacings)
    centre, ext = 0.5 * (lo + hi), hi - lo
    reach = float(np.linalg.norm(ext))
    blob_host = blob_field(counts, np.random.default_rng(SEED))
    density = blob_host[:, 0].reshape(counts)
    inside = None                             # (profiles/sweep_timing.py: the candidate nearest the centre whose grid point is air)
    for off in sorted(((x, y, z) for x in np.linspace(-0.3, 0.3, 7) for y in np.linspace(-0.3, 0.3, 7) for z in (-0.2, 0.0, 0.2)),
                      key=lambda o: o[0] ** 2 + o[1] ** 2 + o[2] ** 2):
        at = centre + np.array(off) * ext
        idx = tuple(int(round((p - m) / s - 0.5)) for p, m, s in zip(at, mins, spacings))
        if density[idx] < 0.05:
            inside = at
            break
    assert inside is not None, 'no free place inside the blob field'
    sensors = [inside, centre + np.array([-0.8, -0.5, 0.4]) * reach, centre + np.array([0.7, -0.6, 0.3]) * reach]
    poses = np.stack([np.concatenate([sc.facing(o, centre + np.array([1.0, 0.0, 0.0]) if i == 0 else centre), o[:, None]], axis=1)
                      for i, o in enumerate(sensors)])
    table = pk.sweep.lidar_directions(BEAMS, AZIMUTHS, 15.0, -25.0)
    res.update(grid=list(counts), queries=n, beams=BEAMS, azimuths=AZIMUTHS)

    esd, dsd = pk.configs.synthetic_weights(pa, ia, SEED)
    enc = pk.model.PointCompletionNetV3(**pa).to(dev).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).to(dev).eval()
    dec.load_state_dict(dsd)
    pcl = pk.configs.synthetic_pcl('greater', N_POINTS, VIDEO_LEN, SEED)

    def call(evidence):
        return pk.inference.perform_inference(
            pcl.clone(), None, None, [enc, dec], dev, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], 3, None,
            sample_implicit=True, num_sample=NUM_SAMPLE, point_sample_mode='grid', batch_size=BATCH,
            predict_segmentation=inf['predict_segmentation'], track_mode='none', semantic_classes=13, density_threshold=0.5,
            data_kind='greater', cube_mode=inf['cube_mode'], compress_air=True, evidence=evidence)

    scene = torch.from_numpy(call(None)['implicit_output'][:, :5].copy()).to(dev)
    fields = dict(blobs=torch.from_numpy(blob_host).to(dev), scene=scene, free=torch.zeros((n, 5), device=dev))
    rng = np.random.default_rng(SEED)
    ring = np.linspace(0.0, 2.0 * np.pi, CLIP_SENSORS, endpoint=False)
    clip_sensors = centre + 0.7 * reach * np.stack([np.cos(ring), np.sin(ring), 0.3 * np.sin(3.0 * ring)], 1)
    clip = ((lo + rng.uniform(size=(CLIP_RETURNS, 3)) * ext).astype(np.float32), rng.integers(0, CLIP_SENSORS, CLIP_RETURNS).astype(np.int32),
            pk.sight.grid_origin(clip_sensors, mins, spacings))
    scene_returns = None

    for fname, field in fields.items():
        patterns = {}
        for pname, V in (('lidar1', 1), ('lidar3', 3)):
            cast = pk.sweep.cast(field, counts, mins, spacings, poses[:V], table, 0.5, shape=(BEAMS, AZIMUTHS))
            hit = (cast['cell'] >= 0).reshape(-1).cpu().numpy()
            points = cast['point'].reshape(-1, 3).cpu().numpy()[hit]
            view = np.repeat(np.arange(V, dtype=np.int32), BEAMS * AZIMUTHS)[hit]
            cells = pk.sight.grid_origin(np.stack(sensors[:V]), mins, spacings)
            patterns[pname] = (points, view, cells)
            order = rng.permutation(len(points))
            patterns[pname + '_shuffled'] = (points[order], view[order], cells)
        if fname == 'scene':
            scene_returns = patterns['lidar3']
        patterns['clip'] = clip
        for pname, (points, view, cells) in patterns.items():
            key = '%s_%s' % (fname, pname)
            ret, sen, org = ec.on(dev, points), ec.on(dev, view), ec.on(dev, cells)
            variants = dict(bits=False, counts=True)
            carve = lambda counts_too: pk.ops.grid_carve(ret, org, counts, mins, spacings, sen, counts_too)
            calls = {name: (lambda v=v: carve(v)) for name, v in variants.items()}
            pk._lib.lib()
            for other, handle in others.items():
                for name, v in variants.items():
                    calls['%s_%s' % (other, name)] = through(handle, lambda v=v: carve(v))
            got = {name: [None if t is None else t.cpu().numpy() for t in fn()] for name, fn in calls.items()}
            first = got['counts']
            for name, arrays in got.items():
                for i in (0, 1, 3):
                    assert np.array_equal(arrays[i], first[i]), (key, name, i)
                assert arrays[2] is None or np.array_equal(arrays[2], first[2]), (key, name)
            res[key + '_returns'] = int(len(points))
            res[key + '_status'] = first[3].tolist()
            res[key + '_marks'] = int(first[2].sum())
            res[key + '_cells_passed'] = int((first[2] > 0).sum())
            res[key + '_most_passes_of_a_cell'] = int(first[2].max())
            passed, hits = carve(variants['bits'])[:2]
            fns = dict(calls)
            fns['classify'] = lambda: pk.ops.grid_evidence(field[:, 0], 0.5, hits, passed=passed)
            for name, (d, h) in time_alternating(fns, a.warmup, a.repeats).items():
                _put(res, '%s_%s_device_ms' % (key, name), d)
                _put(res, '%s_%s_host_inclusive_ms' % (key, name), h)
            code, totals = pk.ops.grid_evidence(field[:, 0], 0.5, hits, passed=passed)
            res[key + '_totals'] = totals.cpu().numpy().tolist()
            if pname == 'lidar1' and not a.no_numpy:
                want = {}

                def numpy_call():
                    want.update(ec.restate_carve(points, view, cells, counts, mins, spacings))
                _put(res, key + '_numpy_restatement_ms', time_host(numpy_call, repeats=1))
                for i, name in enumerate(('passed', 'hits', 'passes', 'status')):
                    assert np.array_equal(first[i], want[name]), (key, name)      # EQUAL, or this script fails
                expect = ec.restate_classify(field[:, 0].cpu().numpy(), 0.5, want['hits'], passed=want['passed'])
                assert np.array_equal(code.cpu().numpy(), expect[0]) and np.array_equal(totals.cpu().numpy(), expect[1])
                res[key + '_equal_to_restatement'] = True

    if not a.no_call:
        points, view, _ = scene_returns
        option = pk.evidence.Evidence(torch.from_numpy(points).to(dev), np.stack(sensors), sensor=torch.from_numpy(view).to(dev))
        times = {m: ([], []) for m in ('plain', 'evidence')}
        out = {}
        for i in range(a.warmup + a.repeats):
            for mode in ('plain', 'evidence'):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                out[mode] = call(option if mode == 'evidence' else None)
                e1.record()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if i >= a.warmup:
                    times[mode][0].append(e0.elapsed_time(e1))
                    times[mode][1].append((t1 - t0) * 1e3)
        for mode in ('plain', 'evidence'):
            _put(res, '%s_call_device_ms' % mode, _stats(times[mode][0]))
            _put(res, '%s_call_host_inclusive_ms' % mode, _stats(times[mode][1]))
        res['evidence_adds_ms'] = round(res['evidence_call_host_inclusive_ms'] - res['plain_call_host_inclusive_ms'], 3)
        res['call_returns'] = int(len(points))
        res['call_totals'] = out['evidence']['evidence']['totals'].tolist()
        res['call_rates'] = {k: float(v) for k, v in pk.evidence.rates(out['evidence']['evidence']['totals']).items()}
        res['call_output_unchanged'] = bool(np.array_equal(out['plain']['implicit_output'], out['evidence']['implicit_output'], equal_nan=True))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
