"""Times the ray cast of the decoded field into camera views (ops.raycast_grid: occ4d_raycast_grid_f32) at the published grid --
the GREATER configuration's geometry.grid_counts for 524 288 samples = 534 528 queries -- into 3 views of 240 x 320 pixels, and
what perform_inference(views=FieldViews(...)) adds to a call.  Not a test: it sets no pass mark.

    python profiles/raycast_timing.py [--repeats 20] [--warmup 3] [--no-numpy]

The field is the six-blob synthetic one of profiles/surface_timing.py (seeded), level 0.5, all five columns sampled at the hit.
The cameras stand round the grid and look at its centre.  Timed:
  - the device call with the field as a strided column of the (n, 5) array (ld = 5) and as a contiguous copy handed in: device
    time by HIP events and the host-inclusive wall clock, median of the repeats after the warm-up, `x_ms_range` = [min, max];
  - projection.render_field on the same array (the host's float64 camera inversion and the march range included);
  - the numpy float32 restatement of the same rules (tests/raycast_cases.py: restate; its ray setup is a scalar loop through
    libm's fmaf, its sample loop is vectorised) on the same box's CPU, once, whose result the device's is compared EQUAL with;
  - projection.render_views (the z-buffer of point splats) of the solid rows at radius = 1, the picture there was before;
  - perform_inference on the synthetic scene of profiles/refine_timing.py with and without views=, the two calls ALTERNATING in
    one process.  The synthetic scene's weights are untrained: its images show whatever the untrained density field crosses 0.5
    at (`call_hit_pixels`); a trained model's images are not measured.
Run the command three times to see the spread between processes."""
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
import occlusions4d_amd as pk  # noqa: E402
import raycast_cases as yc  # noqa: E402
from frontend_timing import _put, _stats, time_device, time_host  # noqa: E402
from surface_timing import BATCH, N_POINTS, NUM_SAMPLE, SEED, VIDEO_LEN, blob_field  # noqa: E402

VIEWS, HEIGHT, WIDTH = 3, 240, 320
CHANNELS = (0, 1, 2, 3, 4)


def cameras(counts, mins, spacings):
    lo, hi = yc.hull(counts, mins, spacings)
    centre, reach = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    eyes = [centre + np.array(o) * reach for o in ([-0.8, -0.5, 0.4], [0.7, -0.6, 0.3], [0.05, 0.1, 0.9])]
    K = np.array([[0.8 * WIDTH, 0.0, (WIDTH - 1) / 2.0], [0.0, 0.8 * WIDTH, (HEIGHT - 1) / 2.0], [0.0, 0.0, 1.0]], np.float32)
    return np.stack([yc.look_at(e, centre) for e in eyes[:VIEWS]]).astype(np.float32), K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-numpy', action='store_true', help='skip the numpy restatement (about a minute of host time)')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads())
    pa, ia, inf = pk.configs.model_args('greater', N_POINTS)
    counts, mins, spacings = pk.geometry.grid_frame(NUM_SAMPLE, inf['min_z'], inf['cube_bounds'], 'greater', inf['cube_mode'])
    counts = tuple(counts)
    field = blob_field(counts, np.random.default_rng(SEED))
    n = field.shape[0]
    field_dev = torch.from_numpy(field).to(dev)
    column = field_dev[:, 0].contiguous()
    cam_RT, cam_K = cameras(counts, mins, spacings)
    views = pk.projection.FieldViews(cam_RT, cam_K, HEIGHT, WIDTH, channels=CHANNELS)
    near, step, n_steps = pk.projection.march_range(counts, mins, spacings, views.rt64)
    rt_inv, k_inv = (torch.from_numpy(m).to(dev) for m in (views.rt_inv, views.k_inv))

    def device_call(values):
        return pk.ops.raycast_grid(values, counts, mins, spacings, 0.5, rt_inv, k_inv, HEIGHT, WIDTH, near, step, n_steps,
                                   attrs=field_dev, channels=CHANNELS)

    got = [t.cpu().numpy() for t in device_call(field_dev[:, 0])]
    again = [t.cpu().numpy() for t in device_call(column)]
    res.update(grid=list(counts), queries=n, views=VIEWS, height=HEIGHT, width=WIDTH, channels=len(CHANNELS), near=round(near, 4),
               step=round(step, 5), n_steps=n_steps, hit_pixels=int((got[1] >= 0).sum()),
               strided_equals_contiguous=bool(yc.same_images(again, dict(depth=got[0], cell=got[1], features=got[2]))))
    for name, values in (('strided', field_dev[:, 0]), ('contiguous', column)):
        d, h = time_device(lambda: device_call(values), a.warmup, a.repeats)
        _put(res, name + '_device_ms', d)
        _put(res, name + '_host_inclusive_ms', h)
    d, h = time_device(lambda: pk.projection.render_field(field_dev, counts, mins, spacings, cam_RT, cam_K, HEIGHT, WIDTH, 0.5,
                                                          channels=CHANNELS), a.warmup, a.repeats)
    _put(res, 'render_field_device_ms', d)
    _put(res, 'render_field_host_inclusive_ms', h)

    # the picture there was before: the z-buffer of the solid rows, radius 1
    points = pk.ops.grid_points(counts, mins, spacings, 3, dev)
    solid = torch.cat([points[:, :3], field_dev], dim=1)[field_dev[:, 0] >= 0.5].contiguous()
    d, h = time_device(lambda: pk.projection.render_views(solid, cam_RT, cam_K, HEIGHT, WIDTH, channels=(3, 4, 5, 6, 7), radius=1),
                       a.warmup, a.repeats)
    res['solid_rows'] = int(solid.shape[0])
    _put(res, 'render_views_radius1_device_ms', d)
    _put(res, 'render_views_radius1_host_inclusive_ms', h)

    if not a.no_numpy:
        want = {}

        def numpy_call():
            want.update(yc.restate(field[:, 0], counts, mins, spacings, 0.5, views.k_inv, views.rt_inv, HEIGHT, WIDTH, near, step, n_steps,
                                   field, CHANNELS))
        _put(res, 'numpy_restatement_ms', time_host(numpy_call, repeats=1))
        res['equal_to_restatement'] = bool(yc.same_images(got, want))
        res['numpy_over_device'] = round(res['numpy_restatement_ms'] / res['strided_host_inclusive_ms'], 1)

    # what views= adds to a call
    esd, dsd = pk.configs.synthetic_weights(pa, ia, SEED)
    enc = pk.model.PointCompletionNetV3(**pa).to(dev).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).to(dev).eval()
    dec.load_state_dict(dsd)
    pcl = pk.configs.synthetic_pcl('greater', N_POINTS, VIDEO_LEN, SEED)

    def call(v):
        return pk.inference.perform_inference(
            pcl.clone(), None, None, [enc, dec], dev, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], 3, None,
            sample_implicit=True, num_sample=NUM_SAMPLE, point_sample_mode='grid', batch_size=BATCH,
            predict_segmentation=inf['predict_segmentation'], track_mode='none', semantic_classes=13, density_threshold=0.5,
            data_kind='greater', cube_mode=inf['cube_mode'], compress_air=True, views=v)

    times = {m: ([], []) for m in ('plain', 'views')}
    out = {}
    for i in range(a.warmup + a.repeats):
        for mode in ('plain', 'views'):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out[mode] = call(views if mode == 'views' else None)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= a.warmup:
                times[mode][0].append(e0.elapsed_time(e1))
                times[mode][1].append((t1 - t0) * 1e3)
    for mode in ('plain', 'views'):
        _put(res, '%s_call_device_ms' % mode, _stats(times[mode][0]))
        _put(res, '%s_call_host_inclusive_ms' % mode, _stats(times[mode][1]))
    res['views_add_ms'] = round(res['views_call_host_inclusive_ms'] - res['plain_call_host_inclusive_ms'], 3)
    res['call_hit_pixels'] = int((out['views']['views']['cell'] >= 0).sum())
    res['call_output_unchanged'] = bool(np.array_equal(out['plain']['implicit_output'], out['views']['implicit_output'], equal_nan=True))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
