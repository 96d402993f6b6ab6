"""Times the object layers in camera views (ops.grid_layers: occ4d_layers_march_i32) at the published grid -- the GREATER
configuration's geometry.grid_counts for 524 288 samples = 96 x 96 x 58 = 534 528 queries -- in 3 views of 240 x 320 pixels with 4 and
8 layers, against a ray cast that stops at the first surface, against the existing way to get amodal masks of K objects, and what
perform_inference(layers=ObjectLayers()) adds to a call with components=.  Not a test: it sets no pass mark.

    python profiles/layers_timing.py [--repeats 20] [--warmup 3] [--no-call]

Four label volumes: those components.label (level 0.5, connectivity 6) gives the six-blob synthetic field of
profiles/surface_timing.py, the density column the untrained synthetic scene of profiles/refine_timing.py decodes to (thousands of
components: nearly every sample changes owner) and an all-solid grid, and the watershed segments (h = 1) of the blobs.  The march is
projection.march_range's default: step = half the smallest spacing.  Timed per volume and per max_layers, device time by HIP events
and the host-inclusive wall clock, median of the repeats after the warm-up, `x_ms_range` = [min, max]:
  - layers: ops.grid_layers with every array;  layers_table: the table and the status alone (no per-pixel stores);
  - status = [pixels that dropped an object, pixels with any object], objects, and the objects the busiest 16 x 16 tile meets;
  - (a) raycast: ONE ops.raycast_grid of the same cameras and march over the volume's own density field at level 0.5 (depth and
    cell): what a march that stops costs;
  - (b) blobs' segments only: K calls of ops.raycast_grid on where(labels == k, 1, 0) at level 0.5, the existing way to the K
    amodal masks; its masks follow the trilinear rule, so `kcasts_mask_agreement` is the share of (object, pixel) pairs on which
    cell >= 0 equals projection.amodal_mask of the 8-layer call.  A timing yardstick, not a parity claim;
  - (c) perform_inference on the synthetic scene with components=Components() and with layers=ObjectLayers() beside it, the two
    calls ALTERNATING in one process.  The call without layers is the code path from before this feature, unchanged: its range is
    the spread to read the difference against.
Run the command three times to see the spread between processes.  A trained model's masks are not measured: there is no checkpoint.
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

H, W = 240, 320
LAYER_COUNTS = (4, 8)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    Rm = np.stack([x, y, z])
    return np.concatenate([Rm, (-Rm @ eye)[:, None]], axis=1)


def cameras(counts, mins, spacings):
    """Three cameras round the grid that look at its centre: two obliquely from outside, one from above and aside."""
    lo = np.array([m + 0.5 * s for m, s in zip(mins, spacings)])
    hi = np.array([m + (c - 0.5) * s for m, s, c in zip(mins, spacings, counts)])
    centre, reach = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    K = np.array([[0.9 * W, 0.0, (W - 1) / 2.0], [0.0, 0.9 * W, (H - 1) / 2.0], [0.0, 0.0, 1.0]], np.float32)
    RT = np.stack([look_at(centre + np.array(d) * reach, centre) for d in ((-0.8, -0.5, 0.4), (0.7, -0.6, 0.3), (0.1, 0.2, 0.9))])
    return RT.astype(np.float32), K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-call', action='store_true', help='skip the perform_inference comparison')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads(),
               constants=pk._lib.LAYERS_CONSTANTS, library=os.path.basename(pk._lib.LIB_PATH))
    pa, ia, inf = pk.configs.model_args('greater', N_POINTS)
    counts, mins, spacings = pk.geometry.grid_frame(NUM_SAMPLE, inf['min_z'], inf['cube_bounds'], 'greater', inf['cube_mode'])
    counts = tuple(int(c) for c in counts)
    n = counts[0] * counts[1] * counts[2]
    cam_RT, cam_K = cameras(counts, mins, spacings)
    rt_inv, k_inv, rt64 = pk.projection.invert_cameras(cam_RT, cam_K)
    near, step, n_steps = pk.projection.march_range(counts, mins, spacings, rt64)
    rt_d, k_d = torch.from_numpy(rt_inv).to(dev), torch.from_numpy(k_inv).to(dev)
    res.update(grid=list(counts), queries=n, views=len(cam_RT), image=[H, W], near=near, step=step, n_steps=n_steps)

    esd, dsd = pk.configs.synthetic_weights(pa, ia, SEED)
    enc = pk.model.PointCompletionNetV3(**pa).to(dev).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).to(dev).eval()
    dec.load_state_dict(dsd)
    pcl = pk.configs.synthetic_pcl('greater', N_POINTS, VIDEO_LEN, SEED)

    def call(components, layers):
        return pk.inference.perform_inference(
            pcl.clone(), None, None, [enc, dec], dev, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], 3, None,
            sample_implicit=True, num_sample=NUM_SAMPLE, point_sample_mode='grid', batch_size=BATCH,
            predict_segmentation=inf['predict_segmentation'], track_mode='none', semantic_classes=13, density_threshold=0.5,
            data_kind='greater', cube_mode=inf['cube_mode'], compress_air=True, components=components, layers=layers)

    scene = torch.from_numpy(call(None, None)['implicit_output']).to(dev)
    blobs = torch.from_numpy(blob_field(counts, np.random.default_rng(SEED))).to(dev)
    fields = dict(blobs=blobs, scene=scene, solid=torch.ones((n, 1), device=dev))
    volumes = {}
    for name, field in fields.items():
        labels, tab = pk.components.label(field, counts, 0.5, 6)
        volumes[name] = (labels, int(tab.shape[0]), field)
    seg_labels, seg_tab, _ = pk.watershed.split(blobs, counts, 0.5, 1)
    volumes['blob_segments'] = (seg_labels, int(seg_tab.shape[0]), blobs)

    def march(labels, K, L, want):
        return pk.ops.grid_layers(labels, K, counts, mins, spacings, rt_d, k_d, H, W, near, step, n_steps, L, want=want)

    for name, (labels, K, field) in volumes.items():
        res[name + '_objects'] = K
        column = field[:, 0].contiguous()
        d, h = time_device(lambda: pk.ops.raycast_grid(column, counts, mins, spacings, 0.5, rt_d, k_d, H, W, near, step, n_steps), a.warmup, a.repeats)
        _put(res, name + '_raycast_device_ms', d)
        _put(res, name + '_raycast_host_inclusive_ms', h)
        for L in LAYER_COUNTS:
            for what, want in (('layers', pk.ops.LAYER_ARRAYS), ('layers_table', ('table', 'status'))):
                d, h = time_device(lambda: march(labels, K, L, want), a.warmup, a.repeats)
                _put(res, '%s_%s%d_device_ms' % (name, what, L), d)
                _put(res, '%s_%s%d_host_inclusive_ms' % (name, what, L), h)
            out = march(labels, K, L, pk.ops.LAYER_ARRAYS)
            res['%s_status%d' % (name, L)] = out['status'].cpu().tolist()
            res['%s_layers%d_over_raycast' % (name, L)] = round(res['%s_layers%d_device_ms' % (name, L)] / max(res[name + '_raycast_device_ms'], 1e-6), 2)
        lab = out['label'].cpu().numpy()                    # (the 8-layer call)
        busiest = 0
        for v in range(lab.shape[0]):
            for y in range(0, H, 16):
                for x in range(0, W, 16):
                    tile = lab[v, y:y + 16, x:x + 16]
                    busiest = max(busiest, int(np.unique(tile[tile >= 0]).size))
        res[name + '_busiest_tile_objects'] = busiest

    # (b) the K ray casts of the blobs' segments
    labels, K, _ = volumes['blob_segments']
    masks = [torch.where(labels == k, 1.0, 0.0) for k in range(K)]

    def k_casts():
        return [pk.ops.raycast_grid(m, counts, mins, spacings, 0.5, rt_d, k_d, H, W, near, step, n_steps)[1] for m in masks]
    d, h = time_device(k_casts, a.warmup, a.repeats)
    _put(res, 'kcasts_device_ms', d)
    _put(res, 'kcasts_host_inclusive_ms', h)
    label8 = march(labels, K, 8, ('label',))['label']
    agree = sum(int(((cell >= 0) == pk.projection.amodal_mask(label8, k)).sum()) for k, cell in enumerate(k_casts()))
    res['kcasts_objects'], res['kcasts_mask_agreement'] = K, round(agree / float(K * len(cam_RT) * H * W), 5)
    res['kcasts_over_layers8'] = round(res['kcasts_device_ms'] / max(res['blob_segments_layers8_device_ms'], 1e-6), 2)

    if not a.no_call:
        comp, option = pk.components.Components(), pk.projection.ObjectLayers(cam_RT, cam_K, H, W, max_layers=4)
        times = {m: ([], []) for m in ('components', 'layers')}
        out = {}
        for i in range(a.warmup + a.repeats):
            for mode in ('components', 'layers'):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                out[mode] = call(comp, option if mode == 'layers' else None)
                e1.record()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if i >= a.warmup:
                    times[mode][0].append(e0.elapsed_time(e1))
                    times[mode][1].append((t1 - t0) * 1e3)
        for mode in ('components', 'layers'):
            _put(res, '%s_call_device_ms' % mode, _stats(times[mode][0]))
            _put(res, '%s_call_host_inclusive_ms' % mode, _stats(times[mode][1]))
        res['layers_adds_ms'] = round(res['layers_call_host_inclusive_ms'] - res['components_call_host_inclusive_ms'], 3)
        res['call_objects'] = int(out['layers']['layers']['table'].shape[1])
        res['call_status'] = out['layers']['layers']['status'].tolist()
        res['call_output_unchanged'] = bool(np.array_equal(out['components']['implicit_output'], out['layers']['implicit_output'], equal_nan=True)
                                            and np.array_equal(out['components']['components']['labels'], out['layers']['components']['labels']))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
