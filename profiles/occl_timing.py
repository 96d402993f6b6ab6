"""Times the id histogram, occlusion.valo_ids and the clip functions with and without live_occl_mode at the published clip
sizes (GREATER 'unfilt': 3 views x 12 frames x 240 x 320 pixels; CARLA: 4 views x 12 sweeps x 40 000 rows) against the
reference-order numpy loop (tests/occl_cases.py's restatement: one `==` scan per id and frame) on the same box, arrays on the
host.  Not a test: it asserts nothing.

    python profiles/occl_timing.py [--repeats 10] [--warmup 3] [--clip-only]

Device time by HIP events around the call (median of the repeats after the warm-up, `x_ms_range` = [min, max]) and the
host-inclusive wall clock of the same calls; run the command three times to see the spread between processes.  `--clip-only`
measures just the clip functions with their default arguments, so that the same script also runs on a checkout that predates
the feature (the added cost of the mode is the difference to that figure)."""
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
from frontend_timing import HUES, _put, carla_sweeps, greater_frames, time_device, time_host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--clip-only', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads())

    def put(name, fn):
        d, h = time_device(fn, a.warmup, a.repeats)
        _put(res, name + '_device_ms', d)
        _put(res, name + '_host_inclusive_ms', h)

    # ------------------------------------------------------------------------------------------------------------ GREATER
    rgb, flat, depth, cam_RT, cam_K = greater_frames()
    V, T, H, W = depth.shape
    frames = [torch.from_numpy(x).to(dev) for x in (rgb, flat, depth)]
    kw = dict(cam_RT=cam_RT, cam_K=cam_K, hue_clusters=HUES, n_points_rnd=14336, pcl_target_frames=1, n_fps_input=14336,
              n_fps_target=14336)

    def greater(**extra):
        np.random.seed(0)
        torch.manual_seed(0)
        return pk.frontend.greater_clip(frames[0], frames[1], frames[2], **kw, **extra)
    put('greater_clip', greater)
    if not a.clip_only:
        put('greater_clip_unfilt', lambda: greater(live_occl_mode='unfilt', track_mode='random'))
        put('greater_clip_normal', lambda: greater(live_occl_mode='normal', track_mode='random'))
        k_inv = torch.from_numpy(pk.frontend.inverse_4x4(cam_K)).to(dev)
        rt_inv = torch.from_numpy(pk.frontend.inverse_4x4(cam_RT)).to(dev)
        clusters = torch.from_numpy(HUES.astype(np.float32)).to(dev)
        raw = [pk.frontend.rgbd_rows(frames[2][v], frames[0][v], frames[1][v], k_inv[v], rt_inv[v], clusters, (-5.0, 5.0, -5.0, 5.0, -1.0, 5.0))
               for v in range(V)]
        off = torch.arange(T + 1, dtype=torch.int64, device=dev) * (H * W)
        n_ids = len(HUES)
        out = torch.zeros((V * T, n_ids + 2), dtype=torch.int32, device=dev)
        put('greater_histograms', lambda: [pk.ops.id_histogram(raw[v][0], 3, off, n_ids, key=raw[v][2], out=out[v * T:(v + 1) * T])
                                           for v in range(V)])
        all_pcl = [[raw[v][0][t * H * W:(t + 1) * H * W][raw[v][2][t * H * W:(t + 1) * H * W] > 0.5][:, :7].contiguous()
                    for t in range(T)] for v in range(V)]
        res['greater_kept_rows'] = int(sum(f.shape[0] for view in all_pcl for f in view))
        put('greater_valo_ids', lambda: pk.occlusion.valo_ids('unfilt', False, 0, None, 3, T, T, 0, V, 32, all_pcl, None, None, n_ids=n_ids))
        import occl_cases as oc
        host = [[f.cpu().numpy() for f in view] for view in all_pcl]

        def loop(clouds, col, n_bins):
            for view in clouds:
                rows = np.concatenate(view)
                oc.restate(rows, col, np.concatenate([[0], np.cumsum([f.shape[0] for f in view])]), n_bins)
        _put(res, 'greater_numpy_loop_ms', time_host(lambda: loop(host, 3, n_ids)))

    # ------------------------------------------------------------------------------------------------------------ CARLA
    lidar, rt = carla_sweeps()
    rng = np.random.default_rng(2)
    for view in lidar:                                             # integer instance ids (40 actors) and semantic tags
        for s in view:
            s[:, 4] = rng.integers(0, 40, size=s.shape[0])
            s[:, 5] = rng.integers(0, 13, size=s.shape[0])
    sweeps = [[torch.from_numpy(s).to(dev) for s in view] for view in lidar]
    ckw = dict(reference_frame=-1, pcl_target_frames=1, n_fps_input=14336, n_fps_target=14336)

    def carla(**extra):
        np.random.seed(0)
        torch.manual_seed(0)
        return pk.frontend.carla_clip(sweeps, rt, **ckw, **extra)
    put('carla_clip', carla)
    if not a.clip_only:
        put('carla_clip_unfilt', lambda: carla(live_occl_mode='unfilt'))
        put('carla_clip_normal', lambda: carla(live_occl_mode='normal'))
        Vc, Tc = len(sweeps), len(sweeps[0])
        cat = [torch.cat(view) for view in sweeps]
        offs = [torch.from_numpy(np.concatenate([[0], np.cumsum([s.shape[0] for s in view])]).astype(np.int64)).to(dev) for view in sweeps]
        n_ids = pk.occlusion.MAX_IDS
        out = torch.zeros(((Vc + 1) * Tc, n_ids + 2), dtype=torch.int32, device=dev)

        def histograms():
            for v in range(Vc):
                pk.ops.id_histogram(cat[v], 4, offs[v], n_ids, out=out[v * Tc:(v + 1) * Tc])
            pk.ops.id_histogram(cat[0], 4, offs[0], n_ids, pred_col=5, pred_values=(4.0, 10.0), out=out[Vc * Tc:])
        put('carla_histograms', histograms)
        put('carla_valo_ids', lambda: pk.occlusion.valo_ids('unfilt', True, 1, 2, 4, Tc, Tc, 0, Vc, 256, sweeps, None, None))
        _put(res, 'carla_numpy_loop_ms', time_host(lambda: loop(lidar, 4, 40)))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
