"""Times perform_inference(refine=GridRefine(...)) against the dense call at the published size: the GREATER configuration,
14 336 input points, the 534 528-query grid, compress_air=True.  Not a test: it asserts nothing.

    python profiles/refine_timing.py [--repeats 10] [--warmup 3]

The synthetic scene's weights are untrained, so the share of blocks its density field makes active says nothing about real
scenes.  What is measured is the cost at a GIVEN share: for block edges 2 and 4 (dilate 1) `low` is set, by bisection over the
representatives' densities of the dense call, to the value that makes about 10 %, 25 % and 50 % of the blocks active.  What is NOT
measured: how much of a trained model's solid set survives at a given `low` (no checkpoint to measure it with).

Per configuration the dense and the refined call ALTERNATE in one process (dense, refined, dense, refined, ...): device time by
HIP events around the call and the host-inclusive wall clock of the same call, median of the repeats after the warm-up,
`x_ms_range` = [min, max]; run the command three times to see the spread between processes.  The dense call is the code path
from before the refinement, unchanged.  Also timed alone: the dense decode (decode_batches on the whole grid, for the
expectation `dense call - (1 - decoded share) * dense decode`) and the refinement's own launches (mark, compaction with its
4-byte count read, expansion) on the arrays of a call."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import occlusions4d_amd as pk  # noqa: E402
from frontend_timing import _put, _stats, time_device  # noqa: E402

N_POINTS, VIDEO_LEN, NUM_SAMPLE, BATCH, SEED = 14336, 12, 524288, 32768, 1830
BLOCKS, SHARES, DILATE = (2, 4), (0.10, 0.25, 0.50), 1


def representative_rows(counts, b):
    axes = [np.minimum(np.arange(-(-n // b)) * b + b // 2, n - 1) for n in counts]
    return ((axes[0][:, None, None] * counts[1] + axes[1][None, :, None]) * counts[2] + axes[2][None, None, :]).reshape(-1)


def active_share(density, low, dilate):
    """Share of active blocks of the (nbx, nby, nbz) density array at `low` (the rule of include/occ4d_refine.h)."""
    hot = ~(density < np.float32(low))
    padded = np.pad(hot, dilate, constant_values=False)
    active = np.zeros_like(hot)
    w = 2 * dilate + 1
    for dx in range(w):
        for dy in range(w):
            for dz in range(w):
                active |= padded[dx:dx + hot.shape[0], dy:dy + hot.shape[1], dz:dz + hot.shape[2]]
    return float(active.mean())


def low_for_share(density, share, dilate):
    """The density value (one of the representatives') whose use as `low` brings the active share closest to `share` from above."""
    values = np.unique(density[np.isfinite(density)])
    lo, hi = 0, len(values) - 1                       # the active share falls as `low` rises
    while lo < hi:
        mid = (lo + hi) // 2
        if active_share(density, values[mid], dilate) > share:
            lo = mid + 1
        else:
            hi = mid
    return float(values[max(lo - 1, 0)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    res = dict(gpu=torch.cuda.get_device_name(0), host_cores=len(os.sched_getaffinity(0)), torch_threads=torch.get_num_threads())
    pa, ia, inf = pk.configs.model_args('greater', N_POINTS)
    esd, dsd = pk.configs.synthetic_weights(pa, ia, SEED)
    enc = pk.model.PointCompletionNetV3(**pa).to(dev).eval()
    enc.load_state_dict(esd)
    dec = pk.implicit.LocalPclResnetFC(**ia).to(dev).eval()
    dec.load_state_dict(dsd)
    pcl = pk.configs.synthetic_pcl('greater', N_POINTS, VIDEO_LEN, SEED)

    def call(refine=None, **kw):
        return pk.inference.perform_inference(
            pcl.clone(), None, None, [enc, dec], dev, 'if', inf['min_z'], inf['cube_bounds'], inf['color_mode'], 3, None,
            sample_implicit=True, num_sample=NUM_SAMPLE, point_sample_mode='grid', batch_size=BATCH,
            predict_segmentation=inf['predict_segmentation'], track_mode='none', semantic_classes=13, density_threshold=0.5,
            data_kind='greater', cube_mode=inf['cube_mode'], compress_air=True, refine=refine, **kw)

    counts = pk.geometry.grid_counts(NUM_SAMPLE, inf['min_z'], inf['cube_bounds'], 'greater', inf['cube_mode'])
    dense = call(return_encoded=True)
    abstract, features = dense.pop('_encoded')
    n, g = dense['implicit_output'].shape
    res.update(queries=n, channels=g, grid=list(counts), dense_solid=int(dense['output_solid'].shape[0]))

    # the dense decode alone (the part the refinement shortens)
    queries = torch.from_numpy(dense['points_query']).to(dev)
    raw = torch.empty((n, g), dtype=torch.float32, device=dev)
    with torch.no_grad():
        d, h = time_device(lambda: pk.inference.decode_batches(dec, queries, 0, n, BATCH, abstract, features, raw), a.warmup, a.repeats)
    _put(res, 'dense_decode_device_ms', d)
    _put(res, 'dense_decode_host_inclusive_ms', h)
    decode_ms = h[0]

    res['configs'] = []
    for b in BLOCKS:
        rep = representative_rows(counts, b)
        nb = tuple(-(-c // b) for c in counts)
        density = dense['implicit_output'][rep, 0].reshape(nb)
        for share in SHARES:
            low = low_for_share(density, share, DILATE)
            refine = pk.inference.GridRefine(b, low, DILATE)
            row = dict(block=b, dilate=DILATE, low=low, target_active_share=share, active_share=round(active_share(density, low, DILATE), 4))
            times = {m: ([], []) for m in ('dense', 'refined')}
            out = {}
            for i in range(a.warmup + a.repeats):
                for mode in ('dense', 'refined'):
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    e0.record()
                    out[mode] = call(refine if mode == 'refined' else None)
                    e1.record()
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    if i >= a.warmup:
                        times[mode][0].append(e0.elapsed_time(e1))
                        times[mode][1].append((t1 - t0) * 1e3)
            for mode in ('dense', 'refined'):
                _put(row, '%s_call_device_ms' % mode, _stats(times[mode][0]))
                _put(row, '%s_call_host_inclusive_ms' % mode, _stats(times[mode][1]))
            st = out['refined']['refine']
            row['decoded_share'] = round(st['n_decoded'] / st['n_queries'], 4)
            row['solid_kept'] = [int(out['refined']['output_solid'].shape[0]), int(out['dense']['output_solid'].shape[0])]
            row['expected_call_ms'] = round(row['dense_call_host_inclusive_ms'] - (1.0 - st['n_decoded'] / st['n_queries']) * decode_ms, 3)
            row['measured_over_expected'] = round(row['refined_call_host_inclusive_ms'] / row['expected_call_ms'], 4)

            # the refinement's own launches on the arrays of such a call: mark, compaction (with the count read), expansion
            rep_out = torch.from_numpy(dense['implicit_output'][rep]).to(dev)
            n_fine = st['n_decoded'] - rep.shape[0]
            fine_out = torch.zeros((n_fine, g), dtype=torch.float32, device=dev)
            expanded = torch.empty((n, g), dtype=torch.float32, device=dev)

            def launches():
                key, _ = pk.ops.refine_mark(rep_out[:, 0], counts, b, DILATE, low, op=0)
                _, count, offsets = pk.ops.compact_rows_with_offsets(queries, key, 0.5)
                pk.ops.refine_expand(key, offsets, rep_out, fine_out[:count], counts, b, out=expanded)
            d, h = time_device(launches, a.warmup, a.repeats)
            _put(row, 'refine_launches_device_ms', d)
            _put(row, 'refine_launches_host_inclusive_ms', h)
            res['configs'].append(row)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
