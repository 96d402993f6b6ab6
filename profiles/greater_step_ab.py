"""GREATER training step (model_args('greater', 14336), 4 x 17203 queries, density 1 / colour 1 / tracking 1, rgb_nosigmoid):
ms per step (median of synchronised steps), device launches per step, host / device time of the loss phase.
Usage: python profiles/greater_step_ab.py TREE_ROOT [steps]   -- TREE_ROOT: the checkout to import (with its built library); only
TrainStep's public arguments are used, so the same file measures an older commit.  Record: profiles/greater_loss_terms_ab.txt"""
import json, os, sys, time
import numpy as np
import torch
root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import occlusions4d_amd as pk  # noqa: E402
from occlusions4d_amd import training as tr  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

steps = int(sys.argv[2]) if len(sys.argv) > 2 else 12
N_POINTS, FRAMES, QUERIES, SEED = 14336, 4, 17203, 1830
dev = torch.device('cuda:0')
pa, ia, inf = pk.configs.model_args('greater', N_POINTS)
esd, dsd = pk.configs.synthetic_weights(pa, ia, SEED)
enc = pk.model.PointCompletionNetV3(**pa).to(dev).train()
dec = pk.implicit.LocalPclResnetFC(**ia).to(dev).train()
enc.load_state_dict(esd)
dec.load_state_dict(dsd)
pcl = pk.configs.synthetic_pcl('greater', N_POINTS, 12, SEED).to(dev)
rng = np.random.default_rng(SEED + 100)
q = np.concatenate([rng.uniform([-5, -5, -1], [5, 5, 5], size=(FRAMES, QUERIES, 3)),
                    np.broadcast_to(np.arange(FRAMES, dtype=np.float64)[:, None, None], (FRAMES, QUERIES, 1))], -1)
dens = (rng.uniform(size=(FRAMES, QUERIES, 1)) < 0.45).astype(np.float64)
rgb = rng.uniform(size=(FRAMES, QUERIES, 3))
rgb[rng.uniform(size=(FRAMES, QUERIES)) < 0.2] = -1.0
rgb = np.where(dens > 0.5, rgb, 0.0)
target = np.concatenate([dens, rgb, rng.integers(-1, 2, size=(FRAMES, QUERIES, 1)), rng.integers(-1, 13, size=(FRAMES, QUERIES, 1))], -1)
q = torch.from_numpy(q.astype(np.float32)).to(dev)
target = torch.from_numpy(target.astype(np.float32)).to(dev)
lkw = dict(density_lw=1.0, color_lw=1.0, segmentation_lw=0.0, tracking_lw=1.0, color_mode='rgb_nosigmoid', static_shapes=True)
step = tr.TrainStep(enc, dec, lr=1e-3, grad_clip=0.2, loss_kwargs=lkw)
losses = []
for _ in range(3):
    losses.append(step(pcl, q, target, pcl))
torch.cuda.synchronize()
# (a) ms per step: each step timed to its own synchronise; and back-to-back
per = []
for _ in range(steps):
    t0 = time.perf_counter()
    losses.append(step(pcl, q, target, pcl))
    torch.cuda.synchronize()
    per.append((time.perf_counter() - t0) * 1e3)
t0 = time.perf_counter()
for _ in range(steps):
    step(pcl, q, target, pcl)
torch.cuda.synchronize()
b2b = (time.perf_counter() - t0) * 1e3 / steps
# (b) the loss phase alone on the decoder outputs of the step: host issue time and device time, forward + its backward
with torch.no_grad():
    (pa_, fg_, _) = enc(pcl, False)
    out0 = dec(q.reshape(FRAMES * QUERIES, 4), pa_[0], fg_[0], None)[0].reshape(FRAMES, QUERIES, -1)
kw = dict(step.loss_kwargs)
host_f, host_b, devt = [], [], []
for i in range(steps + 3):
    o = out0.clone().requires_grad_(True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    loss = tr.implicit_loss(o, target, **kw)
    t1 = time.perf_counter()
    loss.backward()
    t2 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    if i >= 3:
        host_f.append((t1 - t0) * 1e3); host_b.append((t2 - t1) * 1e3); devt.append(e0.elapsed_time(e1))
# (c) device activities of one step / of the loss phase
def count(fn):
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kern = [n for n in names if not n.lower().startswith(('memcpy', 'memset'))]
    return len(names), len(kern), names
n_all, n_kern, _ = count(lambda: step(pcl, q, target, pcl))
def loss_only():
    o = out0.clone().requires_grad_(True)
    tr.implicit_loss(o, target, **kw).backward()
l_all, l_kern, l_names = count(loss_only)
import collections
print(json.dumps(dict(tree=root, steps=steps, ms_per_step_median=float(np.median(per)), ms_per_step_min=float(np.min(per)),
                      ms_per_step_back_to_back=b2b, loss_host_ms_forward=float(np.median(host_f)), loss_host_ms_backward=float(np.median(host_b)),
                      loss_phase_wall_ms_event=float(np.median(devt)), step_device_activities=n_all, step_kernels=n_kern,
                      loss_phase_device_activities=l_all, loss_phase_kernels=l_kern,
                      loss_phase_kernel_names=dict(collections.Counter(n[:60] for n in l_names).most_common(12)),
                      last_loss=float(losses[-1]), first_loss=float(losses[0]),
                      terms=(step.last_loss_terms.tolist() if getattr(step, 'last_loss_terms', None) is not None else None))), flush=True)
