"""One process that runs FusedClipAdamW.step() alone, for a kernel trace of the optimizer step:
    rocprofv3 --kernel-trace --memory-copy-trace --stats -d OUT -- python profiles/optimizer_step_trace.py [steps]
Parameters of the CARLA configuration (two groups: weights / biases), random gradients; 3 warm-up steps, then `steps`.
Expected per step: grad_sumsq_kernel, grad_norm_kernel, adamw_kernel and one host-to-device copy."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import occlusions4d_amd as pk  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
pa, ia, _ = pk.configs.model_args('carla', 28672)
enc = pk.model.PointCompletionNetV3(**pa).cuda()
dec = pk.implicit.LocalPclResnetFC(**ia).cuda()
named = list(enc.named_parameters()) + list(dec.named_parameters())
opt = pk.training.FusedClipAdamW([dict(params=[p for k, p in named if not k.endswith('bias')]),
                                  dict(params=[p for k, p in named if k.endswith('bias')], weight_decay=0.0)], max_norm=0.2)
sched = torch.optim.lr_scheduler.MultiStepLR(opt, [2, 4], gamma=0.4)
grads = [torch.randn_like(p) for _, p in named]
torch.cuda.synchronize()
for i in range(3 + steps):
    for (_, p), g in zip(named, grads):
        p.grad = g
    opt.step()
    sched.step()
torch.cuda.synchronize()
print('optimizer steps: %d (3 warm-up + %d), tensors: %d, elements: %d' % (3 + steps, steps, len(named), opt.flat.numel()))
