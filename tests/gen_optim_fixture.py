"""Writes tests/golden/g18_optim_resume.npz on the CPU: the state of torch.optim.AdamW + MultiStepLR after three clipped
steps over two parameter groups, the seeded gradients of steps 4-6 and torch's parameters after each of them.  (The
reference's optimizer IS torch.optim.AdamW, train.py:313-319; nothing else of it is needed.)  Everything seeded comes from
numpy's default_rng, whose streams do not depend on the platform.

    python tests/gen_optim_fixture.py [OUT_DIR]

The shapes and groups are also what tests/test_gpu_optimizer.py uses for its two-group comparison."""
import os
import sys

import numpy as np
import torch

NAME = 'g18_optim_resume'
# 1 element, not a multiple of 4, more than one 4096-element chunk (twice), one parameter that never has a gradient (3),
# one whose gradient is non-contiguous (1), one that gets gradients only from the third step on (6)
SHAPES = [(1,), (3, 5), (70, 61), (7,), (33, 5), (4099,), (2, 2)]
GROUPS = [dict(members=[1, 2, 4], lr=3e-3, weight_decay=1e-2),                                   # "weights"
          dict(members=[0, 3, 5, 6], lr=1e-3, weight_decay=0.0, betas=(0.8, 0.99), eps=1e-6)]    # "biases" + the 1-element tensor
ORDER = [i for g in GROUPS for i in g['members']]          # position in the optimizer's parameter list -> index in SHAPES
NO_GRAD, LATE, TRANSPOSED = 3, 6, 1
MAX_NORM, MILESTONES, GAMMA, STEPS_BEFORE, STEPS_AFTER, SEED = 0.2, [2, 4], 0.4, 3, 3, 1860


def parameters(seed=SEED):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=s).astype(np.float32) for s in SHAPES]


def gradients(rng, step, scale=1.0):
    """One step's gradients (None where the parameter has none); index TRANSPOSED as the transpose of a (5, 3) array."""
    out = []
    for i, s in enumerate(SHAPES):
        g = (rng.normal(size=s[::-1] if i == TRANSPOSED else s) * scale).astype(np.float32)
        out.append(None if i == NO_GRAD or (i == LATE and step < 2) else g)
    return out


def group_dicts(params):
    return [dict({k: v for k, v in g.items() if k != 'members'}, params=[params[i] for i in g['members']]) for g in GROUPS]


def set_grads(params, grads, device=None):
    for i, (p, g) in enumerate(zip(params, grads)):
        if g is None:
            p.grad = None
            continue
        t = torch.from_numpy(g).to(device or p.device).clone()       # (clip_grad_norm_ scales in place: never the caller's array)
        p.grad = t.t() if i == TRANSPOSED else t


def generate():
    params = [torch.nn.Parameter(torch.from_numpy(a)) for a in parameters()]
    opt = torch.optim.AdamW(group_dicts(params), foreach=False)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, MILESTONES, gamma=GAMMA)
    rng = np.random.default_rng(SEED + 1)
    out = {}

    def one(step):
        grads = gradients(rng, step)
        set_grads(params, grads)
        torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], MAX_NORM, foreach=False)
        opt.step()
        sched.step()                       # (one "epoch" per step: the lr drops after steps 2 and 4)
        return grads
    for step in range(STEPS_BEFORE):
        one(step)
    sd = opt.state_dict()
    for i, p in enumerate(params):
        out['param_%d' % i] = p.detach().numpy().copy()
    for pos, st in sd['state'].items():
        i = ORDER[pos]
        out['exp_avg_%d' % i] = st['exp_avg'].numpy().copy()
        out['exp_avg_sq_%d' % i] = st['exp_avg_sq'].numpy().copy()
        out['step_%d' % i] = np.float32(float(st['step']))
    out['lr'] = np.array([g['lr'] for g in sd['param_groups']], dtype=np.float64)
    out['initial_lr'] = np.array([g['initial_lr'] for g in sd['param_groups']], dtype=np.float64)
    out['last_epoch'] = np.int64(sched.state_dict()['last_epoch'])
    for step in range(STEPS_BEFORE, STEPS_BEFORE + STEPS_AFTER):
        grads = one(step)
        for i, g in enumerate(grads):
            if g is not None:
                out['grad_s%d_%d' % (step, i)] = g
        for i, p in enumerate(params):
            out['after_s%d_%d' % (step, i)] = p.detach().numpy().copy()
        out['lr_s%d' % step] = np.array([g['lr'] for g in opt.param_groups], dtype=np.float64)     # (after this step's epoch)
    return out


def torch_state_dict(golden):
    """The fixture as a torch.optim.AdamW state_dict over the optimizer's parameter order (group hyper-parameters from
    GROUPS, the scheduled lr from the file)."""
    ref = torch.optim.AdamW(group_dicts([torch.nn.Parameter(torch.zeros(s)) for s in SHAPES]))
    sd = ref.state_dict()
    for k, g in enumerate(sd['param_groups']):
        g['lr'], g['initial_lr'] = float(golden['lr'][k]), float(golden['initial_lr'][k])
    for pos, i in enumerate(ORDER):
        if 'step_%d' % i in golden:
            sd['state'][pos] = dict(step=torch.tensor(float(golden['step_%d' % i])),
                                    exp_avg=torch.from_numpy(golden['exp_avg_%d' % i]),
                                    exp_avg_sq=torch.from_numpy(golden['exp_avg_sq_%d' % i]))
    return sd


def write(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, NAME + '.npz')
    np.savez(path, **generate())
    return path


if __name__ == '__main__':
    here = os.path.dirname(os.path.abspath(__file__))
    print(write(sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, 'golden')))
