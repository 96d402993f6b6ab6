"""CPU: tests/golden/g18_optim_resume.npz regenerates from tests/gen_optim_fixture.py (torch.optim.AdamW + MultiStepLR on
the CPU, numpy-seeded), and is what it says it is.  The GPU side of the fixture is tests/test_gpu_optimizer.py."""
import os

import numpy as np
import torch

import gen_optim_fixture as gof
from conftest import GOLDEN, load_golden


def test_fixture_regenerates_bit_for_bit(tmp_path):
    path = gof.write(str(tmp_path))
    with np.load(path) as z:
        fresh = {k: z[k] for k in z.files}
    golden = load_golden(gof.NAME)
    assert sorted(fresh) == sorted(golden)
    for k, v in golden.items():
        assert v.dtype == fresh[k].dtype and np.array_equal(v, fresh[k]), k
    assert os.path.getsize(os.path.join(GOLDEN, gof.NAME + '.npz')) < 512 * 1024


def test_fixture_is_a_loadable_adamw_state_with_the_scheduled_rates():
    g = load_golden(gof.NAME)
    assert int(g['last_epoch']) == gof.STEPS_BEFORE
    # lr after three epochs with milestones [2, 4]: one decay; after epochs 4 (and 5, 6): two
    base = np.array([grp['lr'] for grp in gof.GROUPS])
    assert np.allclose(g['lr'], base * gof.GAMMA, rtol=1e-12) and np.array_equal(g['initial_lr'], base)
    assert np.allclose(g['lr_s3'], base * gof.GAMMA ** 2, rtol=1e-12) and np.allclose(g['lr_s5'], base * gof.GAMMA ** 2, rtol=1e-12)
    assert 'step_%d' % gof.NO_GRAD not in g and float(g['step_%d' % gof.LATE]) == 1.0 and float(g['step_0']) == 3.0
    params = [torch.nn.Parameter(torch.from_numpy(g['param_%d' % i])) for i in range(len(gof.SHAPES))]
    opt = torch.optim.AdamW(gof.group_dicts(params), foreach=False)
    opt.load_state_dict(gof.torch_state_dict(g))
    # replaying step 4 with torch itself from the loaded state gives the recorded parameters
    step = gof.STEPS_BEFORE
    gof.set_grads(params, [g.get('grad_s%d_%d' % (step, i)) for i in range(len(gof.SHAPES))])
    torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], gof.MAX_NORM, foreach=False)
    opt.step()
    for i, p in enumerate(params):
        assert torch.equal(p.detach(), torch.from_numpy(g['after_s%d_%d' % (step, i)])), i
