"""GPU: training.FusedClipAdamW as a torch.optim.Optimizer (occ4d_adamw_clip_groups_f32, csrc/optim.hip) -- lr schedulers,
parameter groups, torch's state_dict layout both ways, exact resume, the moved-module guard, the entry point against
occ4d_adamw_clip_f32, TrainStep checkpoints, and the CPU-written fixture g18 (tests/gen_optim_fixture.py).

Bounds: those of test_gpu_training.py::test_fused_clip_adamw_matches_torch_over_several_steps -- parameters within
2e-6 * max(1, max|p_torch|), moments within 1e-6, norm within 1e-5 relative -- which were set for FIVE steps from a common
state, so no comparison here runs more than five steps without putting both sides on one state again."""
import argparse
import math
import os

import numpy as np
import pytest
import torch

import gen_optim_fixture as gof
import occlusions4d_amd as pk
from conftest import load_golden
from oracle import path as op

pytestmark = pytest.mark.gpu
Fused = pk.training.FusedClipAdamW


def make_params(seed=gof.SEED):
    mine = [torch.nn.Parameter(torch.from_numpy(a).cuda()) for a in gof.parameters(seed)]
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    return mine, theirs


def give_grads(rng, step, *param_lists, scale=1.0):
    grads = gof.gradients(rng, step, scale)
    for params in param_lists:
        gof.set_grads(params, grads)
    return grads


def torch_step(ref, theirs, max_norm=gof.MAX_NORM):
    norm = torch.nn.utils.clip_grad_norm_([p for p in theirs if p.grad is not None], max_norm)
    ref.step()
    return float(norm)


def assert_params_close(mine, theirs, tag):
    for i, (a, b) in enumerate(zip(mine, theirs)):
        err, bound = float((a.detach() - b.detach()).abs().max()), 2e-6 * max(1.0, float(b.detach().abs().max()))
        assert err <= bound, (tag, i, tuple(a.shape), err, bound)


def assert_moments_close(opt, ref, mine, theirs):
    for a, b in zip(mine, theirs):
        st = ref.state.get(b)
        assert bool(st) == (a in opt.state)                                  # no entry without a gradient, as torch
        if st:
            mst = opt.state[a]
            assert float((mst['exp_avg'] - st['exp_avg']).abs().max()) < 1e-6
            assert float((mst['exp_avg_sq'] - st['exp_avg_sq']).abs().max()) < 1e-6
            assert float(mst['step']) == float(st['step'])


def put_on_one_state(opt, ref, mine, theirs):
    """The fused side takes torch's state (load_state_dict, itself under test) and parameters (in place)."""
    opt.load_state_dict(ref.state_dict())
    with torch.no_grad():
        for a, b in zip(mine, theirs):
            a.copy_(b)


def test_is_a_torch_optimizer_and_follows_multisteplr():
    mine, theirs = make_params()
    opt = Fused(mine, lr=3e-3, weight_decay=1e-2, max_norm=gof.MAX_NORM)
    ref = torch.optim.AdamW(theirs, lr=3e-3, weight_decay=1e-2)
    assert isinstance(opt, torch.optim.Optimizer)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, [2, 4], gamma=0.4)
    sched_ref = torch.optim.lr_scheduler.MultiStepLR(ref, [2, 4], gamma=0.4)
    scaler = torch.amp.GradScaler(enabled=False)
    rng = np.random.default_rng(11)
    steps, seen = 0, []
    for epoch in range(6):
        for _ in range(2):
            give_grads(rng, 2, mine, theirs)
            norm = torch_step(ref, theirs)
            scaler.step(opt)                                                 # = opt.step(): the group default max_norm clips
            steps += 1
            assert abs(float(opt.last_norm) - norm) <= 1e-5 * norm
            assert_params_close(mine, theirs, (epoch, steps))
        sched.step()
        sched_ref.step()
        assert opt.param_groups[0]['lr'] == ref.param_groups[0]['lr']
        seen.append(opt.param_groups[0]['lr'])
        if steps % 4 == 0:
            put_on_one_state(opt, ref, mine, theirs)
    assert np.allclose(seen, [3e-3, 3e-3 * 0.4, 3e-3 * 0.4, 3e-3 * 0.16, 3e-3 * 0.16, 3e-3 * 0.16], rtol=1e-12)
    assert sched.state_dict()['last_epoch'] == 6

    # a changed lr acts on the very next update: one step at lr and one at 0.4 lr from the same state
    deltas, scale = {}, make_params(5)[0]
    for side in ('fused', 'torch'):
        for factor in (1.0, 0.4):
            mine2, theirs2 = make_params(5)
            params = mine2 if side == 'fused' else theirs2
            o = Fused(params, lr=3e-3) if side == 'fused' else torch.optim.AdamW(params, lr=3e-3)
            before = [p.detach().clone() for p in params]
            o.param_groups[0]['lr'] = 3e-3 * factor                          # (what a scheduler does)
            give_grads(np.random.default_rng(12), 2, params)
            if side == 'fused':
                o.step(max_norm=gof.MAX_NORM)
            else:
                torch_step(o, params)
            deltas[side, factor] = [p.detach() - b for p, b in zip(params, before)]
    for i in range(len(gof.SHAPES)):
        d_f = deltas['fused', 1.0][i] - deltas['fused', 0.4][i]
        d_t = deltas['torch', 1.0][i] - deltas['torch', 0.4][i]
        assert float((d_f - d_t).abs().max()) <= 4e-6 * max(1.0, float(scale[i].detach().abs().max()))   # (two differences of bounded errors)
        if i != gof.NO_GRAD:
            assert float(d_f.abs().max()) > 1e-3                             # (AdamW's first step moves by ~lr: 3e-3 vs 1.2e-3)


def test_two_groups_match_torch_adamw():
    mine, theirs = make_params()
    opt = Fused(gof.group_dicts(mine))
    ref = torch.optim.AdamW(gof.group_dicts(theirs))
    assert [g['lr'] for g in opt.param_groups] == [3e-3, 1e-3] and opt.param_groups[1]['betas'] == (0.8, 0.99)
    rng = np.random.default_rng(21)
    for step in range(5):
        give_grads(rng, step, mine, theirs, scale=1e-3 if step == 3 else 1.0)      # (step 3: total norm < max_norm)
        assert not mine[gof.TRANSPOSED].grad.is_contiguous()
        norm = torch_step(ref, theirs)
        opt.step(max_norm=gof.MAX_NORM)
        assert abs(float(opt.last_norm) - norm) <= 1e-5 * norm
        assert abs(float(opt.last_coef) - min(1.0, gof.MAX_NORM / (norm + 1e-6))) < 1e-6
        assert_params_close(mine, theirs, step)
    assert_moments_close(opt, ref, mine, theirs)
    assert mine[gof.NO_GRAD] not in opt.state and float(opt.state[mine[gof.LATE]]['step']) == 3
    assert torch.equal(mine[gof.NO_GRAD], theirs[gof.NO_GRAD])
    with pytest.raises(ValueError, match=r'param_groups\[1\]'):
        Fused([dict(params=[torch.nn.Parameter(torch.zeros(3, device='cuda'))]),
               dict(params=[torch.nn.Parameter(torch.zeros(3, device='cuda'))], betas=(1.0, 0.9))])
    with pytest.raises(ValueError, match='amsgrad'):
        Fused([torch.nn.Parameter(torch.zeros(3, device='cuda'))], amsgrad=True)
    opt.param_groups[1]['lr'] = -1.0
    with pytest.raises(ValueError, match=r'param_groups\[1\]'):
        opt.step()
    assert float(opt.state[mine[0]]['step']) == 5                            # (a refused step counts nothing)


def test_state_dicts_cross_load_with_torch_adamw():
    mine, theirs = make_params()
    opt = Fused(gof.group_dicts(mine))
    ref = torch.optim.AdamW(gof.group_dicts(theirs))
    rng = np.random.default_rng(31)
    for step in range(2):
        give_grads(rng, step, mine, theirs)
        torch_step(ref, theirs)
        opt.step(max_norm=gof.MAX_NORM)
    sd, sd_ref = opt.state_dict(), ref.state_dict()
    assert set(sd['param_groups'][0]) == set(sd_ref['param_groups'][0]) and set(sd['state']) == set(sd_ref['state'])
    for i, st in sd['state'].items():
        assert list(st) == list(sd_ref['state'][i])
        assert st['step'].dtype == sd_ref['state'][i]['step'].dtype and st['step'].shape == ()
    assert [g['params'] for g in sd['param_groups']] == [g['params'] for g in sd_ref['param_groups']]

    # fused -> torch: a fresh torch optimizer over copies of the fused parameters continues in step
    theirs2 = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    ref2 = torch.optim.AdamW(gof.group_dicts(theirs2))
    ref2.load_state_dict(sd)
    for step in range(2, 4):
        give_grads(rng, step, mine, theirs2)
        torch_step(ref2, theirs2)
        opt.step(max_norm=gof.MAX_NORM)
        assert_params_close(mine, theirs2, step)
    assert_moments_close(opt, ref2, mine, theirs2)

    # torch -> fused: a copy into the flat buffers, the state entries still views of them
    opt.load_state_dict(ref2.state_dict())
    lo, hi = opt.exp_avg.data_ptr(), opt.exp_avg.data_ptr() + 4 * opt.exp_avg.numel()
    lo2, hi2 = opt.exp_avg_sq.data_ptr(), opt.exp_avg_sq.data_ptr() + 4 * opt.exp_avg_sq.numel()
    for a, b in zip(mine, theirs2):
        if b in ref2.state:
            st = opt.state[a]
            assert torch.equal(st['exp_avg'], ref2.state[b]['exp_avg']) and torch.equal(st['exp_avg_sq'], ref2.state[b]['exp_avg_sq'])
            assert lo <= st['exp_avg'].data_ptr() < hi and lo2 <= st['exp_avg_sq'].data_ptr() < hi2
            assert float(st['step']) == float(ref2.state[b]['step'])
        else:
            assert a not in opt.state
    with torch.no_grad():
        for a, b in zip(mine, theirs2):
            a.copy_(b)
    for step in range(4, 6):
        give_grads(rng, step, mine, theirs2)
        torch_step(ref2, theirs2)
        opt.step(max_norm=gof.MAX_NORM)
        assert_params_close(mine, theirs2, step)
    # a state from the CPU loads too, and what is refused at construction is refused here
    cpu_sd = torch.optim.AdamW(gof.group_dicts([torch.nn.Parameter(p.detach().cpu()) for p in mine])).state_dict()
    opt.load_state_dict(cpu_sd)
    assert not opt.state and float(opt.exp_avg.abs().max()) == 0.0
    cpu_sd['param_groups'][0]['amsgrad'] = True
    with pytest.raises(ValueError, match='amsgrad'):
        opt.load_state_dict(cpu_sd)


def test_resume_through_a_file_is_exact(tmp_path):
    """2 K steps in one object against K steps, state_dict -> torch.save -> torch.load(map_location='cpu') -> a fresh
    optimizer over fresh copies of the parameters, K more steps: the same kernel on the same inputs with fixed-order
    sums, so parameters and moments are bit-identical."""
    K = 3
    grads = [gof.gradients(np.random.default_rng(41 + s), s) for s in range(2 * K)]
    sched_of = lambda o: torch.optim.lr_scheduler.MultiStepLR(o, [2, 4], gamma=0.4)      # noqa: E731
    one, _ = make_params()
    opt1 = Fused(gof.group_dicts(one), max_norm=gof.MAX_NORM)
    sched1 = sched_of(opt1)
    for s in range(2 * K):
        gof.set_grads(one, grads[s])
        opt1.step()
        sched1.step()
    two, _ = make_params()
    opt2 = Fused(gof.group_dicts(two), max_norm=gof.MAX_NORM)
    sched2 = sched_of(opt2)
    for s in range(K):
        gof.set_grads(two, grads[s])
        opt2.step()
        sched2.step()
    path = str(tmp_path / 'opt.pth')
    torch.save(dict(optimizer=opt2.state_dict(), lr_scheduler=sched2.state_dict(), params=[p.detach().cpu() for p in two]), path)
    loaded = torch.load(path, map_location='cpu')
    three = [torch.nn.Parameter(p.cuda()) for p in loaded['params']]
    opt3 = Fused(gof.group_dicts(three), max_norm=gof.MAX_NORM)
    sched3 = sched_of(opt3)
    opt3.load_state_dict(loaded['optimizer'])
    sched3.load_state_dict(loaded['lr_scheduler'])
    for s in range(K, 2 * K):
        gof.set_grads(three, grads[s])
        opt3.step()
        sched3.step()
    assert [g['lr'] for g in opt3.param_groups] == [g['lr'] for g in opt1.param_groups]
    for a, b in zip(one, three):
        assert torch.equal(a, b)
    assert torch.equal(opt1.exp_avg, opt3.exp_avg) and torch.equal(opt1.exp_avg_sq, opt3.exp_avg_sq)
    assert [opt1.state[p]['step'] if p in opt1.state else 0 for p in one] == \
        [opt3.state[p]['step'] if p in opt3.state else 0 for p in three]
    # the flat layout the class wrote before it kept torch's still loads
    old = dict(step=2 * K, counts=[opt1.state[p]['step'] if p in opt1.state else 0 for p in opt1.params],      # (flat order)
               exp_avg=opt1.exp_avg.clone(), exp_avg_sq=opt1.exp_avg_sq.clone())
    four, _ = make_params()
    opt4 = Fused(gof.group_dicts(four))
    opt4.load_state_dict(old)
    assert torch.equal(opt4.exp_avg, opt1.exp_avg) and (four[gof.NO_GRAD] not in opt4.state) and opt4.state[four[0]]['step'] == 2 * K


def test_moved_module_and_late_groups_are_refused():
    net = torch.nn.Linear(5, 3).cuda()
    opt = Fused(net.parameters(), lr=1e-3)
    net.to('cuda')
    net.float()                                                              # no-ops on an fp32 CUDA module
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    opt.step(max_norm=0.2)
    before = [p.detach().clone() for p in net.parameters()]
    net.half().float()                                                       # new storage
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match=r'parameter 0 .*moved or cast'):
        opt.step(max_norm=0.2)
    torch.cuda.synchronize()
    assert all(torch.equal(p, b.half().float()) for p, b in zip(net.parameters(), before))
    with pytest.raises(RuntimeError, match='fixed at construction'):
        opt.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(2, device='cuda'))]))


def _tables(shapes, chunk):
    numels = [int(np.prod(s)) for s in shapes]
    offsets, total, ct, cs = [], 0, [], []
    for t, n in enumerate(numels):
        offsets.append(total)
        total += (n + 3) // 4 * 4
        for lo in range(0, n, chunk):
            ct.append(t)
            cs.append(lo)
    dev = lambda v, dt: torch.tensor(v, dtype=dt, device='cuda')           # noqa: E731
    return total, numels, dev(offsets, torch.int64), dev(numels, torch.int64), dev(ct, torch.int32), dev(cs, torch.int32)


def test_groups_entry_point_equals_the_scalar_one_bit_for_bit():
    """occ4d_adamw_clip_groups_f32 with the same hyper-parameters in every row and grad_scale = 1 against
    occ4d_adamw_clip_f32 (ctypes, three steps): parameters, moments, norm and coefficient; grad_scale = 0.25 on 4 g
    against grad_scale = 1 on g (powers of two are exact)."""
    lib, P, S = pk._lib.lib(), pk.ops._ptr, pk.ops._stream
    shapes = [(1,), (3, 5), (416, 416), (7,), (832, 33), (10001,), (2, 2)]
    T = len(shapes)
    total, numels, offsets, numel_t, ct, cs = _tables(shapes, int(lib.occ4d_adamw_chunk()))
    C = ct.numel()
    lr, b1, b2, eps, wd, max_norm = 3e-3, 0.9, 0.999, 1e-8, 1e-2, 0.2
    gen = torch.Generator(device='cuda').manual_seed(61)
    start = torch.randn(total, device='cuda', generator=gen)

    def run(which, grad_scale=1.0, grad_mul=1.0):
        g2 = torch.Generator(device='cuda').manual_seed(62)
        p, m, v = start.clone(), torch.zeros_like(start), torch.zeros_like(start)
        ws = torch.zeros(C + 2, device='cuda')
        tails = []
        for step in range(3):
            grads = [torch.randn(n, device='cuda', generator=g2) * (1e-4 if step == 1 else 1.0) * grad_mul for n in numels]
            table = np.zeros(5 * T if which == 'groups' else 2 * T, dtype=np.int64)
            for t, g in enumerate(grads):
                if t == 3:
                    continue                                                 # no gradient: skipped
                table[t] = g.data_ptr()
            k = step + 1
            bias = (np.float32(1.0 - b1 ** k), np.float32(math.sqrt(1.0 - b2 ** k)))
            if which == 'groups':
                rows = table[T:].view(np.float32).reshape(T, 8)
                rows[:, 0:2], rows[:, 2:7] = bias, (lr, b1, b2, eps, wd)
            else:
                table[T:].view(np.float32).reshape(T, 2)[:] = bias
            dtab = torch.from_numpy(table).cuda()
            if which == 'groups':
                rc = lib.occ4d_adamw_clip_groups_f32(P(p), P(m), P(v), P(dtab), P(offsets), P(numel_t), T, P(ct), P(cs), C,
                                                     max_norm, grad_scale, P(ws), S())
            else:
                rc = lib.occ4d_adamw_clip_f32(P(p), P(m), P(v), P(dtab), P(offsets), P(numel_t), T, P(ct), P(cs), C,
                                              lr, b1, b2, eps, wd, max_norm, P(ws), S())
            pk._lib.check(rc)
            torch.cuda.synchronize()
            tails.append(ws[C:].clone())
        return p, m, v, torch.stack(tails)
    old, new = run('scalar'), run('groups')
    for a, b in zip(old, new):
        assert torch.equal(a, b)
    assert not torch.equal(old[0], start) and float(old[3][1, 1]) == 1.0 and float(old[3][0, 1]) < 1.0
    scaled = run('groups', grad_scale=0.25, grad_mul=4.0)
    for a, b in zip(new, scaled):
        assert torch.equal(a, b)


def test_train_step_checkpoint_and_resume_are_exact(tmp_path):
    """Two TrainSteps from the same weights under ops.deterministic(): two steps, checkpoint_dict -> file (which
    inference.load_models reads) -> resume into the second; the third step of both gives the same bits."""
    kind, n = 'carla', 512
    pa, ia, inf = pk.configs.model_args(kind, n)
    pa = dict(pa, fps_random_start=False)
    pcl = pk.configs.synthetic_pcl(kind, n, 4, 41).cuda()
    esd, dsd = pk.configs.synthetic_weights(pa, ia, 42)
    rng = np.random.default_rng(43)
    np.random.seed(1245)
    q = torch.stack([torch.from_numpy(np.ascontiguousarray(
        op.sample_query_points(128, inf['min_z'], inf['cube_bounds'], t, kind, 4, 'random'))) for t in range(2)]).float().cuda()
    target = torch.from_numpy(np.concatenate(
        [rng.integers(0, 2, size=(2, 128, 1)), rng.uniform(size=(2, 128, 3)), np.zeros((2, 128, 1)),
         rng.integers(-1, 13, size=(2, 128, 1))], -1).astype(np.float32)).cuda()

    def build():
        enc = pk.model.PointCompletionNetV3(**pa).cuda().train()
        dec = pk.implicit.LocalPclResnetFC(**ia).cuda().train()
        enc.load_state_dict(esd)
        dec.load_state_dict(dsd)
        groups_of = lambda e, d: [dict(params=[p for net in (e, d) for k, p in net.named_parameters() if not k.endswith('bias')]),   # noqa: E731
                               dict(params=[p for net in (e, d) for k, p in net.named_parameters() if k.endswith('bias')],
                                    weight_decay=0.0, lr=1e-4)]
        step = pk.training.TrainStep(enc, dec, lr=2e-4, grad_clip=0.2, loss_kwargs=dict(density_lw=1.0, segmentation_lw=0.6),
                                     param_groups=groups_of)
        return step, torch.optim.lr_scheduler.MultiStepLR(step.optimizer, [1, 2], gamma=0.5)
    with pk.ops.deterministic():
        a, sched_a = build()
        assert isinstance(a.optimizer, Fused) and len(a.optimizer.param_groups) == 2
        for _ in range(2):
            a(pcl, q, target)
            sched_a.step()
        ckpt = pk.training.checkpoint_dict(a, sched_a, 1, argparse.Namespace(name='resume'), dict(pa),
                                           dict(n_points=n, video_len=4, data_kind=inf['data_kind']), dict(ia))
        assert set(ckpt) == {'optimizer', 'lr_scheduler', 'scaler', 'epoch', 'args', 'pcl_args', 'dset_args',
                             'implicit_args', 'pcl_net', 'implicit_net'} and ckpt['scaler'] == {}
        path = str(tmp_path / 'checkpoint.pth')
        torch.save(ckpt, path)
        (nets, targs, _, pcl_args, implicit_args, epoch) = pk.inference.load_models(path, torch.device('cuda'))
        assert epoch == 1 and targs.name == 'resume' and implicit_args == ia
        for mine, loaded in ((a.pcl_net, nets[0]), (a.implicit_net, nets[1])):
            for (k, v), (k2, v2) in zip(mine.state_dict().items(), loaded.state_dict().items()):
                assert k == k2 and torch.equal(v, v2), k
        b, sched_b = build()
        raw = torch.load(path, map_location='cpu', weights_only=False)
        assert pk.training.resume(b, sched_b, raw) == 2
        assert [g['lr'] for g in b.optimizer.param_groups] == [g['lr'] for g in a.optimizer.param_groups]
        assert np.allclose([g['lr'] for g in b.optimizer.param_groups], [5e-5, 2.5e-5], rtol=1e-12)
        loss_a, loss_b = a(pcl, q, target), b(pcl, q, target)
        torch.cuda.synchronize()
    assert torch.equal(loss_a, loss_b)
    for pa_, pb_ in zip(a.params, b.params):
        assert torch.equal(pa_, pb_)
    # torch's own optimizer and scheduler take the file's entries
    ref = torch.optim.AdamW([dict(params=list(g['params'])) for g in b.optimizer.param_groups], lr=2e-4)
    ref_sched = torch.optim.lr_scheduler.MultiStepLR(ref, [1, 2], gamma=0.5)
    ref.load_state_dict(raw['optimizer'])
    ref_sched.load_state_dict(raw['lr_scheduler'])
    assert ref_sched.last_epoch == 2 and np.allclose([g['lr'] for g in ref.param_groups], [5e-5, 2.5e-5], rtol=1e-12)
    with pytest.raises(ValueError, match='exactly once'):
        pk.training.TrainStep(a.pcl_net, a.implicit_net, param_groups=[dict(params=list(a.pcl_net.parameters()))])


def test_fixture_state_from_torch_on_the_cpu_replays_on_the_gpu():
    """g18: AdamW + MultiStepLR state after 3 steps, written by torch on the CPU; steps 4-6 replayed by the fused step."""
    g = load_golden(gof.NAME)
    params = [torch.nn.Parameter(torch.from_numpy(g['param_%d' % i]).cuda()) for i in range(len(gof.SHAPES))]
    opt = Fused(gof.group_dicts(params), max_norm=gof.MAX_NORM)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, gof.MILESTONES, gamma=gof.GAMMA)
    opt.load_state_dict(gof.torch_state_dict(g))
    sched.load_state_dict(dict(last_epoch=int(g['last_epoch'])))
    assert [grp['lr'] for grp in opt.param_groups] == list(g['lr'])
    for step in range(gof.STEPS_BEFORE, gof.STEPS_BEFORE + gof.STEPS_AFTER):
        gof.set_grads(params, [g.get('grad_s%d_%d' % (step, i)) for i in range(len(gof.SHAPES))])
        opt.step()
        sched.step()
        assert np.allclose([grp['lr'] for grp in opt.param_groups], g['lr_s%d' % step], rtol=1e-12)
        assert_params_close(params, [torch.from_numpy(g['after_s%d_%d' % (step, i)]).cuda() for i in range(len(gof.SHAPES))], step)
    assert float(opt.state[params[gof.LATE]]['step']) == 4 and params[gof.NO_GRAD] not in opt.state
