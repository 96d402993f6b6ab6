"""GPU: the four-term training loss as one library call (csrc/loss.hip, occ4d_implicit_loss_terms_f32): density BCE, colour
in its four modes with the pre-loss squash folded in, masked segmentation cross entropy and tracking BCE, value, per-term
values and gradient in two launches.  Yardsticks: the G14 fixtures the reference's own loss code produced (total, terms,
gradient) and the eager torch restatement in training.implicit_loss on the same device tensors."""
import colorsys

import numpy as np
import pytest
import torch

import golden_cases as gc
from conftest import load_golden
import occlusions4d_amd as pk

pytestmark = pytest.mark.gpu
tr = pk.training
CASES = gc.LOSS_CASES + gc.LOSS_COLOR_CASES
WEIGHT_KEYS = ('density_lw', 'color_lw', 'segmentation_lw', 'tracking_lw')
ENTRY = 'occ4d_implicit_loss_terms_f32'


def rel_err(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))


def fused(out, tgt, mode, classes=13, d=1.0, c=1.0, s=0.0, t=1.0, want_grad=True):
    return pk.ops.implicit_loss_terms_fused(out, tgt, mode, classes, d, c, s, t, want_grad=want_grad)


def torch_path(monkeypatch, out, tgt, upstream=1.0, **kw):
    """The eager torch form (the reference's) on the same tensors: (loss, terms, gradient)."""
    monkeypatch.setattr(tr, 'FUSED_LOSS', False)
    o = out.clone().requires_grad_(True)
    loss, terms = tr.implicit_loss(o, tgt, static_shapes=False, return_terms=True, **kw)
    (upstream * loss).backward()
    monkeypatch.setattr(tr, 'FUSED_LOSS', True)
    return loss.detach(), terms, o.grad


def training_size_inputs(frames, n, g, seed):
    rng = np.random.default_rng(seed)
    out = rng.normal(size=(frames, n, g)).astype(np.float32) * 3
    dens = (rng.uniform(size=(frames, n, 1)) < 0.45).astype(np.float32)
    rgb = rng.uniform(size=(frames, n, 3)).astype(np.float32)
    rgb[rng.uniform(size=(frames, n)) < 0.2] = -1.0
    mark = rng.integers(-1, 2, size=(frames, n, 1)).astype(np.float32)
    segm = rng.integers(-1, 13, size=(frames, n, 1)).astype(np.float32)
    tgt = np.concatenate([dens, rgb, mark, segm], -1).astype(np.float32)
    return torch.from_numpy(out).cuda(), torch.from_numpy(tgt).cuda()


# ---------------------------------------------------------------- 1. the reference's fixtures through the ops-level call
@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_reference_fixtures_through_the_library_call(case):
    """Total within 2e-6, gradient within 1e-7, each of the four terms within 2e-6 of what the reference's loss code gave
    (the G14 gates of tests/test_gpu_contracts.py)."""
    g = load_golden('g14_loss_' + case['name'])
    raw_np, target_np = gc.loss_inputs(case)
    T_, B, N, G = raw_np.shape
    out = torch.from_numpy(raw_np).cuda().reshape(T_ * B, N, G)
    tgt = torch.from_numpy(target_np).cuda().reshape(T_ * B, N, 6)
    loss, terms, grad = pk.ops.implicit_loss_terms_fused(out, tgt, case['color_mode'], 13, *[case[k] for k in WEIGHT_KEYS])
    assert loss.shape == (1,) and terms.shape == (4,) and grad.shape == out.shape
    print(case['name'], 'total', float(loss), float(g['total'][0]), 'terms', terms.cpu().numpy(), g['terms'],
          'grad', float(np.abs(grad.cpu().numpy().reshape(raw_np.shape) - g['grad']).max()))
    assert abs(float(loss) - float(g['total'][0])) < 2e-6
    assert np.abs(grad.cpu().numpy().reshape(raw_np.shape) - g['grad']).max() < 1e-7
    for k in range(4):
        assert abs(float(terms[k]) - float(g['terms'][k])) < 2e-6, (k, float(terms[k]), float(g['terms'][k]))
    loss2, terms2, none = pk.ops.implicit_loss_terms_fused(out, tgt, case['color_mode'], 13, *[case[k] for k in WEIGHT_KEYS],
                                                           want_grad=False)
    assert none is None and torch.equal(loss2, loss) and torch.equal(terms2, terms)


# ---------------------------------------------------------------- 2. the published GREATER loss takes the kernel
def test_published_greater_loss_takes_the_kernel(monkeypatch):
    """rgb_nosigmoid, density 1 / colour 1 / tracking 1 on a G = 5 decoder (default semantic_classes = 13, no such term):
    neither the torch colour term nor the torch squash is reached; with the fused loss switched off they are."""
    case = gc.LOSS_CASES[0]
    assert case['name'] == 'greater_nosigmoid'
    g = load_golden('g14_loss_' + case['name'])
    raw_np, target_np = gc.loss_inputs(case)

    def boom(*a, **k):
        raise RuntimeError('torch colour path reached')
    monkeypatch.setattr(tr, '_color_term', boom)
    monkeypatch.setattr(tr, 'squash_for_loss', boom)
    raw = torch.from_numpy(raw_np).cuda().requires_grad_(True)
    total, terms = tr.implicit_loss(raw, torch.from_numpy(target_np).cuda(), return_terms=True, **gc.loss_kwargs(case))
    total.backward()
    assert abs(total.item() - float(g['total'][0])) < 2e-6
    assert np.abs(raw.grad.cpu().numpy() - g['grad']).max() < 1e-7
    assert terms.is_cuda and terms.shape == (4,) and not terms.requires_grad
    assert np.abs(terms.cpu().numpy() - g['terms']).max() < 2e-6
    plain = tr.implicit_loss(raw.detach(), torch.from_numpy(target_np).cuda(), **gc.loss_kwargs(case))
    assert torch.is_tensor(plain) and plain.shape == () and plain.item() == total.item()
    monkeypatch.setattr(tr, 'FUSED_LOSS', False)
    with pytest.raises(RuntimeError, match='torch colour path reached'):
        tr.implicit_loss(raw.detach(), torch.from_numpy(target_np).cuda(), **gc.loss_kwargs(case))


def test_squashed_outputs_with_a_colour_term_stay_on_the_torch_path(monkeypatch):
    """The kernel squashes by itself: outputs the caller already squashed must not be squashed again."""
    case = gc.LOSS_CASES[1]                   # 'rgb': sigmoid
    raw_np, target_np = gc.loss_inputs(case)
    raw, tgt = torch.from_numpy(raw_np).cuda(), torch.from_numpy(target_np).cuda()
    want = tr.implicit_loss(raw, tgt, **gc.loss_kwargs(case))
    calls = []
    real = pk.ops.implicit_loss_terms_fused
    monkeypatch.setattr(pk.ops, 'implicit_loss_terms_fused', lambda *a, **k: calls.append(1) or real(*a, **k))
    got = tr.implicit_loss(tr.squash_for_loss(raw, 'rgb'), tgt, squashed=True, **gc.loss_kwargs(case))
    assert not calls
    assert abs(float(got) - float(want)) < 2e-6
    tr.implicit_loss(raw, tgt, squashed=True, density_lw=1.0, tracking_lw=1.0)      # (no colour term: fused)
    assert len(calls) == 1


# ---------------------------------------------------------------- 3. kernel vs the eager torch form at training size
@pytest.mark.parametrize('mode,g,classes', [('rgb', 5, 0), ('rgb_nosigmoid', 5, 0), ('hsv', 16, 0), ('bins', 11, 0),
                                            ('rgb', 18, 13), ('rgb_nosigmoid', 18, 13), ('hsv', 29, 13), ('bins', 24, 13)])
def test_kernel_matches_the_eager_torch_form_at_training_size(monkeypatch, mode, g, classes):
    """4 cells x 17 203 rows, outputs N(0, 3^2), every weight the layout allows non-zero (a decoder without class channels
    has no segmentation term), upstream gradient 2.5: value to 1e-6 relative, gradient to 2e-6 of its largest entry (the
    bounds of test_fused_loss_matches_the_torch_glue); the terms to the bound of the value."""
    out, tgt = training_size_inputs(4, 17203, g, 7 * g + classes)
    kw = dict(density_lw=0.7, color_lw=0.9, segmentation_lw=0.6 if classes else 0.0, tracking_lw=0.3, color_mode=mode,
              semantic_classes=classes or 13)
    lt, tt, gt = torch_path(monkeypatch, out, tgt, upstream=2.5, **kw)
    o = out.clone().requires_grad_(True)
    calls = []
    real = pk.ops.implicit_loss_terms_fused
    monkeypatch.setattr(pk.ops, 'implicit_loss_terms_fused', lambda *a, **k: calls.append(1) or real(*a, **k))
    lf, tf = tr.implicit_loss(o, tgt, return_terms=True, **kw)
    (2.5 * lf).backward()
    assert len(calls) == 1
    print(mode, g, 'loss', float(lf), float(lt), 'grad rel', rel_err(o.grad, gt), 'terms', tf.cpu().numpy(), tt.cpu().numpy())
    assert abs(float(lf) - float(lt)) <= 1e-6 * abs(float(lt)), (float(lf), float(lt))
    assert rel_err(o.grad, gt) <= 2e-6
    for k in range(4):
        assert abs(float(tf[k]) - float(tt[k])) <= 1e-6 * abs(float(tt[k])), (k, float(tf[k]), float(tt[k]))
    if not classes:
        assert float(tf[2]) == 0.0


def test_two_term_entry_point_agrees_with_the_four_term_one():
    """occ4d_implicit_loss_f32 keeps its results: on the CARLA weights both entry points give the same bits."""
    out, tgt = training_size_inputs(4, 17203, 18, 5)
    l2, g2 = pk.ops.implicit_loss_fused(out, tgt, 13, 1.0, 0.6)
    l4, t4, g4 = fused(out, tgt, 'rgb', 13, d=1.0, c=0.0, s=0.6, t=0.0)
    assert torch.equal(l2, l4) and torch.equal(g2, g4)
    assert float(t4[0]) == 0.0 and float(t4[3]) == 0.0
    assert abs(1.0 * float(t4[1]) + 0.6 * float(t4[2]) - float(l4)) <= 1e-6 * float(l4)


# ---------------------------------------------------------------- 4. same class targets on edge inputs
def edge_colours():
    """Colours on the hue-bin edges of 12 and 6 bins, saturation / value at 0.2 / 0.3 / 0.6 and one fp32 step either side,
    grays, two-channel ties for the minimum, colours 0 and 1; `pad`: saturated bright colours (hue-supervised)."""
    e = []
    for k in range(12):
        for s_ in (0.5, 1.0, 0.2, 0.3):
            for v_ in (1.0, 0.6, 0.2, 0.3, 0.5):
                e.append(colorsys.hsv_to_rgb((15 + 30 * k) / 360.0, s_, v_))
                e.append(colorsys.hsv_to_rgb((30 + 60 * (k % 6)) / 360.0, s_, v_))
    e = np.array(e, dtype=np.float32)
    cols = [e, np.nextafter(e, np.float32(-10)), np.nextafter(e, np.float32(10))]
    rng = np.random.default_rng(4)
    gray = rng.uniform(size=(64, 1)).astype(np.float32)
    cols.append(np.repeat(gray, 3, 1))                                             # r = g = b
    ties = rng.uniform(size=(192, 3)).astype(np.float32)
    ties[:64, 1] = ties[:64, 0]
    ties[64:128, 2] = ties[64:128, 1]
    ties[128:, 2] = ties[128:, 0]
    cols.append(ties)
    one = np.float32(1)
    for x in (0.2, 0.3, 0.6):
        for step in (-1, 0, 1):
            v = np.float32(x)
            if step:
                v = np.nextafter(v, np.float32(step * 10))
            cols.append(np.array([[v, v * np.float32(0.5), 0], [v, v, v], [one, one - v, one - v], [v, 0, 0], [0, v, 0],
                                  [one, v, one], [one - v, one, one - v]], dtype=np.float32))
    cols.append(np.array([[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1]],
                         dtype=np.float32))
    rgb = np.clip(np.concatenate(cols), 0.0, 1.0).astype(np.float32)
    pad = np.array([colorsys.hsv_to_rgb(h, 0.9, 0.9) for h in rng.uniform(size=64)], dtype=np.float32)
    return rgb, pad


def trained_class(grad_block):
    """(rows, K) CE gradient block -> per row the index of its single negative entry, -1 for a row without any."""
    neg = grad_block < 0
    count = neg.sum(1)
    assert int(count.max()) <= 1
    return torch.where(count == 1, neg.to(torch.int64).argmax(1), torch.full_like(count, -1))


@pytest.mark.parametrize('mode,g,width', [('hsv', 16, 12), ('bins', 11, 9)])
def test_class_targets_equal_the_torch_paths_on_edge_colours(monkeypatch, mode, g, width):
    """The class every row is trained toward (the negative entry of its CE gradient block) equals the torch path's for
    every row: hue-bin edges are exact half-way cases of round(), thresholds are hit exactly and one step either side."""
    rgb, pad = edge_colours()
    cells = 3
    per = -(-len(rgb) // cells)
    rows = []
    for c in range(cells):
        part = rgb[c * per:(c + 1) * per]
        rows.append(np.concatenate([part, rgb[:per - len(part)], pad]))     # (equal cell sizes; >= 16 hue-supervised rows each)
    colours = np.stack(rows)
    n = colours.shape[1]
    hsv = tr.rgb_to_hsv(torch.from_numpy(colours.reshape(-1, 3))).reshape(cells, n, 3)          # on the CPU
    assert int(((hsv[..., 1] >= 0.2) & (hsv[..., 2] >= 0.2)).sum(1).min()) >= 16
    x = hsv[..., 0] / 360.0 * 12
    assert int((x - torch.floor(x) == 0.5).sum()) >= 12                    # half-way cases are really among the inputs
    tgt = np.concatenate([np.ones((cells, n, 1)), colours, np.zeros((cells, n, 2))], -1).astype(np.float32)
    rng = np.random.default_rng(40)
    out = torch.from_numpy(rng.normal(size=(cells, n, g)).astype(np.float32)).cuda()
    tgt = torch.from_numpy(tgt).cuda()
    _, _, gt = torch_path(monkeypatch, out, tgt, density_lw=0.0, color_lw=1.0, color_mode=mode)
    _, _, gf = fused(out, tgt, mode, d=0.0, c=1.0, t=0.0)
    want = trained_class(gt[..., 1:1 + width].reshape(-1, width))
    got = trained_class(gf[..., 1:1 + width].reshape(-1, width))
    print(mode, 'rows', want.numel(), 'supervised', int((want >= 0).sum()), 'mismatches', int((want != got).sum()),
          'classes seen', sorted(set(want.cpu().tolist())))
    assert want.numel() == cells * n
    assert int((want != got).sum()) == 0
    if mode == 'bins':
        assert int((want < 0).sum()) == 0                                   # every row is supervised
        assert set(want.cpu().tolist()) == set(range(9))
    else:
        hm = ((hsv[..., 1] >= 0.2) & (hsv[..., 2] >= 0.2)).reshape(-1)
        assert torch.equal(want.cpu() >= 0, hm)                             # exactly the hue-supervised rows
        assert set(want.cpu().tolist()) == set(range(12)) | {-1}
    assert rel_err(gf, gt) <= 2e-6


# ---------------------------------------------------------------- 5. branches
def hsv_cell(n_hue, n=40, seed=50):
    """One cell of n solid coloured rows of which exactly n_hue are hue-supervised (saturated, bright); the rest gray."""
    rng = np.random.default_rng(seed)
    colours = np.repeat(rng.uniform(0.3, 0.9, size=(n, 1)), 3, 1)
    colours[:n_hue] = [colorsys.hsv_to_rgb(h, 0.8, 0.7) for h in rng.uniform(size=n_hue)]
    tgt = np.concatenate([np.ones((1, n, 1)), colours[None], np.zeros((1, n, 2))], -1).astype(np.float32)
    out = rng.normal(size=(1, n, 16)).astype(np.float32)
    return torch.from_numpy(out).cuda(), torch.from_numpy(tgt).cuda()


def test_hue_term_needs_sixteen_supervised_rows(monkeypatch):
    out, tgt = hsv_cell(15)
    hsv = tr.rgb_to_hsv(tgt[0, :, 1:4].cpu())
    assert int(((hsv[:, 1] >= 0.2) & (hsv[:, 2] >= 0.2)).sum()) == 15
    lf, tf, gf = fused(out, tgt, 'hsv', d=0.0, c=1.0, t=0.0)
    assert bool((gf[..., 1:13] == 0).all())
    assert bool((gf[..., 13:15] != 0).any())
    lt, tt, gt = torch_path(monkeypatch, out, tgt, density_lw=0.0, color_lw=1.0, color_mode='hsv')
    sat = (out[0, :, 13].clamp(0, 1) - hsv[:, 1].cuda()).abs().mean()
    val = (out[0, :, 14].clamp(0, 1) - hsv[:, 2].cuda()).abs().mean()
    assert abs(float(tt[0]) - float((sat + val) / 3.0)) <= 1e-6 * float(tt[0])      # (the torch path has no hue part either)
    assert abs(float(tf[0]) - float(tt[0])) <= 1e-6 * float(tt[0]), (float(tf[0]), float(tt[0]))
    assert rel_err(gf, gt) <= 2e-6
    out, tgt = hsv_cell(16)
    lf16, tf16, gf16 = fused(out, tgt, 'hsv', d=0.0, c=1.0, t=0.0)
    assert bool((gf16[0, :16, 1:13] != 0).all()) and bool((gf16[0, 16:, 1:13] == 0).all())
    lt16, tt16, gt16 = torch_path(monkeypatch, out, tgt, density_lw=0.0, color_lw=1.0, color_mode='hsv')
    assert float(tf16[0]) > float(tf[0])
    assert abs(float(tf16[0]) - float(tt16[0])) <= 1e-6 * float(tt16[0])
    assert rel_err(gf16, gt16) <= 2e-6


@pytest.mark.parametrize('mode,g', [('rgb', 5), ('rgb_nosigmoid', 5), ('hsv', 16), ('bins', 11)])
def test_cell_without_a_solid_row_gives_a_non_finite_total(mode, g):
    """As the reference's mean over an empty selection (and as the segmentation term does for a cell without labels)."""
    out, tgt = training_size_inputs(3, 300, g, 60)
    tgt[1, :, 0] = 0.0                                   # no solid row in cell 1
    for c, t, finite in ((1.0, 0.0, False), (0.0, 1.0, False), (0.0, 0.0, True)):
        loss, terms, grad = fused(out, tgt, mode, d=1.0, c=c, t=t)
        assert bool(torch.isfinite(loss).all()) is finite, (mode, c, t, float(loss))
        assert bool(torch.isfinite(terms[1]))            # (the density term does not depend on it)


def test_clamp_gradient_pattern_of_rgb_nosigmoid(monkeypatch):
    """torch's clamp passes the gradient on the closed interval [0, 1]; L1's gradient is sign(), sign(0) = 0."""
    f = np.float32
    vals = np.array([0.0, 1.0, np.nextafter(f(0), f(-1)), np.nextafter(f(0), f(1)), np.nextafter(f(1), f(0)),
                     np.nextafter(f(1), f(2)), -0.0, -7.5, 9.0, 0.25, 0.5, 1e-30, -1e-30], dtype=np.float32)
    n = len(vals)
    out = np.zeros((1, n, 5), dtype=np.float32)
    for c in range(3):
        out[0, :, 1 + c] = np.roll(vals, c)
    tgt = np.zeros((1, n, 6), dtype=np.float32)
    tgt[..., 0] = 1.0
    tgt[..., 1:4] = 0.75
    tgt[0, :, 1] = np.where(vals == 0.25, 0.25, 0.75)    # (a row whose clamped output equals its target: sign(0))
    out, tgt = torch.from_numpy(out).cuda(), torch.from_numpy(tgt).cuda()
    _, _, gf = fused(out, tgt, 'rgb_nosigmoid', d=0.0, c=1.0, t=0.0)
    _, _, gt = torch_path(monkeypatch, out, tgt, density_lw=0.0, color_lw=1.0, color_mode='rgb_nosigmoid')
    assert torch.equal(gf[..., 1:4] != 0, gt[..., 1:4] != 0)
    assert torch.equal(torch.sign(gf[..., 1:4]), torch.sign(gt[..., 1:4]))
    col = gf[0, :, 1].cpu().numpy()
    inside = (vals >= 0.0) & (vals <= 1.0) & (vals != 0.25)
    assert np.array_equal(col != 0, inside), (col, inside)
    assert rel_err(gf, gt) <= 2e-6


# ---------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize('mode,g', [('rgb_nosigmoid', 18), ('hsv', 29), ('bins', 24)])
def test_bit_reproducible_from_call_to_call(mode, g):
    out, tgt = training_size_inputs(4, 17203, g, 70)
    a = fused(out, tgt, mode, d=0.7, c=0.9, s=0.6, t=0.3)
    b = fused(out, tgt, mode, d=0.7, c=0.9, s=0.6, t=0.3)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[2]).all())


# ---------------------------------------------------------------- 7. argument validation
@pytest.mark.parametrize('mode,g,weights,what', [
    ('hsv', 5, (1.0, 1.0, 0.0, 0.0), 'colour channels of hsv on G = 5'),
    ('rgb', 4, (1.0, 0.0, 0.0, 1.0), 'tracking on G = 4'),
    ('hsv', 16, (1.0, 1.0, 0.6, 1.0), '13 classes over the hsv channels of G = 16'),
    ('rgb', 5, (1.0, -1.0, 0.0, 0.0), 'negative weight'),
    (7, 5, (1.0, 1.0, 0.0, 0.0), 'unknown mode'),
])
def test_argument_validation_raises_and_launches_nothing(mode, g, weights, what):
    out, tgt = training_size_inputs(2, 64, g, 80)
    with pytest.raises(AssertionError, match=ENTRY):
        pk.ops.implicit_loss_terms_fused(out, tgt, mode, 13, *weights)
    # nothing is launched: the C entry point leaves every output buffer as it found it
    L = pk.ops._lib.lib()
    ws = torch.full((int(L.occ4d_implicit_loss_terms_workspace_floats(2)),), -3.0, device='cuda')
    scal = torch.full((5,), -3.0, device='cuda')
    grad = torch.full_like(out, -3.0)
    P = pk.ops._ptr
    rc = L.occ4d_implicit_loss_terms_f32(P(out), g, P(tgt), 6, 2, 64, g, int(pk.ops.COLOR_MODES.get(mode, mode)), 13, *weights,
                                         P(ws), P(scal[:1]), P(scal[1:]), P(grad), g, pk.ops._stream())
    torch.cuda.synchronize()
    assert rc != 0, what
    assert bool((ws == -3.0).all()) and bool((scal == -3.0).all()) and bool((grad == -3.0).all())


# ---------------------------------------------------------------- 8. step level
def test_train_step_with_the_greater_loss_calls_the_kernel_once_and_keeps_the_terms(monkeypatch):
    """One TrainStep of the published GREATER configuration (no norm, one abstract level, G = 5; density 1 / colour 1 /
    tracking 1, rgb_nosigmoid): the loss phase is ONE call of the fused op; last_loss_terms equals the torch path's terms on
    the same decoder outputs and sum(weight * term) is the loss."""
    kind, n, frames, nq = 'greater', 512, 2, 160
    pa, ia, inf = pk.configs.model_args(kind, n)
    assert ia['d_out'] == 5
    pcl = pk.configs.synthetic_pcl(kind, n, 4, 91).cuda()
    esd, dsd = pk.configs.synthetic_weights(pa, ia, 92)
    enc = pk.model.PointCompletionNetV3(**pa).cuda().train()
    dec = pk.implicit.LocalPclResnetFC(**ia).cuda().train()
    enc.load_state_dict(esd)
    dec.load_state_dict(dsd)
    rng = np.random.default_rng(93)
    q = np.concatenate([rng.uniform(-4.0, 4.0, size=(frames, nq, 3)),
                        np.broadcast_to(np.arange(frames, dtype=np.float64)[:, None, None], (frames, nq, 1))], -1)
    q = torch.from_numpy(q.astype(np.float32)).cuda()
    _, target = training_size_inputs(frames, nq, 5, 94)
    lkw = dict(density_lw=1.0, color_lw=1.0, segmentation_lw=0.0, tracking_lw=1.0, color_mode='rgb_nosigmoid')
    seen = []
    real = pk.ops.implicit_loss_terms_fused

    def recording(out, tgt, *a, **k):
        seen.append((out.detach().clone(), tgt.detach().clone()))
        return real(out, tgt, *a, **k)
    monkeypatch.setattr(pk.ops, 'implicit_loss_terms_fused', recording)
    step = pk.training.TrainStep(enc, dec, lr=2e-4, grad_clip=0.2, loss_kwargs=lkw)
    assert step.last_loss_terms is None
    loss = step(pcl, q, target)
    assert len(seen) == 1
    terms = step.last_loss_terms
    assert terms.is_cuda and terms.shape == (4,) and not terms.requires_grad
    assert np.isfinite(float(loss)) and any(p.grad is not None for p in dec.parameters())
    out, tgt = seen[0]
    assert out.shape == (frames, nq, 5)
    lt, tt, _ = torch_path(monkeypatch, out, tgt, **lkw)
    print('step terms', terms.cpu().numpy(), 'torch', tt.cpu().numpy(), 'loss', float(loss), float(lt))
    for k in range(4):
        assert abs(float(terms[k]) - float(tt[k])) <= 1e-6 * abs(float(tt[k])), (k, float(terms[k]), float(tt[k]))
    assert float(terms[2]) == 0.0
    weighted = 1.0 * float(terms[0]) + 1.0 * float(terms[1]) + 1.0 * float(terms[3])
    assert abs(weighted - float(loss)) <= 1e-6 * abs(float(loss))
    assert abs(float(lt) - float(loss)) <= 1e-6 * abs(float(loss))
