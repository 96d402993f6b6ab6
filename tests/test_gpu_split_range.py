"""The split-precision kernels (csrc/bf16x6.hpp) at the edges of their range, element by element.

Every output element is held to two bounds (tests/split_scheme.py is the numpy model of both schemes):
  (a) |kernel - model| <= 8 2^-24 sum_k |x~_k w~_k|   only the fp32 accumulation order differs from the model's kept
                                                      products: catches a flushed subnormal piece, a dropped product,
                                                      a wrong scale;
  (b) |kernel - exact| <= contract_bound             the fp64 result of the fp32 operands, within the documented error.
Regimes: tiny activations (fp16 subnormal second pieces), tiny weights, weights up to 255.93, activations up to 65504,
rows of scales 2^-12 .. 2^12 in one launch, signed zeros; bf16x6 from 2^-60 to 2^60 and at gradient magnitudes.
Beyond the fp16 window the failure must be loud: non-finite rows or an error, never finite and wrong."""
import zlib

import numpy as np
import pytest
import torch

import golden_cases as gc
import split_scheme as ss

pytestmark = pytest.mark.gpu

SHAPES = [(1, 208, False, False), (17, 416, True, True), (129, 832, False, True), (1500, 1664, True, False)]


@pytest.fixture(scope='module')
def pk():
    import occlusions4d_amd
    occlusions4d_amd._lib.lib()
    return occlusions4d_amd


def seed(key):
    return zlib.crc32(repr(key).encode())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def loguniform(rng, lo, hi, size, signed=True):
    v = np.exp2(rng.uniform(np.log2(lo), np.log2(hi), size=size))
    return v * (rng.choice([-1.0, 1.0], size=size) if signed else 1.0)


def operands(regime, rng, n, n_out):
    """x (n, 416), w (n_out, 416), row scale of the outputs (n,) for the bias / residual."""
    x = 3.0 * rng.normal(size=(n, 416))
    w = rng.normal(size=(n_out, 416)) / np.sqrt(416)
    rows = np.ones(n)
    if regime == 'tiny_x':              # second piece an fp16 subnormal, the leading one too below 2^-14
        x = loguniform(rng, 2.0 ** -20, 0.25, (n, 416))
        rows = np.full(n, 1e-2)
    elif regime == 'tiny_w':            # weights below 2^-10: absolute 2^-33
        w = loguniform(rng, 2.0 ** -20, 2.0 ** -10, (n_out, 416))
        rows = np.full(n, 1e-3)
    elif regime == 'big_w':             # up to the 255.9375 edge of w * 2^8
        w = loguniform(rng, 1.0, 255.9, (n_out, 416))
        w[0, :3] = [128.0, 255.0, -255.93]
        w[n_out - 1, -3:] = [255.93, -255.0, 128.0]
        x = x / 64.0
        rows = np.full(n, 100.0)
    elif regime == 'big_x':             # activations up to 65504, small weights (outputs stay finite)
        x = loguniform(rng, 1.0, 65504.0, (n, 416))
        x[0, :2] = [65504.0, -65504.0]
        w = w * 2.0 ** -8
        rows = np.full(n, 100.0)
    elif regime == 'mixed_rows':        # 2^-12 .. 2^12 per row in one launch
        rows = 2.0 ** rng.integers(-12, 13, size=n).astype(np.float64)
        x = x * rows[:, None]
    elif regime == 'zeros':
        x[:, ::3] = 0.0
        x[:, 1::3] = -0.0
        w[:, ::5] = -0.0
        if n > 1:
            x[1] = -0.0
    elif regime == 'bf16_huge':         # bf16 x 3: no range restriction (products stay normal fp32 numbers)
        x = loguniform(rng, 2.0 ** 20, 2.0 ** 60, (n, 416))
        w = loguniform(rng, 2.0 ** -60, 2.0 ** -20, (n_out, 416))
    elif regime == 'bf16_tiny':
        x = loguniform(rng, 2.0 ** -60, 2.0 ** -30, (n, 416))
        w = loguniform(rng, 2.0 ** -10, 2.0 ** 10, (n_out, 416))
        rows = np.full(n, 2.0 ** -40)
    elif regime == 'grad':              # training data gradients
        x = loguniform(rng, 1e-12, 1e-4, (n, 416))
        rows = np.full(n, 1e-5)
    return x.astype(np.float32), w.astype(np.float32), rows


F16_REGIMES = ['init', 'tiny_x', 'tiny_w', 'big_w', 'big_x', 'mixed_rows', 'zeros']
BF16_REGIMES = ['init', 'tiny_x', 'big_w', 'big_x', 'mixed_rows', 'zeros', 'bf16_huge', 'bf16_tiny', 'grad']


# fp32 accumulation allowance per unit of sum |x~ w~| for (a), per element: the matrix pipe sums 3 (fp16) / 6 (bf16)
# partial products per k, and the worst of ~1e6 elements reaches a few times the 8 2^-24 of a global-scale bound
ACC_KERNEL = {'f16x3': 16 * 2.0 ** -24, 'bf16x6': 64 * 2.0 ** -24}


def check(tag, scheme, got, model, exact, s, contract, extra=0.0):
    """assertions (a) and (b), per element; prints the worst ratios (error / bound)."""
    acc = ACC_KERNEL[scheme]
    got = got.astype(np.float64)
    assert np.isfinite(got).all(), tag
    ea, eb = np.abs(got - model), np.abs(got - exact)
    ba = acc * s + 2.0 ** -23 * np.abs(model) + extra
    bb = contract + (acc - ss.ACC) * s + extra
    ra, rb = (ea / np.where(ba > 0, ba, 1e-300)).max(), (eb / np.where(bb > 0, bb, 1e-300)).max()
    print('\n[%s] worst |kernel - model| / bound %.3g, |kernel - exact| / contract %.3g' % (tag, ra, rb))
    assert (ea <= ba).all(), '%s: (a) %.3g x the bound' % (tag, ra)
    assert (eb <= bb).all(), '%s: (b) %.3g x the contract' % (tag, rb)


@pytest.mark.parametrize('n,n_out,relu_in,with_res', SHAPES)
@pytest.mark.parametrize('scheme,regime', [('f16x3', r) for r in F16_REGIMES] + [('bf16x6', r) for r in BF16_REGIMES])
def test_rowlin_regimes(pk, scheme, regime, n, n_out, relu_in, with_res):
    rng = np.random.default_rng(seed((regime, n, n_out)) % 2 ** 32)
    x, w, rows = operands(regime, rng, n, n_out)
    b = (rows.min() * rng.normal(size=n_out)).astype(np.float32)
    r = (rows[:, None] * rng.normal(size=(n, n_out))).astype(np.float32) if with_res else None
    got = pk.ops.rowlin_bf16x6(dev(x), dev(w), dev(b), relu_in=relu_in, res=None if r is None else dev(r), scheme=scheme)
    model, exact, s, contract = ss.rowlin(x, w, b, relu_in, r, scheme)
    check('rowlin %s %s %d x %d' % (scheme, regime, n, n_out), scheme, got.cpu().numpy(), model, exact, s, contract)


@pytest.mark.parametrize('n,n_out,after', [(1500, 416, False), (17, 832, True), (129, 208, False)])
@pytest.mark.parametrize('regime', ['grad', 'bf16_tiny', 'mixed_rows', 'zeros'])
def test_rowlin_masked_regimes(pk, regime, n, n_out, after):
    """occ4d_rowlin_bf16x6_masked_f32 at gradient magnitudes: masked entries exactly 0 / the residual, the rest at (a), (b)."""
    rng = np.random.default_rng(seed((regime, n, n_out, after)) % 2 ** 32)
    x, w, rows = operands(regime, rng, n, n_out)
    r = (rows[:, None] * rng.normal(size=(n, n_out))).astype(np.float32)
    m = rng.normal(size=(n, n_out)).astype(np.float32)
    m[::7, ::5] = 0.0
    got = pk.ops.rowlin_bf16x6(dev(x), dev(w), None, res=dev(r), mask=dev(m), res_after_mask=after).cpu().numpy()
    model, exact, s, contract = ss.rowlin(x, w, None, False, None, 'bf16x6')
    keep = m > 0
    r64 = r.astype(np.float64)
    if after:
        model, exact = np.where(keep, model, 0.0) + r64, np.where(keep, exact, 0.0) + r64
    else:
        model, exact = np.where(keep, model + r64, 0.0), np.where(keep, exact + r64, 0.0)
    s, contract = np.where(keep, s, 0.0), np.where(keep, contract + 2.0 ** -23 * np.abs(r64), 2.0 ** -23 * np.abs(r64))
    check('masked %s %d x %d' % (regime, n, n_out), 'bf16x6', got, model, exact, s, contract)
    assert (got[~keep] == (r[~keep] if after else 0.0)).all()


def resblock_ref(x, w0, b0, w1, b1):
    """the two layers of the residual block: model and exact with the chained bounds (layer 2 sees layer 1's error
    through |W1|, and the kernel splits its own fp32 h, not the model's)."""
    m1, e1, s1, c1 = ss.rowlin(x, w0, b0, True, None, 'f16x3')
    h = np.maximum(e1, 0.0)
    m2, e2, s2, c2 = ss.rowlin(np.maximum(m1, 0).astype(np.float32), w1, b1, False, x, 'f16x3')
    exact = x.astype(np.float64) + h @ w1.astype(np.float64).T + b1
    aw1 = np.abs(w1.astype(np.float64)).T
    d1 = ss.ACC * s1 + 2.0 ** -23 * np.abs(m1)                  # kernel h vs model h
    through_a = (d1 + 2 * ss.rep_bound(m1, 'f16x3')) @ aw1 * (1 + 2.0 ** -10)
    through_b = (c1 + 2.0 ** -23 * np.abs(e1)) @ aw1 * (1 + 2.0 ** -10)
    c2x = ss.contract_bound(h.astype(np.float32), w1, 'f16x3') + 2.0 ** -23 * (np.abs(exact) + np.abs(x) + np.abs(b1))
    return m2, exact, s2, through_a, c2x + through_b


@pytest.mark.parametrize('n', [1, 17, 129, 1500])
@pytest.mark.parametrize('regime', ['init', 'tiny_x', 'tiny_w', 'big_w', 'hidden_6e4', 'mixed_rows', 'zeros'])
def test_resblock_f16x3_regimes(pk, regime, n):
    rng = np.random.default_rng(seed((regime, n)) % 2 ** 32)
    x, w0, rows = operands(regime if regime != 'hidden_6e4' else 'init', rng, n, 416)
    _, w1, _ = operands(regime if regime in ('tiny_w', 'big_w') else 'init', rng, 1, 416)
    if regime == 'hidden_6e4':           # one hidden unit per row reaches ~6e4 (< 65504), W1 keeps the output moderate
        x = np.abs(x).astype(np.float32)
        w0[7] = 0.14
        h7 = np.maximum(x, 0).astype(np.float64) @ w0[7].astype(np.float64)
        x = (x * (6.0e4 / h7.max())).astype(np.float32)
        w1 = (w1 * 2.0 ** -6).astype(np.float32)
    b0 = (rows.mean() * rng.normal(size=416)).astype(np.float32)
    b1 = (rows.mean() * rng.normal(size=416)).astype(np.float32)
    if regime == 'mixed_rows':
        b0[:] = 0.0
        b1[:] = 0.0
    got = pk.ops.resblock_f16x3(dev(x), dev(w0), dev(b0), dev(w1), dev(b1)).cpu().numpy()
    model, exact, s, extra_a, contract = resblock_ref(x, w0, b0, w1, b1)
    got = got.astype(np.float64)
    assert np.isfinite(got).all()
    ea, eb = np.abs(got - model), np.abs(got - exact)
    ba = ss.ACC * s + 2.0 ** -23 * (np.abs(model) + np.abs(x)) + extra_a
    ra, rb = (ea / ba).max(), (eb / contract).max()
    print('\n[resblock %s %d] worst (a) %.3g, (b) %.3g' % (regime, n, ra, rb))
    assert ra <= 1 and rb <= 1


def attn_inputs(rng, n, m, k, regime):
    """inputs of the d = 416 split attention kernels (unscaled aq, kt; vtc = vt + c2)."""
    d = 416
    aq, kt = rng.normal(size=(n, 2 * d)), rng.normal(size=(m, 2 * d))
    wp, w2, p2 = 0.1 * rng.normal(size=(2 * d, 32)), 0.03 * rng.normal(size=(d, 2 * d)), 0.1 * rng.normal(size=(d, 32))
    if regime == 'hidden_4090':          # hidden activations up to ~4090 (x 16 = 65440 inside the kernel)
        aq = np.abs(aq)
        aq = aq * (4000.0 / np.abs(aq).max())
        kt = 0.01 * kt
        w2 = w2 / 256.0
    elif regime == 'mixed_rows':
        aq = aq * 2.0 ** rng.integers(-8, 9, size=(n, 1))
    qpos, apos = rng.uniform(-5, 5, size=(n, 3)), rng.uniform(-5, 5, size=(m, 3))
    P1, c1 = rng.normal(size=(32, 3)), rng.normal(size=(32,))
    if regime == 'big_wp':               # merged Wp entries up to 4000 (its window: 65504 / 16), r = 0.5 on their input
        wp[0, 0], wp[5, 0], wp[2 * d - 1, 0] = 4000.0, -3000.0, 255.9
        P1[0], c1[0] = 0.0, 0.5
    vtc = rng.normal(size=(m, d))
    return [np.ascontiguousarray(a, dtype=np.float32) for a in (aq, kt, wp, w2, p2, qpos, apos, P1, c1, vtc)]


def attn_reference(aq, kt, wp, w2, p2, qpos, apos, P1, c1, vtc, idx, dtype):
    """the kernels' formula in torch on the CPU (fp32 or fp64): per pair r, h, logits, pe; agg."""
    t = lambda a: torch.from_numpy(a).to(dtype)          # noqa: E731
    n, k = idx.shape
    j = torch.from_numpy(idx.astype(np.int64)).reshape(-1)
    i = torch.arange(n).repeat_interleave(k)
    r = torch.relu((t(qpos)[i] - t(apos)[j]) @ t(P1).T + t(c1))
    a = t(aq)[i] - t(kt)[j] + r @ t(wp).T
    logits = torch.relu(a) @ t(w2).T
    pe = r @ t(p2).T
    div = torch.tensor(float(np.sqrt(np.float32(416))), dtype=dtype)
    al = torch.softmax((logits / div).reshape(n, k, -1), dim=1)
    agg = (al * (t(vtc)[j].reshape(n, k, -1) + pe.reshape(n, k, -1))).sum(1)
    return [v.numpy() for v in (r, a, logits, pe, agg)]


def run_attn(pk, kernel, ins, idx, n, m, k, logits=False):
    ops = pk.ops
    L, d = ops._lib.lib(), 416
    aq, kt, wp, w2, p2, qpos, apos, P1, c1, vtc = (dev(a) for a in ins)
    idx_d = torch.from_numpy(idx).cuda()
    if kernel == 'bf16x6':
        size, pack, run = (L.occ4d_pt_cross_attn_bf16x6_stream_floats, L.occ4d_pack_attn_bf16x6_stream_f32,
                           L.occ4d_pt_cross_attn_bf16x6_f32)
    elif kernel == 'f16x3':
        size, pack, run = (L.occ4d_pt_cross_attn_f16x3_stream_floats, L.occ4d_pack_attn_f16x3_stream_f32,
                           L.occ4d_pt_cross_attn_f16x3_prescaled_f32)
    else:
        size, pack, run = (L.occ4d_pt_cross_attn_f16w_stream_floats, L.occ4d_pack_attn_f16w_stream_f32,
                           L.occ4d_pt_cross_attn_f16w_f32)
    if kernel != 'bf16x6':
        hs = float(L.occ4d_pt_cross_attn_f16x3_hidden_scale())
        aq, kt = aq * hs, kt * hs
    ws = torch.empty((int(size()),), dtype=torch.float32, device='cuda')
    ops._lib.check(pack(ops._ptr(w2), ops._ptr(wp), ops._ptr(p2), ops._ptr(ws), ops._stream()))
    out = torch.full((n, d), float('nan'), device='cuda')
    div = float(np.sqrt(np.float32(d)))
    common = (ops._ptr(aq), 2 * d, ops._ptr(qpos), 3, ops._ptr(apos), 3, ops._ptr(idx_d), ops._ptr(kt), 2 * d, ops._ptr(vtc), d,
              ops._ptr(P1), ops._ptr(c1), ops._ptr(ws), ops._ptr(out), d)
    if logits:
        lg, a, pe = (torch.full((n * k, w), float('nan'), device='cuda') for w in (d, 2 * d, d))
        c2 = torch.zeros((d,), device='cuda')
        ops._lib.check(L.occ4d_pt_cross_attn_bf16x6_logits_f32(*common, ops._ptr(lg), ops._ptr(a), ops._ptr(pe), ops._ptr(c2),
                                                               n, m, k, d, div, ops._stream()))
        return out.cpu().numpy(), lg.cpu().numpy(), a.cpu().numpy(), pe.cpu().numpy()
    ops._lib.check(run(*common, n, m, k, d, div, ops._stream()))
    return out.cpu().numpy()


def attn_idx(rng, n, m, k):
    return np.stack([rng.choice(m, size=k, replace=False) for _ in range(n)]).astype(np.int32)


def agg_bound(scheme, ins, idx, ref64, ref32):
    """per row: max(2 |fp32 - fp64|, contract) -- the contract carries the logits' bound through the softmax (a logit
    error e moves a weight by <= 2 e / divisor of it) and adds pe's bound."""
    aq, kt, wp, w2, p2, qpos, apos, P1, c1, vtc = ins
    r, a, lg, pe, agg = ref64
    n, k = idx.shape
    ws = ss.F16_WSCALE if scheme != 'bf16x6' else None
    ca = ss.contract_bound(r.astype(np.float32), wp, scheme, ss.F16_HSCALE if ws else None) + 2.0 ** -22 * np.abs(a)
    h = np.maximum(a, 0)
    clg = ss.contract_bound(h.astype(np.float32), w2, scheme) + ca @ np.abs(w2.astype(np.float64)).T
    cpe = ss.contract_bound(r.astype(np.float32), p2, scheme)
    div = np.sqrt(416.0)
    v = np.abs(vtc[idx.reshape(-1)].astype(np.float64) + pe).reshape(n, k, -1).max(1)
    contract = 2 * clg.reshape(n, k, -1).max(1) / div * v + cpe.reshape(n, k, -1).max(1) + 2.0 ** -21 * np.abs(agg)
    return np.maximum(2 * np.abs(ref32[4] - agg).max(1, keepdims=True), contract.max(1, keepdims=True))


@pytest.mark.parametrize('n,m,k', [(17, 76, 14), (129, 531, 14), (9, 30, 5)])
@pytest.mark.parametrize('regime', ['init', 'hidden_4090', 'mixed_rows', 'big_wp'])
@pytest.mark.parametrize('kernel', ['f16x3', 'f16w', 'bf16x6'])
def test_attention_regimes(pk, kernel, regime, n, m, k):
    rng = np.random.default_rng(seed((kernel, regime, n)) % 2 ** 32)
    ins = attn_inputs(rng, n, m, k, regime)
    idx = attn_idx(rng, n, m, k)
    ref64 = attn_reference(*ins, idx, torch.float64)
    ref32 = attn_reference(*ins, idx, torch.float32)
    scheme = 'bf16x6' if kernel == 'bf16x6' else 'f16x3'
    bound = agg_bound(scheme, ins, idx, ref64, ref32)
    got = run_attn(pk, kernel, ins, idx, n, m, k)
    assert np.isfinite(got).all()
    err = np.abs(got - ref64[4]).max(1, keepdims=True)
    print('\n[attn %s %s n %d] worst row error / bound %.3g' % (kernel, regime, n, (err / bound).max()))
    assert (err <= bound).all()


@pytest.mark.parametrize('regime', ['init', 'mixed_rows', 'big_wp'])
def test_attention_bf16x6_pair_tensors(pk, regime):
    """occ4d_pt_cross_attn_bf16x6_logits_f32: a, logits and pe per element at (a) and (b), logits against the model on
    the kernel's own a (which it emits)."""
    n, m, k = 129, 531, 14
    rng = np.random.default_rng(seed(('pairs', regime)) % 2 ** 32)
    ins = attn_inputs(rng, n, m, k, regime)
    aq, kt, wp, w2, p2, qpos, apos, P1, c1, vtc = ins
    idx = attn_idx(rng, n, m, k)
    r, a64, lg64, pe64, _ = attn_reference(*ins, idx, torch.float64)
    out, lg, a, pe = run_attn(pk, 'bf16x6', ins, idx, n, m, k, logits=True)
    # r itself is fp32 VALU work of the kernel: its error enters every GEMM through |W|
    r32 = attn_reference(*ins, idx, torch.float32)[0]
    dr = np.abs(r32.astype(np.float64) - r) * 4 + 2.0 ** -22 * np.abs(r)
    j = idx.reshape(-1).astype(np.int64)
    i = np.repeat(np.arange(n), k)
    init = (aq[i] - kt[j]).astype(np.float64)
    mo, ex, s, cb = ss.rowlin(r32, wp, None, False, None, 'bf16x6')
    # the kernel's accumulator starts at aq - kt (fp32) and rounds at that magnitude after each of its 6 MFMAs
    ainit = 2.0 ** -21 * (np.abs(aq[i]) + np.abs(kt[j]))
    check('pair a %s' % regime, 'bf16x6', a, mo + init, a64, s, cb + 2.0 ** -23 * np.abs(a64),
          extra=dr @ np.abs(wp.astype(np.float64)).T + ainit)
    mo, ex, s, cb = ss.rowlin(np.maximum(a, 0), w2, None, False, None, 'bf16x6')
    da = np.abs(a.astype(np.float64) - a64)
    check('pair logits %s' % regime, 'bf16x6', lg, mo, lg64, s, cb + da @ np.abs(w2.astype(np.float64)).T)
    mo, ex, s, cb = ss.rowlin(r32, p2, None, False, None, 'bf16x6')
    check('pair pe %s' % regime, 'bf16x6', pe, mo, pe64, s, cb, extra=dr @ np.abs(p2.astype(np.float64)).T)


@pytest.mark.parametrize('regime', ['init', 'grad'])
def test_pt_pair_mlp_bf16x6_regimes(pk, regime):
    """the training pair-tensor kernel (occ4d_pt_pair_mlp_bf16x6_f32) at gradient magnitudes: a, logits, pe per element."""
    n, m, k, d = 129, 300, 14, 416
    rng = np.random.default_rng(seed(('pairmlp', regime)) % 2 ** 32)
    sc = 1e-6 if regime == 'grad' else 1.0
    aq = (sc * rng.normal(size=(n, 2 * d))).astype(np.float32)
    kt = (sc * rng.normal(size=(m, 2 * d))).astype(np.float32)
    r = (sc * np.abs(rng.normal(size=(n * k, 32)))).astype(np.float32)
    if regime == 'grad':
        aq = (aq * loguniform(rng, 1e-6, 1e2, (n, 1), signed=False)).astype(np.float32)
    idx = attn_idx(rng, n, m, k)
    c2 = (sc * rng.normal(size=d)).astype(np.float32)
    wp, w2, p2 = ((s_ * rng.normal(size=sh)).astype(np.float32) for s_, sh in ((0.1, (2 * d, 32)), (0.03, (d, 2 * d)),
                                                                            (0.1, (d, 32))))
    ws = pk.ops.pack_attn_bf16x6_stream(dev(w2), dev(wp), dev(p2))
    a, lg, pe = (t.cpu().numpy() for t in pk.ops.pt_pair_mlp_bf16x6(dev(aq), dev(kt), dev(r), torch.from_numpy(idx).cuda(),
                                                                     dev(c2), ws))
    j = idx.reshape(-1).astype(np.int64)
    i = np.repeat(np.arange(n), k)
    init = (aq[i] - kt[j]).astype(np.float64)
    mo, ex, s, cb = ss.rowlin(r, wp, None, False, None, 'bf16x6')
    exact_init = aq[i].astype(np.float64) - kt[j]
    ainit = 2.0 ** -21 * (np.abs(aq[i]) + np.abs(kt[j]))              # (as in test_attention_bf16x6_pair_tensors)
    a64 = ex + exact_init
    check('pair_mlp a %s' % regime, 'bf16x6', a, mo + init, a64, s, cb + 2.0 ** -23 * np.abs(a64), extra=ainit)
    mo, ex, s, cb = ss.rowlin(np.maximum(a, 0), w2, None, False, None, 'bf16x6')
    ex64 = np.maximum(a64, 0) @ w2.astype(np.float64).T
    check('pair_mlp logits %s' % regime, 'bf16x6', lg, mo, ex64, s,
          cb + np.abs(a.astype(np.float64) - a64) @ np.abs(w2.astype(np.float64)).T)
    mo, ex, s, cb = ss.rowlin(r, p2, c2, False, None, 'bf16x6')
    check('pair_mlp pe %s' % regime, 'bf16x6', pe, mo, ex, s, cb)


# ------------------------------------------------------------------ beyond the fp16 window: loud
def test_rowlin_f16x3_activation_past_the_window_is_not_finite(pk):
    rng = np.random.default_rng(11)
    x, w, _ = operands('init', rng, 33, 416)
    x[5, 17] = 7e4
    for relu in (False, True):
        got = pk.ops.rowlin_bf16x6(dev(x), dev(w), None, relu_in=relu, scheme='f16x3').cpu().numpy()
        assert not np.isfinite(got[5]).any()
        model, exact, s, contract = ss.rowlin(np.delete(x, 5, 0), w, None, relu, None, 'f16x3')
        check('rowlin past window, other rows', 'f16x3', np.delete(got, 5, 0), model, exact, s, contract)


def test_resblock_f16x3_activation_past_the_window_is_not_finite(pk):
    """x = 7e4 in one row: its hidden units are NaN; a ReLU that dropped NaN would return exactly x + b1 for the row."""
    rng = np.random.default_rng(12)
    x, w0, _ = operands('init', rng, 33, 416)
    _, w1, _ = operands('init', rng, 1, 416)
    b0, b1 = (rng.normal(size=416).astype(np.float32) for _ in range(2))
    x[5, 17] = 7e4
    got = pk.ops.resblock_f16x3(dev(x), dev(w0), dev(b0), dev(w1), dev(b1)).cpu().numpy()
    assert not np.isfinite(got[5]).any(), 'row 5 finite: %s' % ('x + b1' if np.allclose(got[5], x[5] + b1) else 'other')
    keep = np.delete(np.arange(33), 5)
    model, exact, s, extra_a, contract = resblock_ref(x[keep], w0, b0, w1, b1)
    assert (np.abs(got[keep] - exact) <= contract).all()


def test_resblock_f16x3_weight_past_the_window_is_not_finite(pk):
    """one W0 entry of 300 (> 255.9375): the pieces of 300 * 2^8 are inf / -inf, so its hidden unit is NaN in every row
    (inf * 0 is NaN in the matrix pipe too); a ReLU that dropped NaN would return finite rows without that unit."""
    rng = np.random.default_rng(13)
    x, w0, _ = operands('init', rng, 40, 416)
    _, w1, _ = operands('init', rng, 1, 416)
    b0, b1 = (rng.normal(size=416).astype(np.float32) for _ in range(2))
    w0[9, 21] = 300.0
    got = pk.ops.resblock_f16x3(dev(x), dev(w0), dev(b0), dev(w1), dev(b1)).cpu().numpy()
    assert (~np.isfinite(got)).any(axis=1).all(), '%d of 40 rows finite' % np.isfinite(got).all(axis=1).sum()


@pytest.mark.parametrize('kernel', ['f16x3', 'f16w'])
def test_attention_f16_merged_wp_past_the_window_is_not_finite(pk, kernel):
    """a merged Wp entry of 5000 (> 65504 / 16): with every r_p of that input > 0, every row must come out non-finite."""
    n, m, k = 17, 76, 14
    rng = np.random.default_rng(14)
    ins = attn_inputs(rng, n, m, k, 'init')
    ins[2][3, 7] = 5000.0
    ins[7][7] = 0.0                      # P1 row 7 = 0, c1[7] = 1: r_p[7] = 1 for every pair
    ins[8][7] = 1.0
    got = run_attn(pk, kernel, ins, attn_idx(rng, n, m, k), n, m, k)
    assert (~np.isfinite(got)).any(axis=1).all()


# ------------------------------------------------------------------ path level
def path_inputs():
    """G8r inputs (attention weights x 8) with the to_q column of each cross layer that carries the largest merged W1 Wq
    entry x 4 more: merged entries ~20 (the f16x3 window of the merged projection is |W1 Wq| < 255.9; 16 times less if
    the hidden scale went into its packed weights), raw |w| < 5, hidden activations < 750."""
    q, abstract, fglob, ia, sd = gc.dec_inputs(gc.DEC_REGIME_CASES[1])
    sd = dict(sd)
    for j in range(ia['cross_attn_layers']):
        kq, k1 = 'pt_blocks.%d.layer2.to_q.weight' % j, 'pt_blocks.%d.layer2.attn_mlp.0.weight' % j
        v = int((sd[k1].double() @ sd[kq].double()).abs().max(0).values.argmax())
        sd[kq] = sd[kq].clone()
        sd[kq][:, v] *= 4.0
        assert float((sd[k1].double() @ sd[kq].double()).abs().max()) > 16.0
    return q, abstract, fglob, ia, sd


@pytest.mark.parametrize('scheme', ['f16x3', 'bf16x6'])
def test_decoder_split_precision_with_large_merged_query_weights(pk, scheme):
    """path_inputs through the whole decoder in the split scheme against the CPU oracle in fp64, at
    max(1e-4, 2 |oracle fp32 - oracle fp64|) (golden_cases.regime_bound's rule)."""
    from oracle import path as op
    q, abstract, fglob, ia, sd = path_inputs()
    net = pk.implicit.LocalPclResnetFC(**ia).cuda().eval()
    net.load_state_dict(sd)
    with torch.no_grad(), pk.kernels(precision=scheme):
        out, _ = net(dev(q), dev(abstract), dev(fglob), None)
    out = out.cpu().numpy().astype(np.float64)
    t = torch.from_numpy
    o32, _ = op.decoder_forward(sd, ia, t(q), t(abstract), t(fglob))
    sd64 = {kk: v.double() for kk, v in sd.items()}
    o64, _ = op.decoder_forward(sd64, ia, t(q).double(), t(abstract).double(), t(fglob).double())
    o32, o64 = o32.numpy().astype(np.float64), o64.numpy()
    bound = max(1e-4, 2.0 * float(np.abs(o32 - o64).max()))
    err = float(np.abs(out - o64).max()) if np.isfinite(out).all() else float('inf')
    print('\n[decoder %s, merged W1 Wq ~20] |hip - oracle64| %.3g (bound %.3g)' % (scheme, err, bound))
    assert err <= bound


def test_decoder_f16x3_weight_past_the_window_raises(pk):
    q, abstract, fglob, ia, sd = gc.dec_inputs(gc.DEC_REGIME_CASES[0])
    sd = dict(sd)
    key = 'blocks.0.fc_0.weight'
    w = sd[key].clone()
    w[3, 5] = 300.0
    sd[key] = w
    net = pk.implicit.LocalPclResnetFC(**ia).cuda().eval()
    net.load_state_dict(sd)
    with torch.no_grad(), pk.kernels(precision='f16x3'):
        with pytest.raises(AssertionError, match='block 0 fc_0'):
            net(dev(q), dev(abstract), dev(fglob), None)
    with torch.no_grad(), pk.kernels(precision='bf16x6'):      # no range restriction there
        out, _ = net(dev(q), dev(abstract), dev(fglob), None)
    assert torch.isfinite(out).all()
