"""A plain statement of the fused vector-attention contract of include/occ4d.h (occ4d_pt_cross_attn_f32,
occ4d_pt_cross_attn16p_f32 / _logits_f32, occ4d_pt_self_attn16_f32), the seeded operand sets the direct kernel tests
run on, and the rule that sizes their tolerance.

With j = idx[i, s], in the merged form of DESIGN.md 4 (i):
    r      = relu(P1 (qpos_i - apos_j) + c1)                          (32)
    a      = aq_i - kt_j + Wp r                                       (2d)   hidden pre-activation
    logit  = W2 relu(a) (+ b2)                                        (d)
    pe     = P2 r + c2                                                (d)
    agg[i, c] = sum_s softmax_s(logit[c] / divisor) (vt[j, c] + pe[c])
`c2_in_vt`: the 16p kernels take the value table with c2 folded in (vt = Wv f + c2) and add P2 r alone.

attention_reference() evaluates this in whatever numpy dtype it is given: float64 is the reference the kernels are
compared with, float32 (same formula, numpy's op order) only measures how far an honest fp32 evaluation lies from
it.  Tolerance of a case, from the reference alone:  E32 = max|fp32 - fp64|, S = max|fp64|,
    bound = max(4 E32, 16 2^-24 S)
(4: another summation order and v_exp_f32 instead of expf; the floor keeps a lucky fp32 run from demanding 0), and the
operands are chosen so that bound <= 2e-5 max(1, S), the chain tolerance of the rest of the suite
(tests/test_attention_contract_reference.py checks that without a GPU)."""
import numpy as np

CHAIN_TOL = 2e-5
MI355X_CUS = 256           # operand sets that depend on the CU count are sized with this where no GPU is present


def bound(e32, s):
    return max(4.0 * e32, 16.0 * 2.0 ** -24 * s)


def attention_reference(op, dtype=np.float64, want_pairs=False, chunk=256):
    """op: dict of the operands (aq, qpos, apos, idx, kt, vt, P1, c1, wp, w2, p2, c2, divisor [, b2, c2_in_vt]).
    -> dict(agg (n, d), wmax (n, d) largest softmax weight per cell, live (n, d) number of non-zero weights per cell,
    dom (n, d) value v + pe of the neighbour with the largest logit [, a (n k, 2d), logits (n k, d) without b2,
    pe (n k, d)])."""
    f = lambda t: np.asarray(t).astype(dtype)                      # noqa: E731
    aq, kt, vt = f(op['aq']), f(op['kt']), f(op['vt'])
    qpos, apos = f(op['qpos'])[:, :3], f(op['apos'])[:, :3]
    P1, c1, wp, w2, p2, c2 = (f(op[k]) for k in ('P1', 'c1', 'wp', 'w2', 'p2', 'c2'))
    b2 = f(op['b2']) if op.get('b2') is not None else None
    div = dtype(op['divisor'])
    idx = np.asarray(op['idx']).astype(np.int64)
    n, k = idx.shape
    d = vt.shape[1]
    out = dict(agg=np.empty((n, d), dtype), wmax=np.empty((n, d), dtype), live=np.empty((n, d), np.int64),
               dom=np.empty((n, d), dtype))
    if want_pairs:
        out.update(a=np.empty((n * k, 2 * d), dtype), logits=np.empty((n * k, d), dtype), pe=np.empty((n * k, d), dtype))
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        j = idx[lo:hi]
        rel = qpos[lo:hi, None, :] - apos[j]                        # (c, k, 3)
        r = np.maximum(rel @ P1.T + c1, 0)                          # (c, k, 32)
        a = aq[lo:hi, None, :] - kt[j] + r @ wp.T                   # (c, k, 2d)
        logit = np.maximum(a, 0) @ w2.T                             # (c, k, d)
        pe_r = r @ p2.T
        pe = pe_r + c2
        val = vt[j] + (pe_r if op.get('c2_in_vt') else pe)
        z = (logit if b2 is None else logit + b2) / div
        z = z - z.max(axis=1, keepdims=True)
        e = np.exp(z)
        w = e / e.sum(axis=1, keepdims=True)
        out['agg'][lo:hi] = (w * val).sum(axis=1)
        out['wmax'][lo:hi] = w.max(axis=1)
        out['live'][lo:hi] = (w > 0).sum(axis=1)
        out['dom'][lo:hi] = np.take_along_axis(val, z.argmax(axis=1)[:, None, :], axis=1)[:, 0, :]
        if want_pairs:
            out['a'][lo * k:hi * k] = a.reshape(-1, 2 * d)
            out['logits'][lo * k:hi * k] = logit.reshape(-1, d)
            out['pe'][lo * k:hi * k] = pe.reshape(-1, d)
    return out


def merged_operands(sd, x, pos, x2, pos2, idx):
    """The operands of the contract from a PointTransformerLayer state dict and its inputs, merged in fp64 as
    DESIGN.md 4 (i) does: aq = (W1 Wq) x + W1 (bq - bk + c2) + b1, kt = (W1 Wk) x2, vt = Wv x2 + bv, Wp = W1 P2."""
    g = lambda name: sd[name].double().numpy() if name in sd else 0.0     # noqa: E731
    x, x2 = np.asarray(x, np.float64), np.asarray(x2, np.float64)
    W1, b1 = g('attn_mlp.0.weight'), g('attn_mlp.0.bias')
    P2, c2 = g('pos_mlp.2.weight'), g('pos_mlp.2.bias')
    d = P2.shape[0]
    return dict(aq=x @ (W1 @ g('to_q.weight')).T + (W1 @ (g('to_q.bias') - g('to_k.bias') + c2) + b1),
                kt=x2 @ (W1 @ g('to_k.weight')).T, vt=x2 @ g('to_v.weight').T + g('to_v.bias'),
                qpos=np.asarray(pos), apos=np.asarray(pos2), idx=np.asarray(idx),
                P1=g('pos_mlp.0.weight'), c1=g('pos_mlp.0.bias'), wp=W1 @ P2, w2=g('attn_mlp.2.weight'),
                b2=g('attn_mlp.2.bias'), p2=P2, c2=c2, divisor=np.sqrt(d))


# ------------------------------------------------------------------------------------------------ operand sets
# Row strides as (pad of ld_aq, pad of ld_kt, pad of ld_vt, pad of ld_agg, stride of qpos, stride of apos): the operands
# are cut out of wider buffers of noise.  The self kernel needs ld_vt, ld_agg % 4 == 0 (SELF_LAYOUTS).
CROSS_LAYOUTS = [(4, 64, 1, 3, 3, 4), (64, 4, 3, 1, 4, 8), (4, 4, 1, 1, 8, 3), (64, 64, 3, 3, 3, 3)]
SELF_LAYOUTS = [(4, 64, 4, 4, 3, 4), (64, 4, 4, 4, 4, 8), (4, 4, 4, 4, 8, 3)]


def _case(kernel, d, n, m, k, lists, regime):
    return dict(kernel=kernel, d=d, n=n, m=m, k=k, lists=lists, regime=regime,
                name='%s_d%d_n%s_m%d_k%d_%s_%s' % (kernel, d, n, m, k, lists, regime))


# lists: uniform = any index of [0, m); repeat = a few distinct indices per row, repeated; one = the whole row is one
# index; ends = only 0 and m - 1; distinct = a random subset in random order (what the underflow regime needs: ONE
# dominant neighbour).  n = 'rounds': more than 9 * 2 * cu_count queries with a ragged tail (a second dispatch round).
CROSS_CASES = [
    _case('16p', 416, 1, 76, 14, 'uniform', 'init'),
    _case('16p', 416, 8, 14, 13, 'repeat', 'init'),
    _case('16p', 416, 9, 531, 8, 'uniform', 'saturated'),
    _case('16p', 416, 10, 4096, 5, 'ends', 'init'),
    _case('16p', 416, 17, 76, 2, 'one', 'init'),
    _case('16p', 416, 19, 1, 1, 'one', 'init'),
    _case('16p', 416, 19, 14, 14, 'one', 'init'),
    _case('16p', 416, 130, 531, 14, 'uniform', 'saturated'),
    _case('16p', 416, 1003, 76, 13, 'distinct', 'underflow'),
    _case('16p', 416, 1003, 76, 5, 'one', 'init'),
    _case('16p', 416, 10, 4096, 8, 'uniform', 'equal'),
    _case('16p', 416, 17, 531, 5, 'distinct', 'underflow'),
    _case('16p', 416, 9, 1, 14, 'one', 'init'),
    _case('16p', 416, 8, 14, 2, 'ends', 'saturated'),
    _case('16p', 416, 19, 76, 14, 'repeat', 'init'),
    _case('16p', 416, 'rounds', 4099, 14, 'uniform', 'init'),
    _case('first', 288, 19, 76, 14, 'uniform', 'init'),
    _case('first', 288, 10, 531, 5, 'uniform', 'saturated'),
    _case('first', 288, 10, 14, 5, 'repeat', 'init'),
    _case('first', 288, 1003, 14, 13, 'one', 'init'),
    _case('first', 288, 9, 1, 1, 'one', 'init'),
    _case('first', 416, 17, 76, 8, 'uniform', 'init'),
    _case('first', 416, 1003, 531, 14, 'distinct', 'underflow'),
    _case('first', 416, 1, 4096, 2, 'ends', 'equal'),
    _case('first', 416, 8, 76, 13, 'one', 'init'),
]
SELF_CASES = [
    _case('self', 4, 1, 1, 16, 'one', 'init'),
    _case('self', 20, 3, 76, 16, 'uniform', 'saturated'),
    _case('self', 36, 4, 76, 16, 'repeat', 'init'),
    _case('self', 72, 5, 5, 16, 'uniform', 'equal'),
    _case('self', 100, 16, 16, 16, 'distinct', 'underflow'),
    _case('self', 144, 1001, 1001, 16, 'uniform', 'init'),
    _case('self', 260, 16, 531, 16, 'uniform', 'saturated'),
    _case('self', 20, 3, 3, 16, 'ends', 'init'),
    _case('self', 288, 16, 76, 16, 'uniform', 'saturated'),
    _case('self', 288, 1001, 76, 16, 'uniform', 'init'),
    _case('self', 36, 1001, 1001, 16, 'distinct', 'underflow'),
    _case('self', 288, 5, 4096, 16, 'uniform', 'init'),
    _case('self', 4, 1001, 14, 16, 'one', 'init'),
]
ALL_CASES = CROSS_CASES + SELF_CASES


def rounds_n(cu_count):
    """More queries than the 9 * 2 * cu_count of the first dispatch round of the paired-workgroup kernel, ragged tail."""
    return 9 * 2 * cu_count + 9 * 5 + 4


def _lists(rng, n, m, k, kind):
    if kind == 'uniform':
        idx = rng.integers(0, m, size=(n, k))
    elif kind == 'repeat':
        few = rng.integers(0, m, size=(n, 3))
        idx = np.take_along_axis(few, rng.integers(0, 3, size=(n, k)), axis=1)
    elif kind == 'one':
        idx = np.repeat(rng.integers(0, m, size=(n, 1)), k, axis=1)
    elif kind == 'ends':
        idx = np.where(rng.random(size=(n, k)) < 0.5, 0, m - 1)
        idx[:, 0] = 0
        idx[:, -1] = m - 1
    elif kind == 'distinct':
        assert m >= k
        idx = np.stack([rng.permutation(m)[:k] for _ in range(n)])
    else:
        raise ValueError(kind)
    return idx.astype(np.int32)


def make_operands(case, cu_count=MI355X_CUS):
    """Seeded fp32 operands of a case (logical, contiguous arrays; the GPU tests lay them out with strides)."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(case['name'].encode()))
    d, m, k = case['d'], case['m'], case['k']
    n = rounds_n(cu_count) if case['n'] == 'rounds' else case['n']
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    op = dict(aq=f32(rng.normal(size=(n, 2 * d))), kt=f32(rng.normal(size=(m, 2 * d))), vt=f32(rng.normal(size=(m, d))),
              qpos=f32(rng.uniform(-5, 5, size=(n, 3))), apos=f32(rng.uniform(-5, 5, size=(m, 3))),
              P1=f32(0.3 * rng.normal(size=(32, 3))), c1=f32(0.3 * rng.normal(size=(32,))),
              wp=f32(0.1 * rng.normal(size=(2 * d, 32))), w2=f32(rng.normal(size=(d, 2 * d)) / np.sqrt(2 * d)),
              p2=f32(0.1 * rng.normal(size=(d, 32))), c2=f32(0.1 * rng.normal(size=(d,))),
              b2=f32(0.1 * rng.normal(size=(d,))) if case['kernel'] == 'first' else None,
              idx=_lists(rng, n, m, k, case['lists']), divisor=float(np.sqrt(np.float32(d))),
              c2_in_vt=case['kernel'] == '16p')
    regime = case['regime']
    if regime == 'equal':
        op['w2'] = np.zeros_like(op['w2'])
    elif regime == 'underflow':
        # every hidden unit grows with the neighbour's index, every weight of W2 is positive: the logits of a row's
        # neighbours are ordered like their indices in every channel, adjacent indices UNDERFLOW_GAP apart in the
        # softmax's argument (exp(-104) is already 0 in fp32)
        op['w2'] = np.abs(op['w2'])
        step = UNDERFLOW_GAP * op['divisor'] / float(op['w2'].astype(np.float64).sum(axis=1).min())
        step = float(2.0 ** np.ceil(np.log2(step)))
        base = 8.0 + float(np.abs(op['aq']).max()) + 32 * float(np.abs(op['wp']).max()) * 20.0   # keeps every unit > 0
        op['kt'] = f32(-(base + step * np.arange(1, m + 1, dtype=np.float64))[:, None] * np.ones((1, 2 * d)))
    elif regime == 'saturated':
        # the smallest scale of W2 (steps of 2^(1/4)) at which the largest weight passes 0.99 in 52 % of the cells of the
        # fp64 reference: no larger than the regime needs, because the fp32 error of the logits grows with them
        lg = attention_reference(op, want_pairs=True)['logits'].reshape(-1, k, d) / op['divisor']
        s = 1.0
        while s < 2.0 ** 16:
            z = s * lg
            e = np.exp(z - z.max(axis=1, keepdims=True))
            if ((e / e.sum(axis=1, keepdims=True)).max(axis=1) > 0.99).mean() >= 0.52:
                break
            s *= 2.0 ** 0.25
        op['w2'] = f32(op['w2'].astype(np.float64) * s)
        op['w2_scale'] = s
        # Logits of size 1e3 carry ~1e-3 of fp32 rounding, 1e-5 in the weights of a cell that is NOT saturated, and that
        # multiplies the differences between the neighbours' values: at unit-scale values 4 E32 would pass the chain
        # tolerance.  The values of this regime are 1 / 16 of the others' (vt, P2, c2), which keeps bound <= 2e-5.
        for key in ('vt', 'p2', 'c2'):
            op[key] = f32(op[key] / 16.0)
    return op


UNDERFLOW_GAP = 160.0


def case_bounds(case, op=None, want_pairs=False):
    """-> (op, ref64, {tensor: (E32, S, bound)}) from the reference alone."""
    op = make_operands(case) if op is None else op
    r64 = attention_reference(op, np.float64, want_pairs)
    r32 = attention_reference(op, np.float32, want_pairs)
    out = {}
    for key in ('agg',) + (('a', 'logits', 'pe') if want_pairs else ()):
        e32 = float(np.abs(r32[key].astype(np.float64) - r64[key]).max())
        s = float(np.abs(r64[key]).max())
        out[key] = (e32, s, bound(e32, s))
    return op, r64, r32, out


def check_regime(case, op, r64, r32):
    """What a regime promises, asserted on the reference (never on a kernel)."""
    k = op['idx'].shape[1]
    distinct = np.array([len(set(row)) for row in op['idx'].tolist()])
    if case['regime'] == 'saturated':
        assert (r64['wmax'] > 0.99).mean() >= 0.5, 'saturated: largest weight > 0.99 in under half of the cells'
    if case['regime'] == 'underflow':
        assert (distinct == k).all()
        assert (r32['live'] == 1).all() and (r32['wmax'] == 1).all(), 'underflow: another weight is non-zero in fp32'
        assert np.isfinite(r64['agg']).all() and np.abs(r64['agg'] - r64['dom']).max() <= 1e-12 * max(1.0, np.abs(r64['dom']).max())
    if case['regime'] == 'equal':
        assert np.abs(r64['wmax'] - 1.0 / k).max() < 1e-12
    if case['lists'] == 'one':
        assert np.abs(r64['agg'] - r64['dom']).max() <= 1e-12 * max(1.0, np.abs(r64['dom']).max())
