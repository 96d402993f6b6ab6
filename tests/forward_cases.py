"""Shared by tests/test_forward_host.py (through the g++ twin) and tests/test_gpu_forward_edges.py (on the device): the case
matrices, the fp64 references, the derived bounds and the check_* functions of the fp32 Linear (csrc/linear.hip: every column-tile
count NT x every epilogue EPI, the swish-on-load template) and of the forward reductions of csrc/pointops.hip (interp_add,
mean_rows, layernorm).  No GPU in here: every check_* takes the package and a torch device and runs one case through pk.ops.

Bounds are derived, not tuned (U = 2^-24, the unit roundoff of fp32; the argument is the one in the module docstring of
tests/test_gpu_backward_edges.py: a fp32 sum of L terms in ANY order is within (L - 1) U sum|term| of the exact sum to first
order, a term that is itself the rounded result of c fp32 operations adds c more, 2 is constant slack).

Linear, per output element, against the fp64 value of the same fp32 inputs, a = act(x):

    |got - ref| <= (K + c + 2) U (sum_k |a_k w_k| + |bias| + |add| + |sub| + |residual|)

c = 1 for the product + 1 per epilogue term present.  relu_out is 1-Lipschitz: the bound of the value before it holds after it.
For relu_in = 2 the term a_k is a rounded swish x * (1 / (1 + exp(-x))) whose exp (__expf on the device) has no stated ulp bound
in this tree, so its allowance is measured, not fixed: `swish_allowance()` is the worst relative error, in units of U, of a numpy
float32 evaluation of the same expression against fp64 over 200 000 uniform samples of [-20, 20]; the kernel is allowed four times
that, at least 8 units, added to c (the precedent is the Fourier-feature test of tests/test_gpu_small_kernels.py).

interp_add (x += cvec + sum_j w_j t_j, k neighbours): products (1), the k - 1 additions of the sum, + cvec, + x:

    |got - ref| <= (k + 3 + 2) U (sum_j |w_j t_j| + |cvec| + |x_old|)

The operation order is documented in the source (s = ((w0 t0) + w1 t1) + ..., then + cvec, then + x; no FMA contraction), so the
device must ALSO equal `restate_interp(order='device')` bit for bit, whichever of its three kernels takes the call.  The g++ twin
adds cvec first (order='twin'): with a cvec only that restatement is compared equal on the host.

mean_rows (n rows): the n - 1 additions and the division:

    |got - ref| <= (n + 1 + 2) U sum_i |x_i| / n          per column

layernorm (row of d values, mu, var the exact statistics of the fp32 row, rstd = 1 / sqrt(var + eps), y the exact output):
  * the fp32 mean (d - 1 additions, one division) is off by at most dmu = (d + 1) U mean|x|; this shift reaches every output of the
    row multiplied by rstd |gamma|.  To first order the variance does not see it: sum(x - mu) = 0.
  * the variance: each (x - mean) is rounded (1), squared (2 more: twice the relative error of the factor, and the product's own
    rounding makes 3), d - 1 additions, / d (1), + eps (1): (d + 4) U relative; the square root halves that and adds its own
    rounding (1), the reciprocal one more: rstd is within (d / 2 + 4) U relative.
  * the output: (x - mean) rounded (1), * rstd (1), * gamma (1): with the above (d / 2 + 7) U of |x - mu| rstd |gamma|; c = 8
    leaves the constant slack of the other bounds.
  * + beta: one rounding of the result, at most U |y|; U (|beta| + |y|) is allowed.

    |got - y| <= |gamma| rstd (dmu + |x - mu| (d / 2 + 8) U) + U (|beta| + |y|)

relu is 1-Lipschitz.  A row of one dyadic constant (its fp32 partial sums are exact, so the fp32 mean is the constant itself) and
every row of d = 1 have x - mean == 0 exactly: the output must be exactly beta, relu(beta), or 0."""
import collections
import functools
import os
import re
import zlib

import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24
SENTINEL = 0x7FA5C3D1          # the NaN bit pattern of tests/test_gpu_attention_contract.py: no kernel computes it
GUARD_ROWS = 2
PAD = 8                        # a strided array has ld = width + PAD; the view starts 4 floats (aligned) or 1 float (not) into its rows
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINEAR_HIP = os.path.join(ROOT, 'occlusions-4d_amd', 'csrc', 'linear.hip')


# ---------------------------------------------------------------------------------------------------------------- plumbing
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def sentinel(rows, cols):
    return np.full((rows, cols), SENTINEL, dtype=np.int32).view(F32)


def to_device(a, device):
    """Host array -> tensor on `device`, bits preserved (the CPU copy is torch's own, 64-byte aligned allocation)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.clone() if torch.device(device).type == 'cpu' else t.to(device)


def host(t):
    return t.detach().cpu().numpy()


def framed(a, off, device, guard=0, pad=PAD):
    """-> (buffer, view): `a` (rows, cols) as the view buffer[:rows, off:off + cols] of a (rows + guard, cols + pad) buffer whose
    every other float holds the sentinel."""
    rows, cols = a.shape
    buf = sentinel(rows + guard, cols + pad)
    buf[:rows, off:off + cols] = a
    buf = to_device(buf, device)
    return buf, buf[:rows, off:off + cols]


def frame_intact(buf, rows, off, cols, what):
    """Every float of `buf` outside [0, rows) x [off, off + cols) still holds the sentinel."""
    bits = host(buf.view(torch.int32)) != SENTINEL
    bits[:rows, off:off + cols] = False
    assert not bits.any(), '%s: %d floats outside the view were written' % (what, int(bits.sum()))


def within(got, ref, bound, what=''):
    """Every element of the float32 `got` within `bound` of the fp64 `ref` (a NaN is outside) -> the worst error / bound."""
    got = np.asarray(got)
    assert got.dtype == F32 and got.shape == ref.shape == bound.shape, (what, got.dtype, got.shape, ref.shape, bound.shape)
    err = np.abs(got.astype(np.float64) - ref)
    bad = ~(err <= bound)
    if bad.any():
        at = np.unravel_index(np.argmax(np.where(bad, np.nan_to_num(err, nan=np.inf) / np.maximum(bound, 1e-300), 0)), err.shape)
        raise AssertionError('%s: %d elements outside the bound; worst at %s: got %r, fp64 %r, error %.3g, bound %.3g'
                             % (what, int(bad.sum()), at, got[at], ref[at], err[at], bound[at]))
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def scaled_rows(rng, a, lo, hi):
    """Rows of `a` times 2^e, e uniform in [lo, hi]: no rounding changes, the magnitudes spread over (hi - lo) binades."""
    e = rng.integers(lo, hi + 1, size=a.shape[0])
    return np.ldexp(a.astype(F32), e[:, None]).astype(F32), e


# ---------------------------------------------------------------------------------------------------------------- the launch rule
NT_TABLE = (13, 9, 5, 4, 3, 2, 1)
BM = 128
MIN_WORKGROUPS = 128


def cdiv(a, b):
    return -(-a // b)


def picked_nt(M, N):
    """The column-tile count occ4d_linear_f32 launches for an (M, N) output: the smallest of the table that covers N (else 13),
    stepped down while the grid has fewer than 128 workgroups.  The device cannot report which instantiation ran: this
    restatement is what the coverage assertions rest on, and `launch_rule_in_source` ties it to the source text."""
    pick = 0
    for i in range(6, -1, -1):
        if 32 * NT_TABLE[i] >= N or i == 0:
            pick = i
            break
    row_tiles = cdiv(M, BM)
    while pick < 6 and row_tiles * cdiv(N, 32 * NT_TABLE[pick]) < MIN_WORKGROUPS:
        pick += 1
    return NT_TABLE[pick]


def launch_rule_in_source(text=None):
    """The pieces of the launcher's choice that `picked_nt` restates are still in csrc/linear.hip as restated."""
    if text is None:
        with open(LINEAR_HIP) as f:
            text = f.read()
    flat = re.sub(r'\s+', ' ', text)
    for piece in ('static const int kNT[7] = {13, 9, 5, 4, 3, 2, 1};',
                  'constexpr int BM = 128;',
                  'if (32 * kNT[i] >= n || i == 0) { pick = i; break; }',
                  'const int row_tiles = occ4d::cdiv(a.M, BM);',
                  'while (pick < 6 && row_tiles * occ4d::cdiv(n, 32 * kNT[pick]) < 128) ++pick;'):
        assert piece in flat, 'csrc/linear.hip no longer says %r: restate picked_nt and the shapes of LINEAR_CASES' % piece
    for nt in NT_TABLE:
        assert 'launch<%d>(a, st)' % nt in flat, nt


# ---------------------------------------------------------------------------------------------------------------- Linear
# terms: b bias, o relu_out, r residual, a add_rows[row // add_div], s sub_rows[sub_idx[row]]
# layout: plain    everything contiguous, the wrapper allocates the output
#         strided  x, w, residual, add_rows, sub_rows aligned strided views (4 floats into rows of width + 8, sentinel padding);
#                  out= such a view, with guard rows behind it
#         out1     out= a view ONE float into its rows (ops._out adopts it; its base is not 16-byte aligned -> EPI 0)
#         res1     the residual is such a view (-> EPI 0), the wrapper allocates the output
#         alias    out is the residual tensor itself (the in-place residual block), contiguous
#         alias1   the same, both being the view one float into its rows (-> EPI 0)
Lin = collections.namedtuple('Lin', 'M K N relu_in terms layout add_div')


def L(M, K, N, relu_in, terms, layout='plain', add_div=1):
    assert set(terms) <= set('boras') and relu_in in (0, 1, 2) and add_div in (1, 14)
    assert layout in ('plain', 'strided', 'out1', 'res1', 'alias', 'alias1')
    assert 'r' in terms or layout not in ('res1', 'alias', 'alias1')
    # Every swish case carries an epilogue term.  With rows of x times 2^[-12, 12] a whole row can lie far below 0, where its
    # product is of the order x e^x: under fp32's normal range from x = -87 on, so NO fp32 evaluation of the sigmoid holds a
    # relative bound there (the fp64 reference is 1e-40, fp32 has flushed to 0).  The problem, not the kernel, is ill-posed on
    # such a row alone; next to a bias or a residual the row is held to the bound of the sum it is part of.
    assert relu_in != 2 or set(terms) & set('bars'), 'a swish case needs an epilogue term'
    return Lin(M, K, N, relu_in, terms, layout, add_div)


LINEAR_CASES = [
    # NT = 13: one column block of 416; 420 = 416 + 4 live columns in the second; 836 = 2 * 416 + 4
    L(16257, 4, 416, 0, 'bo'), L(16257, 8, 416, 2, 'b', 'strided'),
    L(8065, 4, 420, 1, 'boras', 'strided', 14), L(8065, 8, 420, 2, 'r', 'alias'),
    L(5377, 4, 836, 0, 'a', 'plain', 14), L(5377, 4, 836, 1, 'bs', 'out1'),
    L(16257, 4, 416, 2, 'br', 'alias1'),
    L(16300, 68, 416, 0, 'boras', 'strided', 1),                  # the largest product; K = 68: the third k-tile holds 4 of 32
    # NT = 9: 832 = 2 * 288 + 256 (the last chunk of the staged epilogue is partial); one row below the NT = 13 threshold
    L(6000, 4, 832, 0, 'b', 'strided'), L(16257, 8, 288, 1, 's'), L(16300, 4, 286, 0, 'bora', 'plain', 14),
    L(16256, 4, 416, 0, 'r', 'alias'), L(16256, 4, 416, 0, 'bo', 'out1'),
    # NT = 5
    L(16257, 4, 160, 1, 'bo'), L(16257, 4, 160, 0, 'a', 'strided', 1), L(16257, 4, 130, 2, 'bs'),
    # NT = 4
    L(16257, 8, 128, 0, '', 'strided'), L(16257, 4, 128, 2, 'boras', 'plain', 14), L(16257, 4, 98, 1, 'br', 'res1'),
    # NT = 3
    L(16257, 4, 96, 0, 'b'), L(16257, 4, 96, 1, 'r', 'strided'), L(16257, 4, 66, 0, 'boa', 'plain', 1),
    # NT = 2
    L(16257, 4, 64, 1, 'o'), L(16257, 8, 64, 0, 's', 'strided'), L(16257, 4, 34, 0, 'b', 'out1'),
    # NT = 1
    L(16257, 4, 32, 2, 'bo'), L(16257, 4, 32, 2, 'a', 'strided', 14), L(16257, 4, 5, 2, 'br'), L(16257, 4, 32, 0, 'r', 'res1'),
    # the k loop at few rows: one k-tile (K < 32), a k-tile that is half zeros, 26 k-tiles (both LDS buffers on both parities),
    # K % 4 != 0 through the wrapper's padding (of a plain and of an aligned strided operand)
    L(300, 4, 36, 0, 'b'), L(300, 8, 36, 1, 'bo', 'strided'), L(301, 36, 40, 0, 'br', 'alias'), L(300, 68, 36, 2, 'b'),
    L(257, 416, 36, 0, 'bo', 'strided'), L(257, 832, 68, 1, 'boras', 'plain', 14), L(257, 832, 36, 2, 'r', 'alias1'),
    L(300, 6, 36, 0, 'b', 'strided'), L(129, 35, 33, 2, 'br'),
]


def lin_id(c):
    return '%dx%dx%d-act%d-%s-%s%s' % (c.M, c.K, c.N, c.relu_in, c.terms or 'none', c.layout, '-div14' if c.add_div == 14 else '')


def case_epi(c):
    """The epilogue the launcher takes for a case built by `check_linear` (which asserts it from the real pointers)."""
    if c.N % 4 or c.layout in ('out1', 'res1', 'alias1'):
        return 0
    return 2 if set(c.terms) & set('ras') else 1


def picked_epi(N, pairs, bias):
    """launch<NT>'s choice from (tensor or None, row stride) of y, residual, add_rows, sub_rows, and the bias."""
    out, res, add, sub = pairs
    vec = N % 4 == 0 and (bias is None or bias.data_ptr() % 16 == 0)
    for t, ld in pairs:
        vec = vec and (t is None or (t.data_ptr() % 16 == 0 and ld % 4 == 0))
    return 0 if not vec else (2 if any(t is not None for t, _ in (res, add, sub)) else 1)


def act64(x, relu_in):
    x = x.astype(np.float64)
    if relu_in == 1:
        return np.maximum(x, 0.0)
    if relu_in == 2:
        with np.errstate(over='ignore'):
            return x * (1.0 / (1.0 + np.exp(-x)))
    return x


@functools.lru_cache(maxsize=None)
def swish_allowance():
    """-> (measured, allowed), in units of U: the worst relative error of numpy float32 x * (1 / (1 + exp(-x))) against fp64
    over 200 000 uniform samples of [-20, 20], and what the kernel's swish is allowed per term: four times that, at least 8."""
    x = np.random.default_rng(2024).uniform(-20, 20, size=200000).astype(F32)
    got = x * (F32(1) / (F32(1) + np.exp(-x)))
    assert got.dtype == F32
    ref = act64(x, 2)
    live = ref != 0
    measured = float((np.abs(got.astype(np.float64) - ref)[live] / np.abs(ref[live])).max() / U)
    return measured, max(4.0 * measured, 8.0)


SWISH_SPECIALS = (0.0, -0.0, 88.0, -88.0, 104.0, -104.0)      # exp(88) is the last finite fp32 exp, exp(104) = inf, exp(-104) = 0


def linear_inputs(c):
    """Host arrays of a case: rows of x times 2^[-12, 12], rows of w times 2^[-6, 6] (the outputs spread over ten orders of
    magnitude, so that a per-element bound sees every row); the epilogue terms on the scales of the product's factors."""
    rng = _rng('linear', *c)
    base = rng.uniform(-20, 20, size=(c.M, c.K)) if c.relu_in == 2 else rng.normal(size=(c.M, c.K))
    x, ex = scaled_rows(rng, base, -12, 12)
    if c.relu_in == 2:
        # after the scaling, one per row so that no row is made of them: first rows, the middle, the last row tile
        rows = [0, 1, 2, c.M // 2, c.M - 2, c.M - 1]
        for j, (r, v) in enumerate(zip(rows, SWISH_SPECIALS)):
            x[r, j % c.K] = v
    w, ew = scaled_rows(rng, rng.normal(size=(c.N, c.K)), -6, 6)
    h = dict(x=x, w=w)
    if 'b' in c.terms:
        h['bias'] = np.ldexp(rng.normal(size=c.N).astype(F32), ew).astype(F32)
    if 'r' in c.terms:
        h['residual'] = np.ldexp(rng.normal(size=(c.M, c.N)).astype(F32), ex[:, None]).astype(F32)
    if 'a' in c.terms:
        h['add'] = (rng.normal(size=(cdiv(c.M, c.add_div), c.N)) * 0.125).astype(F32)
    if 's' in c.terms:
        h['sub'] = (rng.normal(size=(37, c.N)) * 0.125).astype(F32)
        h['sub_idx'] = rng.integers(0, 37, size=c.M).astype(np.int32)
    return h


def linear_reference(c, h):
    """-> (fp64 result, per-element bound) of a case on the host arrays `h`."""
    a, w = act64(h['x'], c.relu_in), h['w'].astype(np.float64)
    ref, mag, n_terms = a @ w.T, np.abs(a) @ np.abs(w).T, 1
    if 'b' in c.terms:
        ref += h['bias'].astype(np.float64)
        mag += np.abs(h['bias']).astype(np.float64)
    if 'a' in c.terms:
        rows = np.arange(c.M) // c.add_div
        ref += h['add'][rows]
        mag += np.abs(h['add'][rows])
    if 's' in c.terms:
        ref -= h['sub'][h['sub_idx']]
        mag += np.abs(h['sub'][h['sub_idx']])
    if 'o' in c.terms:
        np.maximum(ref, 0.0, out=ref)
    if 'r' in c.terms:
        ref += h['residual']
        mag += np.abs(h['residual'])
    n_terms += sum(t in c.terms for t in 'bars')
    units = c.K + n_terms + 2 + (swish_allowance()[1] if c.relu_in == 2 else 0.0)
    return ref, units * U * mag


def check_linear(pk, device, c):
    """One case through ops.linear -> the worst error / bound.  Asserts the epilogue the launcher takes from the real pointers."""
    what = 'linear ' + lin_id(c)
    h = linear_inputs(c)
    ref, bound = linear_reference(c, h)
    strided = c.layout == 'strided'
    frames = []

    def place(a, off=None):
        if off is None:
            return to_device(a, device)
        buf, view = framed(a, off, device)
        frames.append((buf, a.shape[0], off, a.shape[1], 'an operand'))
        return view

    x, w = place(h['x'], 4 if strided else None), place(h['w'], 4 if strided else None)
    bias = to_device(h['bias'], device) if 'b' in c.terms else None
    add = place(h['add'], 4 if strided else None) if 'a' in c.terms else None
    sub = place(h['sub'], 4 if strided else None) if 's' in c.terms else None
    sub_idx = to_device(h['sub_idx'], device) if 's' in c.terms else None
    res = out = out_frame = None
    if c.layout in ('res1', 'alias1'):
        buf, res = framed(h['residual'], 1, device, GUARD_ROWS)
        out_frame = (buf, c.M, 1, c.N, 'the residual view')
    elif 'r' in c.terms:
        res = place(h['residual'], 4 if strided else None)
    if c.layout in ('alias', 'alias1'):
        out = res
    elif c.layout in ('strided', 'out1'):
        off = 4 if strided else 1
        buf, out = framed(sentinel(c.M, c.N), off, device, GUARD_ROWS)     # the view itself starts as sentinels too
        out_frame = (buf, c.M, off, c.N, 'out')

    def ld(t):
        return (None, 0) if t is None else (t, t.stride(0))
    epi = picked_epi(c.N, (ld(out), ld(res), ld(add), ld(sub)), bias)      # (an output the wrapper allocates is aligned)
    assert epi == case_epi(c), '%s: built for EPI %d, the launcher takes EPI %d' % (what, case_epi(c), epi)

    got = pk.ops.linear(x, w, bias, relu_in=c.relu_in, relu_out='o' in c.terms, residual=res, out=out, add_rows=add,
                        add_div=c.add_div, sub_rows=sub, sub_idx=sub_idx)
    assert got.shape == (c.M, c.N) and got.dtype == torch.float32
    assert out is None or got is out
    ratio = within(np.ascontiguousarray(host(got)), ref, bound, what)
    for frame in frames + ([out_frame] if out_frame else []):
        frame_intact(*frame[:4], what + ': ' + frame[4])
    if c.layout == 'res1':                                                # read, not written
        assert np.array_equal(host(res).view(np.int32), h['residual'].view(np.int32)), what
    return ratio


# ---------------------------------------------------------------------------------------------------------------- interp_add
# layout: plain, strided (x and table aligned views, sentinel padding, guard rows behind x), off1 (x a view one float into its rows)
Interp = collections.namedtuple('Interp', 'n d k cvec layout')
TABLE_ROWS = 50


def _interp_cases():
    cases, i = [], 0
    for n in (1, 63, 65, 1000):
        for d in (4, 36, 38, 416):
            cases.append(Interp(n, d, 8, bool(i & 1), ('plain', 'strided', 'off1')[i % 3]))
            cases.append(Interp(n, d, (1, 3, 12, 16)[i % 4], not (i & 1), ('strided', 'plain', 'off1')[(i // 4 + i) % 3]))
            i += 1
    return cases


INTERP_CASES = _interp_cases()


def interp_kernel(c):
    """Which of the three kernels occ4d_interp_add_f32 launches for a case."""
    if c.d % 4 or c.layout == 'off1':
        return 'scalar'
    return 'float4 k=8' if c.k == 8 else 'float4 runtime k'


def interp_inputs(c):
    rng = _rng('interp', *c)
    x, _ = scaled_rows(rng, rng.normal(size=(c.n, c.d)), -4, 4)
    table, _ = scaled_rows(rng, rng.normal(size=(TABLE_ROWS, c.d)), -6, 6)
    w, _ = scaled_rows(rng, rng.normal(size=(c.n, c.k)), -3, 3)
    idx = rng.integers(0, TABLE_ROWS, size=(c.n, c.k)).astype(np.int32)
    if c.k > 1:
        idx[::3, 1] = idx[::3, 0]                                          # a neighbour twice
    cvec = rng.normal(size=c.d).astype(F32) if c.cvec else None
    return dict(x=x, table=table, w=w, idx=idx, cvec=cvec)


def restate_interp(h, order='device'):
    """interp_add in numpy float32, one rounding per operation.  order='device': s = ((0 + w0 t0) + w1 t1) + ..., then + cvec,
    then x + s (the order csrc/pointops.hip documents for all three kernels); order='twin': s starts from cvec."""
    n, k = h['idx'].shape
    s = np.zeros_like(h['x'])
    if order == 'twin' and h['cvec'] is not None:
        s = s + h['cvec']
    for j in range(k):
        s = s + h['w'][:, j:j + 1] * h['table'][h['idx'][:, j]]
    if order == 'device' and h['cvec'] is not None:
        s = s + h['cvec']
    out = h['x'] + s
    assert out.dtype == F32
    return out


def interp_reference(h):
    k = h['idx'].shape[1]
    terms = h['w'].astype(np.float64)[:, :, None] * h['table'].astype(np.float64)[h['idx']]       # (n, k, d)
    ref, mag = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    if h['cvec'] is not None:
        ref, mag = ref + h['cvec'], mag + np.abs(h['cvec'])
    return ref + h['x'], (k + 3 + 2) * U * (mag + np.abs(h['x']))


def _run_interp(pk, device, h, layout, what):
    n, d = h['x'].shape
    off = {'plain': None, 'strided': 4, 'off1': 1}[layout]
    if off is None:
        buf, x = None, to_device(h['x'], device)
    else:
        buf, x = framed(h['x'], off, device, GUARD_ROWS)
    tbuf, table = framed(h['table'], 4, device) if layout == 'strided' else (None, to_device(h['table'], device))
    cvec = None if h['cvec'] is None else to_device(h['cvec'], device)
    ret = pk.ops.interp_add(x, cvec, table, to_device(h['idx'], device), to_device(h['w'], device))
    assert ret is x
    got = np.ascontiguousarray(host(x))
    if buf is not None:
        frame_intact(buf, n, off, d, what + ': x')
    if tbuf is not None:
        frame_intact(tbuf, TABLE_ROWS, 4, d, what + ': table')
        assert np.array_equal(host(table).view(np.int32), h['table'].view(np.int32)), what
    return got


def check_interp(pk, device, c, order):
    """One case through ops.interp_add -> error / bound.  `order`: the restatement the result must equal bit for bit --
    'device' on the device; on the g++ twin 'twin', which adds cvec FIRST (a different, equally valid order: where a case has
    a cvec the twin is not held to the documented device order).  An aligned case is repeated through the view one float into
    its rows: the scalar kernel must give the same bits as the float4 kernel that took the first call."""
    what = 'interp_add n=%d d=%d k=%d cvec=%s %s (%s)' % (c + (interp_kernel(c),))
    h = interp_inputs(c)
    got = _run_interp(pk, device, h, c.layout, what)
    ratio = within(got, *interp_reference(h), what)
    want = restate_interp(h, order)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), what + ': not the documented operation order'
    if interp_kernel(c) != 'scalar':
        again = _run_interp(pk, device, h, 'off1', what + ' scalar twin')
        assert np.array_equal(got.view(np.int32), again.view(np.int32)), what + ': the scalar kernel gives other bits'
    return ratio


# ---------------------------------------------------------------------------------------------------------------- mean_rows
Mean = collections.namedtuple('Mean', 'n d strided')
MEAN_CASES = [Mean(n, d, bool((i + j) & 1)) for i, n in enumerate((1, 7, 8, 9, 531, 20000)) for j, d in enumerate((1, 31, 32, 33, 288))]


def mean_inputs(c):
    """Columns of spread 2^[-6, 6]; every even column has a mean 1e3 times its spread."""
    rng = _rng('mean', *c)
    spread = np.ldexp(1.0, rng.integers(-6, 7, size=c.d))
    mean = np.where(np.arange(c.d) % 2 == 0, 1e3 * spread * rng.choice([-1.0, 1.0], size=c.d), 0.0)
    return (mean + spread * rng.normal(size=(c.n, c.d))).astype(F32)


def mean_reference(x):
    n = x.shape[0]
    x64 = x.astype(np.float64)
    return x64.sum(axis=0) / n, (n + 1 + 2) * U * np.abs(x64).sum(axis=0) / n


def restate_mean(x, order):
    """Column means in numpy float32: 'serial' adds the rows in order; 'groups' is mean_rows_kernel's order (row i goes to
    partial i % 8, the 8 partials are added in order)."""
    n, d = x.shape
    if order == 'serial':
        s = np.zeros(d, F32)
        for i in range(n):
            s = s + x[i]
    else:
        part = np.zeros((8, d), F32)
        for i in range(0, n, 8):
            rows = x[i:i + 8]
            part[:rows.shape[0]] = part[:rows.shape[0]] + rows
        s = part[0]
        for g in range(1, 8):
            s = s + part[g]
    out = s / F32(n)
    assert out.dtype == F32
    return out


def check_mean(pk, device, c):
    what = 'mean_rows n=%d d=%d strided=%s' % c
    x = mean_inputs(c)
    xt = framed(x, 3, device)[1] if c.strided else to_device(x, device)
    got = pk.ops.mean_rows(xt)
    assert got.shape == (c.d,) and got.is_contiguous()
    return within(host(got), *mean_reference(x), what)


# ---------------------------------------------------------------------------------------------------------------- layernorm
Norm = collections.namedtuple('Norm', 'n d affine relu strided kind0')
NORM_KINDS = ('normal', 'constant', 'large mean', 'times 2^12', 'times 2^-12')
EPS = 1e-5


def _norm_cases():
    cases, i = [], 0
    for j, d in enumerate((1, 2, 63, 64, 65, 416, 600)):
        for n in (1, 3, 4, 5, 1000):
            cases.append(Norm(n, d, bool(i & 1), bool(i & 2), bool(i & 4), j % len(NORM_KINDS)))
            i += 1
    return cases


NORM_CASES = _norm_cases()


def norm_inputs(c):
    """Row r is of kind NORM_KINDS[(r + kind0) % 5].  A constant row holds one dyadic value: the partial sums of its fp32 mean are
    then exact in any order, the mean is the value itself and the variance exactly 0 (with an arbitrary constant the fp32 mean
    may be one ulp off, and rstd = 1 / sqrt(eps) turns that ulp into an output of 1e-6 |gamma|: true of any fp32 evaluation,
    so the case is posed where 'exactly beta' is a property of the operation)."""
    rng = _rng('norm', *c)
    x = rng.normal(size=(c.n, c.d))
    kind = (np.arange(c.n) + c.kind0) % len(NORM_KINDS)
    const = rng.choice([-2.5, 0.75, 3.0, -1024.0, 0.0], size=c.n)
    x[kind == 1] = const[kind == 1][:, None]
    sign = rng.choice([-1.0, 1.0], size=c.n)
    x[kind == 2] += 1e3 * sign[kind == 2][:, None]
    x[kind == 3] *= 2.0 ** 12
    x[kind == 4] *= 2.0 ** -12
    gamma = rng.normal(size=c.d).astype(F32) if c.affine else None
    beta = rng.normal(size=c.d).astype(F32) if c.affine else None
    return x.astype(F32), gamma, beta, kind


def norm_reference(x, gamma, beta, relu, eps=EPS):
    """-> (fp64 result, per-element bound): the derivation is in the module docstring."""
    n, d = x.shape
    x64 = x.astype(np.float64)
    g = np.ones(d) if gamma is None else gamma.astype(np.float64)
    b = np.zeros(d) if beta is None else beta.astype(np.float64)
    mu = x64.mean(axis=1, keepdims=True)
    var = ((x64 - mu) ** 2).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + float(F32(eps)))                            # eps reaches the kernel as a float
    y = (x64 - mu) * rstd * g + b
    dmu = (d + 1) * U * np.abs(x64).mean(axis=1, keepdims=True)
    bound = np.abs(g) * rstd * (dmu + np.abs(x64 - mu) * (d / 2.0 + 8) * U) + U * (np.abs(b) + np.abs(y))
    return (np.maximum(y, 0.0) if relu else y), bound


def _sum_f32(a, order):
    """Row sums of a float32 (n, d) array: 'serial' in column order; 'lanes' is the wave's order (column c goes to lane c % 64,
    the 64 partials are folded by an xor butterfly)."""
    n, d = a.shape
    if order == 'serial':
        s = np.zeros(n, F32)
        for c in range(d):
            s = s + a[:, c]
        return s
    part = np.zeros((n, 64), F32)
    for c0 in range(0, d, 64):
        blk = a[:, c0:c0 + 64]
        part[:, :blk.shape[1]] = part[:, :blk.shape[1]] + blk
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lanes ^ o]
    assert part.dtype == F32
    return part[:, 0].copy()


def restate_norm(x, gamma, beta, relu, order, eps=EPS):
    """layernorm_kernel in numpy float32, one rounding per operation, with the two reductions in `order`."""
    d = F32(x.shape[1])
    mean = (_sum_f32(x, order) / d)[:, None]
    t = x - mean
    q = _sum_f32(t * t, order) / d
    rstd = (F32(1) / np.sqrt(q + F32(eps)))[:, None]
    y = t * rstd
    if gamma is not None:
        y = y * gamma + beta
    assert y.dtype == F32
    return np.maximum(y, F32(0)) if relu else y


def norm_exact_rows(x, gamma, beta, relu, kind, got, what):
    """Rows of one constant and every row of d = 1: exactly beta (relu(beta); 0 without gamma / beta)."""
    d = x.shape[1]
    rows = np.ones(x.shape[0], bool) if d == 1 else kind == 1
    want = np.zeros(d, F32) if beta is None else beta
    want = np.maximum(want, F32(0)) if relu else want
    assert np.array_equal(got[rows], np.broadcast_to(want, got[rows].shape)), what + ': a zero-variance row is not exactly beta'
    return int(rows.sum())


def check_norm(pk, device, c):
    what = 'layernorm n=%d d=%d affine=%s relu=%s strided=%s kind0=%d' % c
    x, gamma, beta, kind = norm_inputs(c)
    buf = None
    if c.strided:
        _, xt = framed(x, 4, device)
        buf, out = framed(sentinel(c.n, c.d), 1, device, GUARD_ROWS)
    else:
        xt, out = to_device(x, device), None
    got = pk.ops.layernorm(xt, None if gamma is None else to_device(gamma, device), None if beta is None else to_device(beta, device),
                           EPS, relu=c.relu, out=out)
    assert got.shape == (c.n, c.d) and (out is None or got is out)
    got = np.ascontiguousarray(host(got))
    if buf is not None:
        frame_intact(buf, c.n, 1, c.d, what + ': out')
    ratio = within(got, *norm_reference(x, gamma, beta, c.relu), what)
    norm_exact_rows(x, gamma, beta, c.relu, kind, got, what)
    return ratio
