"""numpy model of the two split-precision schemes of csrc/bf16x6.hpp (a plain helper module of the suite).

fp16 x 2 pieces ('f16x3'), 3 kept products:
    xs = x * s (fp32, exact),  x1 = rn_f16(xs),  x2 = rn_f16(xs - x1)   (the residual in fp32, exact)
    a b ~ a1 b1 + a1 b2 + a2 b1
s = 1 for activations, F16_WSCALE (2^8) for packed weights.  numpy's float32 -> float16 cast rounds to nearest even,
keeps subnormals and overflows to inf: the conversion v_cvt_pk_f16_f32 makes in the default mode.

bf16 x 3 pieces ('bf16x6'), 6 kept products:
    h = trunc_bf16(x),  m = trunc_bf16(x - h),  l = trunc_bf16(x - h - m)   (x = h + m + l exactly)
    a b ~ a1 b1 + a1 b2 + a2 b1 + a2 b2 + a1 b3 + a3 b1

The model sums the kept products in fp64: a kernel differs from it only by its fp32 accumulation order.
`contract_bound` is the per-element error against the exact product that the header comments state.
"""
import numpy as np

SCHEMES = ('f16x3', 'bf16x6')
F16_WSCALE = 256.0          # SplitF16x3::WSCALE
F16_HSCALE = 16.0           # SplitF16x3::HSCALE (the attention kernel's hidden activations)
ACC = 8 * 2.0 ** -24        # fp32 accumulation allowance per unit of sum |x w| (the suite's GEMM bound)

# the fp16 scheme's representation error of x * s (divided back by s): relative above the threshold, absolute below it
F16_REL = 2.0 ** -23
F16_THRESH = 0.25           # below |x s| = 0.25 the second piece is an fp16 subnormal
F16_ABS = 2.0 ** -25
F16_DROP = 2.0 ** -22       # the dropped a2 b2, relative to |a b|
BF16_DROP = 2.0 ** -21      # the dropped a2 b3 + a3 b2 + a3 b3, relative to |a b| (tests/test_split_scheme.py: reached)

# the windows: the largest |x s| whose leading fp16 piece is finite (65520 rounds to inf)
F16_MAX = 65520.0


def f16_pieces(x, scale=1.0):
    """the two fp16 pieces of x * scale as float64 arrays (still in scaled units; may be +-inf outside the window)."""
    with np.errstate(over='ignore', invalid='ignore'):
        xs = np.asarray(x, dtype=np.float32) * np.float32(scale)
        p1 = xs.astype(np.float16)
        r = xs - p1.astype(np.float32)
        p2 = r.astype(np.float16)
    return p1.astype(np.float64), p2.astype(np.float64)


def _trunc_bf16(x):
    return (np.asarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def bf16_pieces(x):
    """the three bf16 truncation pieces of x (split2 of csrc/bf16x6.hpp) as float64 arrays."""
    x = np.asarray(x, dtype=np.float32)
    h = _trunc_bf16(x)
    r = x - h
    m = _trunc_bf16(r)
    t = r - m
    l_ = _trunc_bf16(t)
    return h.astype(np.float64), m.astype(np.float64), l_.astype(np.float64)


def represent(x, scheme, scale=1.0):
    """the value the kept pieces carry (fp64), dropped products aside."""
    if scheme == 'f16x3':
        p1, p2 = f16_pieces(x, scale)
        return (p1 + p2) / scale
    h, m, l_ = bf16_pieces(x)
    return h + m + l_


def rep_bound(x, scheme, scale=1.0):
    """per-element bound of |x - represent(x)| the header states."""
    ax = np.abs(np.asarray(x, dtype=np.float64))
    if scheme == 'bf16x6':
        return np.zeros_like(ax)
    return np.where(ax * scale >= F16_THRESH, F16_REL * ax, F16_ABS / scale)


def kept_matmul(x, w, scheme, wscale=None):
    """sum_k of the kept partial products of x (n, K) against w (n_out, K), in fp64, (n, n_out).  `wscale`: the power
    of two the packer multiplies the weights with (f16x3: F16_WSCALE unless the caller packs otherwise)."""
    if scheme == 'f16x3':
        ws = F16_WSCALE if wscale is None else wscale
        a1, a2 = f16_pieces(x)
        b1, b2 = f16_pieces(w, ws)
        return (a1 @ b1.T + a1 @ b2.T + a2 @ b1.T) / ws
    a = bf16_pieces(x)
    b = bf16_pieces(w)
    return (a[2] @ b[0].T + a[0] @ b[2].T + a[1] @ b[1].T + a[1] @ b[0].T + a[0] @ b[1].T + a[0] @ b[0].T)


def abs_sum(x, w, scheme=None, wscale=None):
    """sum_k |x_k w_k| (n, n_out) in fp64 -- of the represented operands when a scheme is given."""
    if scheme is not None:
        ws = (F16_WSCALE if wscale is None else wscale) if scheme == 'f16x3' else 1.0
        x, w = represent(x, scheme), represent(w, scheme, ws)
    return np.abs(np.asarray(x, dtype=np.float64)) @ np.abs(np.asarray(w, dtype=np.float64)).T


def contract_bound(x, w, scheme, wscale=None, acc=ACC):
    """per-element bound of |split GEMM - exact x w^T| (n, n_out): the operands' representation errors through the
    other operand, their product, the dropped partial products and `acc` x sum |x w| of fp32 accumulation."""
    ws = (F16_WSCALE if wscale is None else wscale) if scheme == 'f16x3' else 1.0
    x64, w64 = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    ex, ew = rep_bound(x64, scheme), rep_bound(w64, scheme, ws)
    drop = F16_DROP if scheme == 'f16x3' else BF16_DROP
    s = np.abs(x64) @ np.abs(w64).T
    return ex @ np.abs(w64).T + np.abs(x64) @ ew.T + ex @ ew.T + (drop + acc) * s


def product_error(x, w, scheme, wscale=None):
    """elementwise |x w - kept products of (x, w)| in fp64 (x, w broadcast against each other)."""
    x, w = np.broadcast_arrays(np.asarray(x, dtype=np.float32), np.asarray(w, dtype=np.float32))
    exact = x.astype(np.float64) * w.astype(np.float64)
    if scheme == 'f16x3':
        ws = F16_WSCALE if wscale is None else wscale
        a1, a2 = f16_pieces(x)
        b1, b2 = f16_pieces(w, ws)
        kept = (a1 * b1 + a1 * b2 + a2 * b1) / ws
    else:
        a, b = bf16_pieces(x), bf16_pieces(w)
        kept = a[2] * b[0] + a[0] * b[2] + a[1] * b[1] + a[1] * b[0] + a[0] * b[1] + a[0] * b[0]
    return np.abs(kept - exact)


def product_bound(x, w, scheme, wscale=None):
    """elementwise counterpart of contract_bound without the accumulation term."""
    ws = (F16_WSCALE if wscale is None else wscale) if scheme == 'f16x3' else 1.0
    x64, w64 = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64))
    ex, ew = rep_bound(x64, scheme), rep_bound(w64, scheme, ws)
    drop = F16_DROP if scheme == 'f16x3' else BF16_DROP
    return ex * np.abs(w64) + np.abs(x64) * ew + ex * ew + drop * np.abs(x64 * w64)


def rowlin(x, w, b=None, relu_in=False, res=None, scheme='f16x3', wscale=None):
    """y = [res +] w [relu](x) + b as the split row kernel computes it -> (model, exact, sum |x~ w~|, contract), fp64.
    model: the kept products in fp64 (+ bias / residual); exact: fp64 of the fp32 operands."""
    x = np.asarray(x, dtype=np.float32)
    xin = np.maximum(x, np.float32(0)) if relu_in else x
    add = 0.0
    if b is not None:
        add = add + np.asarray(b, dtype=np.float64)
    if res is not None:
        add = add + np.asarray(res, dtype=np.float64)
    model = kept_matmul(xin, w, scheme, wscale) + add
    exact = xin.astype(np.float64) @ np.asarray(w, dtype=np.float64).T + add
    s = abs_sum(xin, w, scheme, wscale)
    # + the fp32 roundings of the epilogue (bias, residual) on the result
    contract = contract_bound(xin, w, scheme, wscale) + 2.0 ** -23 * (np.abs(exact) + np.abs(np.asarray(add)))
    return model, exact, s, contract
