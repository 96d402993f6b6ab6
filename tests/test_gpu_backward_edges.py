"""GPU: the reduction kernels under the backward pass (csrc/backward.hip) at the shapes where they take another path --
the counting-sort segmentation, the sorted-segment sum, the fixed-order sums behind ops.deterministic(), the position-MLP
gradient, the max-pool tie rule and the two small row helpers -- each against an fp64 statement of the same sum on the
same fp32 inputs.

Tolerances are derived, not tuned.  A fp32 sum of L terms in ANY order differs from the exact sum by at most
(L - 1) 2^-24 sum|term| to first order; a term that is itself the rounded result of c fp32 operations adds c more.  The
bound of one output element is therefore

    (L + c + 2) * 2^-24 * sum|term|          L: that element's own segment length, 2: constant slack

(`_within`).  An empty segment has sum|term| = 0, so its bound is 0: it must be exactly 0.0.  Where the summation order is
documented (ops.segment_gather_sum: stable by target row, pair order inside a segment; the library is built with
-ffp-contract=off) the result must also equal a numpy float32 restatement of that order bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                  # unit roundoff of fp32
TINY = np.finfo(np.float32).tiny                # smallest positive normal


@pytest.fixture(scope='module')
def pk():
    import occlusions4d_amd
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    occlusions4d_amd._lib.lib()
    return occlusions4d_amd


def C(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


def _rel(got, ref):
    """max|got - ref| / max|ref|: the measure of tests/test_gpu_kernels_random.py."""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else got
    ref = ref.detach().double().numpy() if isinstance(ref, torch.Tensor) else ref
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return np.abs(got - ref).max() / max(1e-6, np.abs(ref).max())


# ------------------------------------------------------------------ references (plain numpy / torch CPU; no GPU in here)
def _segment_reference(terms, target, n_out):
    """(fp64 sum, sum of |term|, segment length) per target row of `terms` (pairs, ...) scattered by `target` (pairs)."""
    x = torch.from_numpy(np.ascontiguousarray(terms, dtype=np.float64))
    t = torch.from_numpy(np.ascontiguousarray(target).astype(np.int64))
    shape = (n_out,) + tuple(x.shape[1:])
    ref = torch.zeros(shape, dtype=torch.float64).index_add_(0, t, x)
    mag = torch.zeros(shape, dtype=torch.float64).index_add_(0, t, x.abs())
    return ref.numpy(), mag.numpy(), np.bincount(np.asarray(target).reshape(-1), minlength=n_out)


def _bound(length, c, mag):
    length = np.asarray(length, dtype=np.float64)
    return (length.reshape(length.shape + (1,) * (np.ndim(mag) - length.ndim)) + c + 2) * U * mag


def _within(got, ref, mag, length, c, what=''):
    """Every element of `got` within (L + c + 2) 2^-24 sum|term| of the fp64 sum; empty segments exactly 0.0."""
    got = N(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == ref.shape and got.dtype == np.float32, (what, got.shape, ref.shape, got.dtype)
    err, bound = np.abs(got.astype(np.float64) - ref), _bound(length, c, mag)
    bad = err > bound
    if bad.any():
        at = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0)), err.shape)
        raise AssertionError('%s: %d elements outside the bound; worst at %s: got %r, fp64 %r, error %.3g, bound %.3g'
                             % (what, int(bad.sum()), at, got[at], ref[at], err[at], bound[at]))
    empty = np.asarray(length) == 0
    assert not np.any(got[empty]), what + ': an empty segment is not exactly 0.0'


def _stable_segments(target, n_out):
    order = np.argsort(target, kind='stable')
    off = np.concatenate([[0], np.cumsum(np.bincount(target, minlength=n_out))])
    return order, off


def _restate_gather_sum(src, target, n_out, scale, w=None, div=1):
    """ops.segment_gather_sum in numpy float32, one rounding per operation as the kernel has them:
    s = f32(s + f32(w[p] * v)) (or f32(s + v)) over the pairs of a row in pair order, then f32(scale * s).
    Vectorised over the rows: step t adds the t-th pair of every row that has one."""
    order, off = _stable_segments(target, n_out)
    cnt = np.diff(off)
    s = np.zeros((n_out, src.shape[1]), dtype=np.float32)
    for t in range(int(cnt.max()) if cnt.size else 0):
        rows = np.nonzero(cnt > t)[0]
        p = order[off[rows] + t]
        v = src[p // div]
        if w is not None:
            v = w[p][:, None] * v
        s[rows] = s[rows] + v
    assert s.dtype == np.float32
    return np.float32(scale) * s


def _maxpool_expectation(y, idx, dz):
    """(flat target element per (i, c), fp64 dy, sum|term|, length per element of dy): the gradient of row i, channel c goes to
    the LOWEST j whose y[idx[i][j]][c] equals the row maximum."""
    m, d = y.shape
    first = y[idx].argmax(axis=1)                                        # numpy: first maximum
    rows = np.take_along_axis(idx, first, axis=1)                        # (n_out, d)
    target = (rows.astype(np.int64) * d + np.arange(d)).reshape(-1)
    ref, mag, length = _segment_reference(dz.reshape(-1), target, m * d)
    return target, ref.reshape(m, d), mag.reshape(m, d), length.reshape(m, d)


def test_references_hold_their_own_bounds_on_the_host():
    """No GPU in this one: the float32 restatement of the fixed-order sum against fp64 within the bound the kernels are
    held to, the first-maximum expectation against a plain loop, and the bound helper's arithmetic -- the references
    alone stay inside the stated limits for inputs of the kind used below."""
    rng = np.random.default_rng(5)
    for n, n_out, d, k in ((3000, 1, 3, 1), (3000, 60, 96, 1), (30000, 20000, 1, 1), (500, 60, 36, 3), (500, 60, 36, 8)):
        src = rng.normal(size=(n, d)).astype(np.float32)
        target = rng.integers(0, n_out, size=n * k).astype(np.int32)
        w = rng.uniform(size=n * k).astype(np.float32) if k > 1 else None
        got = _restate_gather_sum(src, target, n_out, -1.0, w, k)
        terms = -src.astype(np.float64)[np.arange(n * k) // k] * (1.0 if w is None else w.astype(np.float64)[:, None])
        _within(got, *_segment_reference(terms, target, n_out), 1 if w is None else 2, 'restatement %s' % ((n, n_out, d, k),))
    # a sum in the reverse order stays inside the bound too (any order does), but is not the same bits everywhere
    src = rng.normal(size=(3000, 8)).astype(np.float32)
    target = rng.integers(0, 5, size=3000).astype(np.int32)
    fwd = _restate_gather_sum(src, target, 5, 1.0)
    rev = _restate_gather_sum(src[::-1], target[::-1], 5, 1.0)
    _within(rev, *_segment_reference(src, target, 5), 1, 'reverse order')
    assert not np.array_equal(fwd, rev)
    # the bound itself: (L + c + 2) 2^-24 sum|term| per element, 0 for an empty segment, violated by one part in 10^5
    ref, mag, length = _segment_reference(np.ones((6, 2)), np.array([0, 0, 0, 2, 2, 2]), 4)
    assert np.array_equal(length, [3, 0, 3, 0]) and np.array_equal(ref[:, 0], [3, 0, 3, 0]) and np.array_equal(mag, ref)
    assert np.array_equal(_bound(length, 1, mag)[:, 0], [6 * U * 3, 0, 6 * U * 3, 0])
    with pytest.raises(AssertionError):
        _within((ref * (1 + 1e-5)).astype(np.float32), ref, mag, length, 1)
    with pytest.raises(AssertionError):
        _within((ref + np.array([0, 1e-30, 0, 0])[:, None]).astype(np.float32), ref, mag, length, 1)
    # first maximum: lowest j among equals, against a plain loop
    y = np.maximum(rng.normal(size=(9, 4)), 0).astype(np.float32)
    y[[1, 4, 5]] = 0
    idx = rng.integers(0, 9, size=(7, 5)).astype(np.int32)
    dz = rng.normal(size=(7, 4)).astype(np.float32)
    loop = np.zeros((9, 4))
    for i in range(7):
        for c in range(4):
            vals = [y[idx[i, j], c] for j in range(5)]
            loop[idx[i, vals.index(max(vals))], c] += float(dz[i, c])
    assert np.array_equal(_maxpool_expectation(y, idx, dz)[1], loop)


# ------------------------------------------------------------------ 1. segmentation (counting sort)
SEG_BLOCKS, SEG_TPB, SEG_MAX_ROWS = 128, 256, 16384

SEGMENT_CASES = [(1, 1, 'uniform'), (5, 7, 'uniform'), (127, 3, 'uniform'), (128, 3, 'uniform'), (129, 3, 'uniform'),
                 (SEG_BLOCKS * SEG_TPB - 1, 1023, 'uniform'), (SEG_BLOCKS * SEG_TPB + 1, 1024, 'uniform'),
                 (100003, 1025, 'uniform'), (70001, SEG_MAX_ROWS, 'uniform'), (40000, 1, 'uniform'),
                 (40000, SEG_MAX_ROWS, 'first'), (40000, SEG_MAX_ROWS, 'last'), (SEG_MAX_ROWS, SEG_MAX_ROWS, 'once'),
                 (129, 3, 'inner'), (100003, 1025, 'inner'), (70001, SEG_MAX_ROWS, 'inner'), (5, 7, 'inner')]


def _segment_pattern(rng, n, n_out, pattern):
    if pattern == 'first':
        return np.zeros(n, dtype=np.int32)
    if pattern == 'last':
        return np.full(n, n_out - 1, dtype=np.int32)
    if pattern == 'once':
        return rng.permutation(n_out).astype(np.int32)
    if pattern == 'inner':                                                # empty rows at both ends
        lo = max(1, n_out // 3)
        return rng.integers(lo, max(lo + 1, n_out - lo), size=n).astype(np.int32)
    return rng.integers(0, n_out, size=n).astype(np.int32)


@pytest.mark.parametrize('n,n_out,pattern', SEGMENT_CASES)
def test_counting_sort_segments(pk, n, n_out, pattern):
    """occ4d_segments_build_i32 through ops._segments(stable=False): offsets are the exclusive prefix of the row counts,
    `order` is a permutation of the pairs, and the rows it lists do not decrease.  One row, rows on either side of the
    1024-thread scan, the LDS limit, fewer pairs than blocks, ragged block slices, everything on the first / last row,
    every row once, empty rows at both ends."""
    rng = np.random.default_rng(1000 * n_out + n)
    idx = _segment_pattern(rng, n, n_out, pattern)
    if pattern == 'inner':
        assert idx.min() > 0 and idx.max() < n_out - 1
    pk.ops._SEGMENTS.clear()
    order, off = pk.ops._segments(C(idx), n_out, stable=False)
    assert order.dtype == torch.int32 and off.dtype == torch.int32
    order, off = N(order), N(off)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n_out))]))
    assert order.shape == (n,) and np.array_equal(np.sort(order), np.arange(n))
    assert np.all(np.diff(idx[order]) >= 0)
    pk.ops._SEGMENTS.clear()


def test_counting_sort_argument_contract(pk):
    lib, ops = pk._lib.lib(), pk.ops
    idx = torch.zeros((8,), dtype=torch.int32, device='cuda')
    order = torch.full((8,), -1, dtype=torch.int32, device='cuda')
    off = torch.full((SEG_MAX_ROWS + 2,), -1, dtype=torch.int32, device='cuda')
    ws = torch.zeros((int(lib.occ4d_segments_workspace_ints(SEG_MAX_ROWS + 1)),), dtype=torch.int32, device='cuda')
    assert ws.numel() >= (SEG_BLOCKS + 1) * (SEG_MAX_ROWS + 1)

    def build(n, n_out):
        return lib.occ4d_segments_build_i32(ops._ptr(idx), n, n_out, ops._ptr(order), ops._ptr(off), ops._ptr(ws), ops._stream())
    assert build(8, 0) == pk._lib.EINVAL
    assert build(8, SEG_MAX_ROWS + 1) == pk._lib.EINVAL
    torch.cuda.synchronize()
    assert bool((off == -1).all()) and bool((order == -1).all())         # a rejected call writes nothing
    for n_out in (1, 5, 1025):
        off.fill_(-1)
        assert build(0, n_out) == pk._lib.OK
        got = N(off)
        assert not got[:n_out + 1].any() and np.all(got[n_out + 1:] == -1)
    assert bool((order == -1).all())


# ------------------------------------------------------------------ 2. sorted-segment sum
SORTED_LENGTHS = [0, 1, 3, 4, 5, 7, 8, 9, 5000, 0]       # the rest of the ~40 rows: 20 .. 170 pairs, ~8000 in all


@pytest.fixture(scope='module')
def sorted_case():
    """Pairs of 40 target rows whose segment lengths cover 0, 1, around the 4-unroll and around parts = 8, one hot row of
    5000 pairs, and empty rows at both ends; a wide fp32 source to slice columns from; the segmentation by a stable
    torch.sort (so that this kernel is tested apart from the counting sort)."""
    rng = np.random.default_rng(2)
    lengths = np.array(SORTED_LENGTHS[:-1] + [int(v) for v in rng.integers(20, 170, size=30)] + SORTED_LENGTHS[-1:])
    inner = rng.permutation(len(lengths) - 2) + 1                         # rows 0 and n_out - 1 stay empty
    lengths[1:-1] = lengths[inner]
    n_out, n = len(lengths), int(lengths.sum())
    assert n_out == 40 and 7000 <= n <= 10500 and lengths[0] == 0 and lengths[-1] == 0
    target = rng.permutation(np.repeat(np.arange(n_out), lengths)).astype(np.int32)
    wide = rng.normal(size=(n, 832 + 8)).astype(np.float32)
    keys, order = torch.sort(torch.from_numpy(target).long(), stable=True)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    assert np.array_equal(N(keys), np.repeat(np.arange(n_out), lengths))
    return dict(n=n, n_out=n_out, target=target, wide=wide, wide_dev=C(wide), order=order.to(torch.int32).cuda(), off=C(off))


@pytest.mark.parametrize('d', [4, 64, 100, 832])
def test_sorted_segment_sum_parts_tails_and_padding(pk, sorted_case, d):
    """occ4d_segment_sum_sorted_f32 called directly: every `parts` in {1, 3, 8, 64} (segments shorter than parts, slices that
    end in the 4-unroll's tail), a column slice as source (lds = d + 8), a padded output (ldo = d + 4) whose padding must
    survive zero_rows and the atomics, scale = -0.5."""
    lib, ops, s = pk._lib.lib(), pk.ops, sorted_case
    n, n_out, lds, ldo, sentinel = s['n'], s['n_out'], d + 8, d + 4, -7.25
    wide = s['wide_dev'][:, :lds].contiguous()
    src = wide[:, 4:4 + d]                                               # 16 bytes into the rows: still aligned
    assert src.stride(0) == lds and src.data_ptr() % 16 == 0
    ref, mag, length = _segment_reference(-0.5 * s['wide'][:, 4:4 + d].astype(np.float64), s['target'], n_out)
    for parts in (1, 3, 8, 64):
        out = torch.full((n_out, ldo), sentinel, dtype=torch.float32, device='cuda')
        rc = lib.occ4d_segment_sum_sorted_f32(ops._ptr(src), lds, ops._ptr(s['order']), ops._ptr(s['off']), n_out, d, parts,
                                              -0.5, ops._ptr(out), ldo, ops._stream())
        assert rc == pk._lib.OK
        got = N(out)
        assert np.all(got[:, d:] == sentinel), 'parts=%d: the padding columns were written' % parts
        _within(np.ascontiguousarray(got[:, :d]), ref, mag, length, 1, 'parts=%d d=%d' % (parts, d))


def test_sorted_segment_sum_argument_contract(pk, sorted_case):
    lib, ops, s = pk._lib.lib(), pk.ops, sorted_case
    n_out, d = s['n_out'], 8
    wide = s['wide_dev'][:, :24].contiguous()
    out = torch.full((n_out, 16), 3.0, dtype=torch.float32, device='cuda')

    def call(src_ptr, lds, d, parts):
        return lib.occ4d_segment_sum_sorted_f32(src_ptr, lds, ops._ptr(s['order']), ops._ptr(s['off']), n_out, d, parts, 1.0,
                                                ops._ptr(out), 16, ops._stream())
    assert call(ops._ptr(wide), 24, 6, 8) == pk._lib.EINVAL                                  # d % 4
    assert call(ops._ptr(wide), 22, d, 8) == pk._lib.EINVAL                                  # lds % 4
    assert call(ctypes.c_void_p(wide.data_ptr() + 4), 24, d, 8) == pk._lib.EINVAL           # src 4 bytes off
    assert call(ops._ptr(wide), 24, d, 0) == pk._lib.EINVAL                                  # parts = 0
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    assert call(ops._ptr(wide), 24, d, 8) == pk._lib.OK


# ------------------------------------------------------------------ 3. fixed-order segment sum
def _check_gather_sum(pk, src, target, n_out, scale, w=None, div=1, what=''):
    """ops.segment_gather_sum on the device == the float32 restatement bit for bit, and within the fp64 bound."""
    src_h = N(src)
    got = pk.ops.segment_gather_sum(src, C(target), n_out, scale=scale, weights=None if w is None else C(w), div=div)
    want = _restate_gather_sum(src_h, target, n_out, scale, None if w is None else w.reshape(-1), div)
    assert got.shape == (n_out, src_h.shape[1]) and got.is_contiguous()
    assert torch.equal(got.cpu(), torch.from_numpy(want)), what + ': not the documented summation order'
    terms = scale * src_h.astype(np.float64)[np.arange(target.size) // div]
    if w is not None:
        terms = terms * w.reshape(-1).astype(np.float64)[:, None]
    _within(got, *_segment_reference(terms, target, n_out), 1 if w is None else 2, what)


@pytest.mark.parametrize('n_out', [1, 60, 20000])
@pytest.mark.parametrize('d', [1, 3, 96])
def test_fixed_order_segment_sum_is_the_documented_order(pk, d, n_out):
    """Plain form: a strided source, scale -1, one row / a few rows / more rows than the counting sort takes (n_out >
    16384 switches inside ops._segments); empty rows among them."""
    rng = np.random.default_rng(100 * d + n_out)
    n = 30000 if n_out == 20000 else 3000
    src = C(rng.normal(size=(n, d + 5)).astype(np.float32))[:, 2:2 + d]
    assert src.stride(0) == d + 5
    target = rng.integers(0, n_out, size=n).astype(np.int32)
    if n_out > 2:
        target[target == 0] = 1                                          # row 0 and the last row: empty
        target[target == n_out - 1] = n_out - 2
    pk.ops._SEGMENTS.clear()
    with pk.ops.deterministic():
        _check_gather_sum(pk, src, target, n_out, -1.0, what='plain d=%d n_out=%d' % (d, n_out))
    pk.ops._SEGMENTS.clear()


@pytest.mark.parametrize('k', [1, 3, 8])
def test_fixed_order_segment_sum_weighted_with_div(pk, k):
    """The interpolation backward's form: pair p reads source row p // k and its own weight."""
    rng = np.random.default_rng(40 + k)
    n, m, d = 500, 60, 36
    src = C(rng.normal(size=(n, d)).astype(np.float32))
    target = rng.integers(1, m - 1, size=n * k).astype(np.int32)
    w = rng.uniform(size=(n, k)).astype(np.float32)
    pk.ops._SEGMENTS.clear()
    _check_gather_sum(pk, src, target, m, 1.0, w, k, 'weighted k=%d' % k)
    pk.ops._SEGMENTS.clear()


def test_fixed_order_segment_sum_elementwise_targets(pk):
    """The max-pool backward's form: d = 1, one target per ELEMENT, m * d > 16384 target elements."""
    rng = np.random.default_rng(44)
    m, d, n_rows = 700, 36, 900
    src = C(rng.normal(size=(n_rows * d, 1)).astype(np.float32))
    rows = rng.integers(0, 40, size=(n_rows, d))                         # few distinct rows: segments of ~20 elements
    target = (rows * d + np.arange(d)).reshape(-1).astype(np.int32)
    assert m * d > SEG_MAX_ROWS
    pk.ops._SEGMENTS.clear()
    _check_gather_sum(pk, src, target, m * d, 1.0, what='element-wise')
    pk.ops._SEGMENTS.clear()


# ------------------------------------------------------------------ 4. position-MLP gradient, both modes
def _pos_hidden_case(rng, n, k, h, m=37):
    pos = rng.uniform(-5, 5, size=(n, 4)).astype(np.float32)
    pos2 = rng.uniform(-5, 5, size=(m, 4)).astype(np.float32)
    idx = rng.integers(0, m, size=(n, k)).astype(np.int32)
    # r: exact +0.0 and -0.0 (masked: the comparison is strict), the smallest positive normal (kept), ordinary values
    kind = rng.integers(0, 6, size=(n * k, h))
    if kind.size >= 6:
        kind.reshape(-1)[-3:] = [0, 1, 2]
    r = (np.abs(rng.normal(size=(n * k, h))) + 0.01).astype(np.float32)
    r[kind == 0], r[kind == 1], r[kind == 2] = 0.0, -0.0, TINY
    gr = rng.normal(size=(n * k, h)).astype(np.float32)
    keep = (r > 0).astype(np.float64)
    assert np.array_equal(keep, (kind >= 2).astype(np.float64))
    gm = gr.astype(np.float64) * keep
    delta = (pos.astype(np.float64)[:, None, :3] - pos2.astype(np.float64)[idx, :3]).reshape(n * k, 3)
    length = keep.sum(axis=0)                                             # masked pairs add exact zeros
    ref = dict(dP1=gm.T @ delta, dP1_mag=np.abs(gm).T @ np.abs(delta), dc1=gm.sum(axis=0), dc1_mag=np.abs(gm).sum(axis=0),
               length=length)
    dev = (C(pos)[:, :3], C(pos2)[:, :3], C(idx), C(r), C(gr))
    assert dev[0].stride(0) == 4 or n == 1
    return dev, ref


def _pos_hidden_counts(h):
    counts = [(1, 1), (3, 1), (1, 3), (4, 1), (5, 1), (1, 5), (4 * 1024 - 1, 1), (273, 15), (4 * 1024 + 1, 1), (241, 17)]
    # `edge` pairs: every lane of the full grid (512 blocks x 4 slices x 64 // h pairs) runs the 8-deep loop exactly once and
    # has no tail; one pair fewer sends the last lane through the tail alone, one more gives the first lane both.  (Below
    # 8 grid strides -- every count above -- the unrolled loop does not run at all, whatever h.)
    edge = 512 * 4 * (64 // h) * 8
    counts += [(edge - 1, 1), (edge + 1, 1)]
    counts += [(edge // 16 - 1, 16), (edge // 16 + 1, 16)] if h in (32, 64) else [(300, 16)]
    return counts


@pytest.mark.parametrize('h', [1, 3, 24, 32, 33, 48, 64])
def test_pos_hidden_backward_both_modes(pk, h):
    """ops.pt_pos_hidden_bwd, atomic and deterministic: widths with a partial last slice and several pairs per slice (3, 33),
    h = 1, pair counts around the slice count, the block count and the unrolled loop's tail, 4-float position rows, r with
    exact zeros of both signs and the smallest normal.  Terms gv * (a - b): c = 3; the bias gradient sums gv itself: c = 0."""
    rng = np.random.default_rng(900 + h)
    for n, k in _pos_hidden_counts(h):
        dev, ref = _pos_hidden_case(rng, n, k, h)
        for det in (False, True):
            with pk.ops.deterministic(det):
                dP1, dc1 = pk.ops.pt_pos_hidden_bwd(*dev)
                again = pk.ops.pt_pos_hidden_bwd(*dev) if det else None
            what = 'h=%d n=%d k=%d %s' % (h, n, k, 'deterministic' if det else 'atomic')
            assert dP1.shape == (h, 3) and dc1.shape == (h,)
            _within(dP1, ref['dP1'], ref['dP1_mag'], ref['length'], 3, what + ' dP1')
            _within(dc1, ref['dc1'], ref['dc1_mag'], ref['length'], 0, what + ' dc1')
            if det:
                assert torch.equal(again[0], dP1) and torch.equal(again[1], dc1), what + ': not the same bits twice'


def test_pos_hidden_backward_rejects_wide_hidden_layers(pk):
    rng = np.random.default_rng(65)
    dev, _ = _pos_hidden_case(rng, 10, 3, 65)
    for det in (False, True):
        with pk.ops.deterministic(det):
            with pytest.raises(AssertionError):
                pk.ops.pt_pos_hidden_bwd(*dev)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 5. the remaining wrappers, deterministic and default
def _both_modes(pk, fn):
    out = {}
    for det in (False, True):
        pk.ops._SEGMENTS.clear()
        with pk.ops.deterministic(det):
            out['deterministic' if det else 'atomic'] = fn()
    pk.ops._SEGMENTS.clear()
    return out


@pytest.mark.parametrize('k,d', [(1, 5), (12, 5), (1, 72), (12, 72)])
def test_maxpool_backward_first_maximum_both_modes(pk, k, d):
    rng = np.random.default_rng(10 * k + d)
    m, n_out = 300, 233
    y = rng.normal(size=(m, d)).astype(np.float32)
    idx = rng.integers(0, m, size=(n_out, k)).astype(np.int32)
    dz = rng.normal(size=(n_out, d)).astype(np.float32)
    _, ref, mag, length = _maxpool_expectation(y, idx, dz)
    for mode, got in _both_modes(pk, lambda: pk.ops.maxpool_gather_bwd(C(y), C(idx), C(dz))).items():
        _within(got, ref, mag, length, 0, 'maxpool k=%d d=%d %s' % (k, d, mode))


@pytest.mark.parametrize('k', [1, 8])
def test_interp_backward_both_modes(pk, k):
    rng = np.random.default_rng(50 + k)
    n, m, d = 500, 60, 36
    dy = rng.normal(size=(n, d)).astype(np.float32)
    idx = rng.integers(1, m - 1, size=(n, k)).astype(np.int32)
    w = rng.uniform(size=(n, k)).astype(np.float32)
    terms = (w.astype(np.float64)[:, :, None] * dy.astype(np.float64)[:, None, :]).reshape(n * k, d)
    ref = _segment_reference(terms, idx.reshape(-1), m)
    for mode, got in _both_modes(pk, lambda: pk.ops.interp_bwd(C(dy), C(idx), C(w), m)).items():
        _within(got, *ref, 2, 'interp k=%d %s' % (k, mode))


@pytest.mark.parametrize('n,d', [(1, 36), (300, 600)])
def test_layernorm_backward_both_modes(pk, n, d):
    """One row; a width above the register path (per-row atomics in the default mode, column sums by torch in the
    deterministic one).  2e-5 relative, the bound of tests/test_gpu_kernels_random.py for this kernel."""
    rng = np.random.default_rng(n + d)
    x = rng.normal(size=(n, d)).astype(np.float32)
    gam = rng.normal(size=d).astype(np.float32)
    go = rng.normal(size=(n, d)).astype(np.float32)
    xt, gt = torch.from_numpy(x).double().requires_grad_(True), torch.from_numpy(gam).double().requires_grad_(True)
    bt = torch.zeros(d, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.layer_norm(xt, (d,), gt, bt, 1e-5).backward(torch.from_numpy(go).double())
    for mode, (dx, dg, db) in _both_modes(pk, lambda: pk.ops.layernorm_bwd(C(x), C(gam), C(go), 1e-5)).items():
        errs = (_rel(dx, xt.grad), _rel(dg, gt.grad), _rel(db, bt.grad))
        assert max(errs) <= 2e-5, (mode, errs)


def _per_pair_value_gradients(pk, logits, v, pe, idx, dagg):
    """The kernel's per-pair value gradients a_j * dagg (fp32), through the library: the terms whose sum per table row dv is."""
    lib, ops = pk._lib.lib(), pk.ops
    n, k = idx.shape
    d = logits.shape[1]
    dl, dval = torch.empty_like(logits), torch.empty_like(logits)
    rc = lib.occ4d_pt_softmax_agg_bwd_f32(ops._ptr(logits), ops._ptr(v), v.stride(0), ops._ptr(pe), ops._ptr(idx), n, k, d,
                                          ops._divisor(d), ops._ptr(dagg), dagg.stride(0), ops._ptr(dl), ops._ptr(dval), None,
                                          d, ops._stream())
    assert rc == pk._lib.OK
    return N(dval)


@pytest.mark.parametrize('with_pe', [True, False])
@pytest.mark.parametrize('k,d', [(13, 38), (13, 416), (14, 38), (14, 416)])
def test_softmax_aggregate_backward_both_modes(pk, k, d, with_pe):
    """k = 13 and d = 38: the scalar kernel; (14, 416): the 16-byte-lane kernel.  dlogits, dpe, dv against fp64 autograd at
    1e-5 relative; dv also within the summation bound of the fp64 sum of the kernel's own per-pair terms (c = 0: the terms
    are summed as they are)."""
    rng = np.random.default_rng(1000 * k + d + with_pe)
    n, m = 257, 76
    idx = rng.integers(1, m - 1, size=(n, k)).astype(np.int32)
    logits = rng.normal(size=(n * k, d)).astype(np.float32)
    v = rng.normal(size=(m, d)).astype(np.float32)
    pe = rng.normal(size=(n * k, d)).astype(np.float32) if with_pe else None
    dagg = rng.normal(size=(n, d)).astype(np.float32)
    lt, vt = (torch.from_numpy(a).double().requires_grad_(True) for a in (logits, v))
    pt = torch.from_numpy(pe).double().requires_grad_(True) if with_pe else None
    att = torch.softmax(lt.view(n, k, d) / float(np.float32(np.sqrt(d))), dim=1)
    val = vt[torch.from_numpy(idx).long()] + (pt.view(n, k, d) if with_pe else 0.0)
    (att * val).sum(dim=1).backward(torch.from_numpy(dagg).double())
    dev = (C(logits), C(v), C(pe) if with_pe else None, C(idx), C(dagg))
    dval = _per_pair_value_gradients(pk, *dev)
    assert _rel(dval, att.detach().numpy().reshape(n * k, d) * dagg.astype(np.float64).repeat(k, axis=0)) <= 1e-5
    ref = _segment_reference(dval, idx.reshape(-1), m)
    for mode, (dl, dpe, dv) in _both_modes(pk, lambda: pk.ops.pt_softmax_agg_bwd(*dev)).items():
        what = 'softmax k=%d d=%d pe=%s %s' % (k, d, with_pe, mode)
        assert _rel(dl, lt.grad) <= 1e-5 and _rel(dv, vt.grad) <= 1e-5, what
        if with_pe:
            assert _rel(dpe, pt.grad) <= 1e-5, what
            assert np.array_equal(N(dpe), dval), what
        else:
            assert dpe is None
        _within(dv, *ref, 0, what + ' dv')
    # default mode, reduction left to the caller: the triple, reduced by scatter_add_rows, is the same dv
    _, _, left = pk.ops.pt_softmax_agg_bwd(*dev, reduce_dv=False)
    if isinstance(left, tuple):
        assert (k, d) == (14, 416)
        pairs, idx32, rows = left
        assert rows == m and np.array_equal(N(pairs), dval) and np.array_equal(N(idx32), idx)
        left = pk.ops.scatter_add_rows(pairs, idx32, rows)
    else:
        assert (k, d) != (14, 416)
    assert _rel(left, vt.grad) <= 1e-5
    _within(left, *ref, 0, 'softmax k=%d d=%d pe=%s reduce_dv=False' % (k, d, with_pe))


# ------------------------------------------------------------------ 6. max-pool ties
def test_maxpool_backward_ties_go_to_the_first_neighbour_in_both_modes(pk):
    """The layer pools ReLU outputs: whole neighbourhoods tie at 0.0, neighbours repeat inside a row.  The gradient goes to
    the lowest j whose value equals the row maximum, identically in both modes: exact where a target element receives one
    contribution, else within the summation bound (c = 0); the same set of non-zero target elements."""
    rng = np.random.default_rng(6)
    m, d, n_out, k = 200, 40, 150, 12
    y = np.maximum(rng.normal(size=(m, d)), 0).astype(np.float32)
    y[rng.permutation(m)[:120]] = 0.0                                    # whole rows of zeros
    idx = rng.integers(0, m, size=(n_out, k)).astype(np.int32)
    idx[:, 3], idx[:, 7], idx[::2, 1] = idx[:, 0], idx[:, 5], idx[::2, 0]   # repeated neighbours
    dz = rng.normal(size=(n_out, d)).astype(np.float32)
    assert not np.any(dz == 0)
    gathered = y[idx]
    ties = (gathered == gathered.max(axis=1, keepdims=True)).sum(axis=1)
    all_zero = gathered.max(axis=1) == 0
    assert all_zero.mean() > 0.05 and (ties[~all_zero] > 1).any() and (ties[all_zero] == k).all()
    target, ref, mag, length = _maxpool_expectation(y, idx, dz)
    once = length == 1
    assert once.any() and (length > 1).any()
    single = np.zeros(m * d, dtype=np.float32)
    single[target] = dz.reshape(-1)                                      # (right wherever one contribution arrives)
    got = _both_modes(pk, lambda: pk.ops.maxpool_gather_bwd(C(y), C(idx), C(dz)))
    for mode, dy in got.items():
        _within(dy, ref, mag, length, 0, 'ties ' + mode)
        assert np.array_equal(N(dy)[once], single.reshape(m, d)[once]), mode
    assert np.array_equal(N(got['atomic']) != 0, N(got['deterministic']) != 0)
    assert np.array_equal(N(got['atomic']) != 0, length > 0)


# ------------------------------------------------------------------ 7. small helpers
@pytest.mark.parametrize('n,d', [(1, 1), (257, 7), (1000, 416)])
def test_add_rows_is_the_fp32_sum(pk, n, d):
    rng = np.random.default_rng(n + d)
    a, b = rng.normal(size=(n, d + 3)).astype(np.float32), (1e3 * rng.normal(size=(n, d + 6))).astype(np.float32)
    got = pk.ops.add_rows(C(a)[:, 1:1 + d], C(b)[:, 2:2 + d])
    assert got.shape == (n, d) and got.is_contiguous()
    assert np.array_equal(N(got), a[:, 1:1 + d] + b[:, 2:2 + d])


@pytest.mark.parametrize('n', [1, 300])
@pytest.mark.parametrize('d', [1, 65])
def test_broadcast_rows_is_the_scaled_vector_repeated(pk, n, d):
    rng = np.random.default_rng(n + d)
    vec = rng.normal(size=d).astype(np.float32)
    for scale in (1.0, 0.3, -1.0 / 7):
        got = pk.ops.broadcast_rows(C(vec), n, scale)
        want = np.float32(scale) * vec
        assert want.dtype == np.float32 and got.shape == (n, d)
        assert np.array_equal(N(got), np.broadcast_to(want, (n, d)))
