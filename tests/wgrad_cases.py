"""Shared by tests/test_wgrad_host.py (no GPU) and tests/test_gpu_wgrad_edges.py (on the device): the weight gradient
dW[n][k] = sum_m g[m][n] [relu](x)[m][k], db[n] = sum_m g[m][n] at the edges of its launch plan -- a Python restatement of the
plan (occ4d::wgrad16_plan of csrc/wgrad16.hip and the generic branch of occ4d_linear_wgrad_workspace, csrc/backward.hip), the
case matrix with the edge each case exists for, the two kinds of input, the references and the derived bounds, and the column
sums of ops.colsum.  No GPU in here: the check_* functions take the package and a torch device.

Two kernels compute the weight gradient.  `w16` (wgrad16_kernel<4, RELU, BIAS>, csrc/wgrad16.hip) takes N % 416 == 0, K % 32 == 0,
K >= 64, M >= 4096: M is cut into `splits` slices of `mps` rows (a multiple of 16), slice z runs on XCD z % 8, a workgroup owns one
(slice, 416-row chunk of N, 64-column block of K), works in stages of 16 rows and leaves the M % 16 rows behind the last full stage
to tail_partial_kernel, whose partial is the (splits + 1)-th.  When K % 64 == 32 the last K column is shifted back to end at K
(k0 = K - 64) and does not store its first `kskip` = 32 columns.  A slice without a full stage stores zeros.  `gen1`
(wgrad_kernel<NT>, NT in {1, 2, 3, 5, 9, 13} by K) takes every other shape: 128 rows of N x 32 NT columns of K per workgroup, ragged
edges by clamped loads.  wgrad_reduce4_kernel (or the scalar wgrad_reduce_kernel when dW is not 16-byte aligned) sums the dW
partials and short_reduce_kernel the db partials; occ4d_colsum_f32 ends in the same short_reduce_kernel.

Inputs.  (a) `int`: g in [-3, 3], x in [-4, 4], integers; one column of x is <= 0 everywhere (under relu_x that column of dW is
exactly 0.0) and one column of g is zero.  Every product and every partial sum is an integer of magnitude <= 12 M < 2^24, so in
ANY summation order every fp32 operation is exact: dW and db must equal the integer reference bit for bit -- a dropped, duplicated
or mispaired row, column, tile or slice cannot hide under a tolerance.  (b) `real`: Gaussian, one column of g offset by +50 so
that one row of dW and one element of db is large and free of cancellation.

Bound for the real inputs (U = 2^-24; the argument is in the module docstring of tests/test_gpu_backward_edges.py): a fp32 sum of
L terms in any order is within (L - 1) U sum|term| of the exact sum, the rounded product adds 1, 2 is slack; here L <= M + splits
(the rows, then the partials of the slices), so per element

    |dW - ref| <= (M + splits + 3) U sum_m |g| |[relu] x|          |db - ref| <= (M + splits + 3) U sum_m |g|

and + U |base| when the call accumulates onto `base`.  ops.colsum: the same with L = n + chunks."""
import collections
import ctypes
import functools
import os
import zlib

import numpy as np
import torch

from forward_cases import F32, U, cdiv, host, within

SENTINEL = 0x7FA5C3D1          # a NaN bit pattern no kernel computes (tests/forward_cases.py)
POISON = F32(1e30)             # finite: a padding column read as data shows in every sum it enters
GUARD = 64                     # canary floats behind each buffer
WN, WBM = 416, 16              # csrc/wgrad16.hip: rows of an N chunk, rows of M per stage
PINNING_ENV = ('OCC4D_W16_ROUNDS', 'OCC4D_WGRAD_NARROW_WGS')


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def to_device(a, device):
    """Host array -> a fresh tensor on `device`, bits preserved (a copy: the cached inputs are read-only arrays)."""
    return torch.tensor(np.ascontiguousarray(a)).to(device)


def pinning_is_off():
    """The two environment switches that move the plan: with one of them set the pinned numbers do not apply."""
    return any(v in os.environ for v in PINNING_ENV)


# ---------------------------------------------------------------------------------------------------------------- the plan
Plan = collections.namedtuple('Plan', 'route splits mps floats empty min_stages tail ncol kskip nchunk nt kblocks')
Plan.__doc__ = """route: 'w16' | 'gen1'; splits, mps: M slices and rows per slice; floats: the workspace; empty: slices that hold no
row (w16: no full 16-row stage); min_stages: the fewest 16-row tiles in a slice that holds one (gen1 counts a ragged tile); tail:
M % 16; ncol, kskip, nchunk: the w16 grid (K column blocks of 64, columns the shifted last block leaves to its neighbour, N chunks
of 416) -- for gen1 the K and N block counts of its grid and 0; nt: gen1's column-tile count (w16: its NTB = 4); kblocks: K blocks."""


def w16_plan(M, N, K, rounds=3):
    """occ4d::wgrad16_plan: (splits, rows per slice) or None when the shape goes to the generic kernel."""
    if N % WN != 0 or K % 32 != 0 or K < 64 or M < 4096:
        return None
    cc = cdiv(K, 64) * (N // WN)
    cap = max(M // 512, 8)
    s, best = 8, -1.0
    for cand in range(8, cap + 1, 8):
        wgs = cand * cc
        r = cdiv(wgs, 512)
        if r > rounds:
            break
        fill = wgs / (512.0 * r)
        if fill > best + 1e-9:
            best, s = fill, cand
    return s, cdiv(cdiv(M, s), WBM) * WBM


def generic_nt(K):
    for limit, nt in ((32, 1), (64, 2), (96, 3), (160, 5), (288, 9)):
        if K <= limit:
            return nt
    return 13


def plan(M, N, K, rounds=3, narrow=2048):
    """occ4d_linear_wgrad_workspace + the slicing of the two kernels, restated (defaults: OCC4D_W16_ROUNDS 3,
    OCC4D_WGRAD_NARROW_WGS 2048)."""
    w16 = w16_plan(M, N, K, rounds)
    if w16 is not None:
        s, mps = w16
        m_full = M // WBM * WBM
        stages = [max(0, min(m_full, (z + 1) * mps) - z * mps) // WBM for z in range(s)]
        ncol = cdiv(K, 64)
        return Plan('w16', s, mps, (s + 1) * (N * K + N), sum(1 for v in stages if v == 0), min(v for v in stages if v > 0), M % WBM,
                    ncol, ncol * 64 - K, N // WN, 4, ncol)
    tiles = cdiv(N, 128) * cdiv(K, 416)
    s = max(1, min(cdiv(narrow if K <= 64 else 512, tiles), max(M // 256, 1)))
    mps = cdiv(cdiv(M, s), WBM) * WBM
    tiles_m = [cdiv(max(0, min(M, (z + 1) * mps) - z * mps), WBM) for z in range(s)]
    nt = generic_nt(K)
    return Plan('gen1', s, mps, s * (N * K + N), sum(1 for v in tiles_m if v == 0), min(v for v in tiles_m if v > 0), M % WBM,
                cdiv(K, 32 * nt), 0, cdiv(N, 128), nt, cdiv(K, 32 * nt))


def library_plan(pk, M, N, K):
    """(splits, floats) of occ4d_linear_wgrad_workspace: host arithmetic, no device needed."""
    splits, floats = ctypes.c_int(0), ctypes.c_int64(0)
    assert pk._lib.lib().occ4d_linear_wgrad_workspace(M, N, K, ctypes.byref(splits), ctypes.byref(floats)) == pk._lib.OK
    return splits.value, floats.value


# ---------------------------------------------------------------------------------------------------------------- the cases
Case = collections.namedtuple('Case', 'M N K edge holds')       # holds(plan) -> the edge the case exists for is still there


def _w16(M, N, K, edge, holds):
    return Case(M, N, K, edge, lambda p: p.route == 'w16' and holds(p))


def _gen(M, N, K, edge, holds):
    return Case(M, N, K, edge, lambda p: p.route == 'gen1' and holds(p))


W16_CASES = [
    _w16(4096, 416, 64, 'splits 8, no tail, one K column',
         lambda p: p.splits == 8 and p.tail == 0 and p.ncol == 1 and p.kskip == 0 and p.empty == 0),
    _w16(4112, 416, 416, "the decoder's own layer: 7 K columns, kskip 32", lambda p: p.ncol == 7 and p.kskip == 32 and p.tail == 0),
    _w16(4104, 832, 224, 'two N chunks, 4 K columns, kskip 32, 8 tail rows',
         lambda p: p.nchunk == 2 and p.ncol == 4 and p.kskip == 32 and p.tail == 8),
    _w16(8200, 416, 96, 'splits 16 (second XCD group), kskip 32, tail', lambda p: p.splits == 16 and p.kskip == 32 and p.tail == 8),
    _w16(16385, 416, 64, 'splits 32, the last non-empty slice has exactly one stage, 1 tail row',
         lambda p: p.splits == 32 and p.min_stages == 1 and p.empty == 0 and p.tail == 1),
    _w16(20488, 416, 96, 'splits 40, one empty slice with kskip 32, tail',
         lambda p: p.splits == 40 and p.empty == 1 and p.kskip == 32 and p.tail == 8),
    _w16(4100, 416, 832, '13 K columns, 4 tail rows', lambda p: p.ncol == 13 and p.kskip == 0 and p.tail == 4),
]
OFF_W16_CASES = [
    _gen(4095, 416, 64, 'one row short of the w16 route', lambda p: p.nt == 2),
    _gen(4096, 420, 64, 'N is not a multiple of 416', lambda p: p.nt == 2 and p.nchunk == 4),
    _gen(4096, 416, 36, 'K is not a multiple of 32', lambda p: p.nt == 2),
]
GEN_CASES = [
    _gen(17, 4, 4, 'NT 1, four live columns each way, one slice of two tiles', lambda p: p.nt == 1 and p.splits == 1 and p.min_stages == 2),
    _gen(300, 132, 32, 'NT 1 at its full width, two N blocks (the second 4 rows)', lambda p: p.nt == 1 and p.nchunk == 2),
    _gen(1000, 36, 36, 'NT 2 just above NT 1, three slices', lambda p: p.nt == 2 and p.splits == 3),
    _gen(255, 128, 64, 'NT 2 at its full width, a full N block, ragged last tile', lambda p: p.nt == 2 and p.tail == 15),
    _gen(16, 4, 68, 'NT 3 just above NT 2, one full tile', lambda p: p.nt == 3 and p.min_stages == 1 and p.tail == 0),
    _gen(15, 124, 96, 'NT 3 at its full width, one ragged tile', lambda p: p.nt == 3 and p.min_stages == 1),
    _gen(5003, 832, 100, 'NT 5 just above NT 3, 7 N blocks, 19 slices', lambda p: p.nt == 5 and p.nchunk == 7 and p.splits == 19),
    _gen(1, 36, 164, 'NT 9 just above NT 5, one row', lambda p: p.nt == 9 and p.splits == 1),
    _gen(255, 72, 288, 'NT 9 at its full width', lambda p: p.nt == 9 and p.kblocks == 1),
    _gen(1000, 124, 292, 'NT 13 just above NT 9', lambda p: p.nt == 13 and p.kblocks == 1),
    _gen(16, 4, 416, 'NT 13 at its full width', lambda p: p.nt == 13 and p.kblocks == 1),
    _gen(17, 260, 420, 'two K blocks, the second 4 columns wide', lambda p: p.nt == 13 and p.kblocks == 2 and p.nchunk == 3),
    _gen(4609, 128, 32, '18 slices, one of them empty', lambda p: p.nt == 1 and p.splits == 18 and p.empty == 1),
]
ALL_CASES = W16_CASES + OFF_W16_CASES + GEN_CASES
ALL_COMBOS = ((True, True), (True, False), (False, True), (False, False))          # (relu_x, bias)


def case_id(c):
    return '%d-%d-%d' % (c.M, c.N, c.K)


def combos(c):
    """Every (relu_x, bias) on the w16 route; both flags together and neither on the generic one."""
    return ALL_COMBOS if plan(c.M, c.N, c.K).route == 'w16' else ((True, True), (False, False))


def reached(c, relu_x, bias, aligned=True):
    """The kernels one call of the case launches (for the record the tests print)."""
    p = plan(c.M, c.N, c.K)
    first = ['wgrad16_kernel<4, %s, %s>' % (str(relu_x).lower(), str(bias).lower()), 'tail_partial_kernel'] if p.route == 'w16' \
        else ['wgrad_kernel<%d>' % p.nt]
    return first + ['wgrad_reduce4_kernel' if aligned else 'wgrad_reduce_kernel'] + (['short_reduce_kernel'] if bias else [])


# ---------------------------------------------------------------------------------------------------------------- inputs
def special_columns(N, K):
    """(the column of g that is zero / offset, the column of x that is <= 0): inside the last blocks of either kernel."""
    return max(0, N - 2), max(0, K - 3)


@functools.lru_cache(maxsize=6)
def inputs(M, N, K, kind):
    """(g (M, N), x (M, K)) float32, read-only.  kind 'int' | 'real' (module docstring)."""
    rng = _rng('wgrad', M, N, K, kind)
    gc, xc = special_columns(N, K)
    if kind == 'int':
        g = rng.integers(-3, 4, size=(M, N)).astype(F32)
        x = rng.integers(-4, 5, size=(M, K)).astype(F32)
        g[:, gc] = 0
        x[:, xc] = -np.abs(x[:, xc])
    else:
        g = rng.normal(size=(M, N)).astype(F32)
        x = rng.normal(size=(M, K)).astype(F32)
        g[:, gc] += F32(50)
    g.setflags(write=False)
    x.setflags(write=False)
    return g, x


Ref = collections.namedtuple('Ref', 'dw db mag_w mag_b')


@functools.lru_cache(maxsize=8)
def reference(M, N, K, kind, relu_x):
    """fp64 dW, db and the sums of |term| of the same float32 inputs.  For the integer inputs fp64 is exact (every partial sum is
    an integer below 2^53): the values are checked to be integers and returned as int64."""
    g, x = inputs(M, N, K, kind)
    g64 = g.astype(np.float64)
    a64 = np.maximum(x, 0).astype(np.float64) if relu_x else x.astype(np.float64)
    dw, db = g64.T @ a64, g64.sum(axis=0)
    mag_w, mag_b = np.abs(g64).T @ np.abs(a64), np.abs(g64).sum(axis=0)
    if kind == 'int':
        assert np.array_equal(dw, np.rint(dw)) and np.array_equal(db, np.rint(db))
        dw, db = dw.astype(np.int64), db.astype(np.int64)
    return Ref(dw, db, mag_w, mag_b)


def integer_headroom(M):
    """The largest magnitude a partial sum of the integer inputs can reach (|g| <= 3, |x| <= 4): < 2^24 keeps fp32 exact."""
    return 12 * M


def bounds(M, splits, ref, base_w=None, base_b=None):
    """(bound of dW, bound of db) per element."""
    f = (M + splits + 3) * U
    bw, bb = f * ref.mag_w, f * ref.mag_b
    if base_w is not None:
        bw = bw + U * np.abs(base_w)
    if base_b is not None:
        bb = bb + U * np.abs(base_b)
    return bw, bb


def same_bits(got, want_int, what):
    """float32 `got` equals the integer array `want_int`, bit for bit (an exact zero is +0.0)."""
    got = np.asarray(got)
    want = want_int.astype(F32)
    assert np.array_equal(want.astype(np.int64), want_int), what + ': the reference does not fit float32'
    assert got.dtype == F32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = got.view(np.int32) != want.view(np.int32)
    if bad.any():
        at = np.unravel_index(np.argmax(bad), bad.shape)
        raise AssertionError('%s: %d of %d elements differ from the integer reference; first at %s: got %r, want %r'
                             % (what, int(bad.sum()), bad.size, at, got[at], want[at]))


# ---------------------------------------------------------------------------------------------------------------- through ops
def run_ops(pk, g, x, relu_x, bias):
    res = pk.ops.linear_wgrad(g, x, bias=bias, relu_x=relu_x)
    dw, db = res if bias else (res, None)
    return host(dw), None if db is None else host(db)


def check_exact(pk, device, c):
    """Integer inputs through ops.linear_wgrad: the integer reference bit for bit, twice the same bits, the relu column and the
    zero column of g exactly 0.0."""
    g, x = (to_device(a, device) for a in inputs(c.M, c.N, c.K, 'int'))
    gc, xc = special_columns(c.N, c.K)
    for relu_x, bias in combos(c):
        what = 'int %s relu_x=%s bias=%s' % (case_id(c), relu_x, bias)
        ref = reference(c.M, c.N, c.K, 'int', relu_x)
        dw, db = run_ops(pk, g, x, relu_x, bias)
        same_bits(dw, ref.dw, what + ' dW')
        assert not dw[gc].any() and (not relu_x or not dw[:, xc].any()), what
        if bias:
            same_bits(db, ref.db, what + ' db')
        again = run_ops(pk, g, x, relu_x, bias)
        assert np.array_equal(again[0].view(np.int32), dw.view(np.int32)), what + ': not the same bits twice'
        assert not bias or np.array_equal(again[1].view(np.int32), db.view(np.int32)), what + ': not the same bits twice'


def check_real(pk, device, c):
    """Real inputs through ops.linear_wgrad within the derived bound -> the worst error / bound."""
    g, x = (to_device(a, device) for a in inputs(c.M, c.N, c.K, 'real'))
    splits, _ = library_plan(pk, c.M, c.N, c.K)                           # (the split in force, whatever the environment says)
    worst = 0.0
    for relu_x, bias in combos(c):
        what = 'real %s relu_x=%s bias=%s' % (case_id(c), relu_x, bias)
        ref = reference(c.M, c.N, c.K, 'real', relu_x)
        bw, bb = bounds(c.M, splits, ref)
        dw, db = run_ops(pk, g, x, relu_x, bias)
        worst = max(worst, within(dw, ref.dw, bw, what + ' dW'))
        if bias:
            worst = max(worst, within(db, ref.db, bb, what + ' db'))
    return worst


# ---------------------------------------------------------------------------------------------------------------- through the C ABI
def sentinel(n):
    return np.full((n,), SENTINEL, dtype=np.int32).view(F32)


def guard_intact(t, used, what):
    """The floats of the 1-D device buffer `t` from `used` on still hold the sentinel."""
    bits = host(t.view(torch.int32))[used:]
    assert bits.size >= GUARD and np.all(bits == SENTINEL), '%s: %d canary floats were written' % (what, int((bits != SENTINEL).sum()))


class Abi:
    """One case's operands laid out for a direct call of occ4d_linear_wgrad_bias_f32: g and x as the first N / K columns of
    (M, ldg) / (M, ldx) buffers whose padding columns hold POISON; a workspace of exactly the floats the plan asks for, all of it
    (and GUARD floats behind it) the NaN sentinel, so that a partial nobody wrote shows in dW; dW and db buffers with GUARD floats
    behind them and `dw_off` floats (0 or 1: 1 takes dW off 16-byte alignment) in front."""

    def __init__(self, pk, device, c, kind='int', pad_g=0, pad_x=0, dw_off=0):
        self.pk, self.c, self.kind = pk, c, kind
        M, N, K = c.M, c.N, c.K
        g, x = inputs(M, N, K, kind)
        self.ldg, self.ldx, self.dw_off = N + pad_g, K + pad_x, dw_off
        gb, xb = np.full((M, self.ldg), POISON, F32), np.full((M, self.ldx), POISON, F32)
        gb[:, :N], xb[:, :K] = g, x
        self.g, self.x = to_device(gb, device), to_device(xb, device)
        self.splits, self.floats = library_plan(pk, M, N, K)
        self.ws = to_device(sentinel(self.floats + GUARD), device)
        self.dw = to_device(sentinel(dw_off + N * K + GUARD), device)
        self.db = to_device(sentinel(N + GUARD), device)
        assert self.g.data_ptr() % 16 == 0 and self.x.data_ptr() % 16 == 0 and self.dw.data_ptr() % 16 == 0 and self.ws.data_ptr() % 16 == 0

    def seed(self, base_w, base_b):
        N, K = self.c.N, self.c.K
        self.dw[self.dw_off:self.dw_off + N * K] = to_device(base_w.astype(F32).reshape(-1), self.dw.device)
        self.db[:N] = to_device(base_b.astype(F32), self.db.device)

    def call(self, relu_x, bias, accumulate, **over):
        """-> the return code.  `over`: arguments replaced for one call (M, N, K, ldg, ldx, splits; g, x, dw, db, ws as ctypes
        pointers)."""
        ops, c = self.pk.ops, self.c
        a = dict(g=ops._ptr(self.g), ldg=self.ldg, x=ops._ptr(self.x), ldx=self.ldx, M=c.M, N=c.N, K=c.K,
                 dw=ctypes.c_void_p(self.dw.data_ptr() + 4 * self.dw_off), db=ops._ptr(self.db) if bias else ctypes.c_void_p(0),
                 ws=ops._ptr(self.ws), splits=self.splits)
        a.update(over)
        return self.pk._lib.lib().occ4d_linear_wgrad_bias_f32(a['g'], a['ldg'], a['x'], a['ldx'], a['M'], a['N'], a['K'], int(relu_x),
                                                              a['dw'], a['db'], int(accumulate), a['ws'], a['splits'], ops._stream())

    def results(self):
        N, K = self.c.N, self.c.K
        return host(self.dw)[self.dw_off:self.dw_off + N * K].reshape(N, K), host(self.db)[:N]

    def guards_intact(self, what, db_written=True):
        N, K = self.c.N, self.c.K
        guard_intact(self.ws, self.floats, what + ' workspace')
        guard_intact(self.dw, self.dw_off + N * K, what + ' dW')
        guard_intact(self.db, N if db_written else 0, what + ' db')
        if self.dw_off:
            assert np.all(host(self.dw.view(torch.int32))[:self.dw_off] == SENTINEL), what + ': the floats in front of dW were written'

    def untouched(self, what):
        """Nothing at all was written: a rejected call."""
        for name, t in (('workspace', self.ws), ('dW', self.dw), ('db', self.db)):
            guard_intact(t, 0, '%s %s' % (what, name))


def check_abi(pk, device, c, relu_x=True, bias=True, accumulate=False, pad_g=0, pad_x=0, dw_off=0):
    """One direct call on the integer inputs: return code OK, dW (and db) the integer reference (+ the integer base under
    accumulate) bit for bit, every canary intact."""
    what = 'abi %s relu_x=%s bias=%s accumulate=%s ldg=N+%d ldx=K+%d dw_off=%d' % (case_id(c), relu_x, bias, accumulate, pad_g, pad_x, dw_off)
    a = Abi(pk, device, c, 'int', pad_g, pad_x, dw_off)
    ref = reference(c.M, c.N, c.K, 'int', relu_x)
    want_w, want_b = ref.dw, ref.db
    if accumulate:
        rng = _rng('base', case_id(c))
        base_w, base_b = rng.integers(-1000, 1001, size=(c.N, c.K)), rng.integers(-1000, 1001, size=(c.N,))
        assert integer_headroom(c.M) + 1000 < 2 ** 24
        a.seed(base_w, base_b)
        want_w, want_b = want_w + base_w, want_b + base_b
    assert a.call(relu_x, bias, accumulate) == pk._lib.OK, what
    dw, db = a.results()
    same_bits(dw, want_w, what + ' dW')
    if bias:
        same_bits(db, want_b, what + ' db')
    a.guards_intact(what, db_written=bias)


# ---------------------------------------------------------------------------------------------------------------- column sums
COLSUM_CHUNKS = (1, 3, 4, 5, 28, 29, 32, 33, 36, 512)          # both sides of short_reduce_kernel's 8-deep loop (z + 28 < chunks)
COLSUM_WIDTHS = (1, 63, 65)                                    # one partial 64-column strip; a full one and one live column


def colsum_rows(chunks):
    """n = 256 chunks + r: r = 1 (at 512 chunks the last chunk is empty and the one before holds 3 rows) and r = 255."""
    return (256 * chunks + 1, 256 * chunks + 255)


def colsum_chunks(n):
    """ops.colsum: (chunks, rows per chunk, empty chunks)."""
    chunks = max(1, min(512, n // 256))
    rpc = cdiv(n, chunks)
    return chunks, rpc, sum(1 for z in range(chunks) if z * rpc >= n)


@functools.lru_cache(maxsize=4)
def colsum_inputs(n, d, kind):
    rng = _rng('colsum', n, d, kind)
    if kind == 'int':
        x = rng.integers(-4, 5, size=(n, d)).astype(F32)
        x[:, d // 2] = -np.abs(x[:, d // 2])
    else:
        x = rng.normal(size=(n, d)).astype(F32)
        x[:, d // 2] += F32(50)
    x.setflags(write=False)
    return x


def check_colsum(pk, device, n, d):
    """ops.colsum: the integer inputs (as a column slice of a wider buffer whose other columns hold POISON) bit for bit, the real
    inputs within (n + chunks + 3) U sum|x| -> the worst error / bound."""
    chunks, _, _ = colsum_chunks(n)
    assert 4 * n < 2 ** 24
    x = colsum_inputs(n, d, 'int')
    buf = np.full((n, d + 3), POISON, F32)
    buf[:, 2:2 + d] = x
    view = to_device(buf, device)[:, 2:2 + d]
    assert view.stride(0) == d + 3
    got = host(pk.ops.colsum(view))
    same_bits(got, x.astype(np.int64).sum(axis=0), 'colsum int n=%d d=%d' % (n, d))
    assert np.array_equal(host(pk.ops.colsum(view)).view(np.int32), got.view(np.int32))
    x = colsum_inputs(n, d, 'real')
    x64 = x.astype(np.float64)
    return within(host(pk.ops.colsum(to_device(x, device))), x64.sum(axis=0), (n + chunks + 3) * U * np.abs(x64).sum(axis=0),
                  'colsum real n=%d d=%d' % (n, d))
