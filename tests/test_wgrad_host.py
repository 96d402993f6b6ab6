"""No GPU: what tests/test_gpu_wgrad_edges.py rests on, checked on the host first.  The restated launch plan of the weight
gradient reproduces the table the cases were chosen from and equals occ4d_linear_wgrad_workspace (host arithmetic: the library
answers without a device); every case still sits on the edge it is named for, and the restatement is tied to the source text; the
integer inputs keep every partial sum below 2^24 and carry their two special columns; the references hold their own bounds -- a
float32 sum of the real inputs in four different orders stays inside the bound the kernels are held to, and the helpers reject
a result off by one part in 10^4 (at M = 1000, where the bound is 6 parts in 10^5), one row left out, one changed integer, a
negative zero, a NaN and one written canary."""
import numpy as np
import pytest

import occlusions4d_amd as pk
import wgrad_cases as wc

F32, U = wc.F32, wc.U

# (M, N, K): route, splits, rows per slice, empty slices, fewest stages, tail rows, ncol, kskip, nchunk, NT, K blocks
TABLE = {
    (4096, 416, 64): ('w16', 8, 512, 0, 32, 0, 1, 0, 1, 4, 1),
    (4112, 416, 416): ('w16', 8, 528, 0, 26, 0, 7, 32, 1, 4, 7),
    (4104, 832, 224): ('w16', 8, 528, 0, 25, 8, 4, 32, 2, 4, 4),
    (8200, 416, 96): ('w16', 16, 528, 0, 17, 8, 2, 32, 1, 4, 2),
    (16385, 416, 64): ('w16', 32, 528, 0, 1, 1, 1, 0, 1, 4, 1),
    (20488, 416, 96): ('w16', 40, 528, 1, 26, 8, 2, 32, 1, 4, 2),
    (4100, 416, 832): ('w16', 8, 528, 0, 25, 4, 13, 0, 1, 4, 13),
    (4095, 416, 64): ('gen1', 15, 288, 0, 4, 15, 1, 0, 4, 2, 1),
    (4096, 420, 64): ('gen1', 16, 256, 0, 16, 0, 1, 0, 4, 2, 1),
    (4096, 416, 36): ('gen1', 16, 256, 0, 16, 0, 1, 0, 4, 2, 1),
    (17, 4, 4): ('gen1', 1, 32, 0, 2, 1, 1, 0, 1, 1, 1),
    (300, 132, 32): ('gen1', 1, 304, 0, 19, 12, 1, 0, 2, 1, 1),
    (1000, 36, 36): ('gen1', 3, 336, 0, 21, 8, 1, 0, 1, 2, 1),
    (255, 128, 64): ('gen1', 1, 256, 0, 16, 15, 1, 0, 1, 2, 1),
    (16, 4, 68): ('gen1', 1, 16, 0, 1, 0, 1, 0, 1, 3, 1),
    (15, 124, 96): ('gen1', 1, 16, 0, 1, 15, 1, 0, 1, 3, 1),
    (5003, 832, 100): ('gen1', 19, 272, 0, 7, 11, 1, 0, 7, 5, 1),
    (1, 36, 164): ('gen1', 1, 16, 0, 1, 1, 1, 0, 1, 9, 1),
    (255, 72, 288): ('gen1', 1, 256, 0, 16, 15, 1, 0, 1, 9, 1),
    (1000, 124, 292): ('gen1', 3, 336, 0, 21, 8, 1, 0, 1, 13, 1),
    (16, 4, 416): ('gen1', 1, 16, 0, 1, 0, 1, 0, 1, 13, 1),
    (17, 260, 420): ('gen1', 1, 32, 0, 2, 1, 2, 0, 3, 13, 2),
    (4609, 128, 32): ('gen1', 18, 272, 1, 17, 1, 1, 0, 1, 1, 1),
}


# ---------------------------------------------------------------------------------------------------------------- the plan
def test_the_restated_plan_reproduces_the_table():
    assert {(c.M, c.N, c.K) for c in wc.ALL_CASES} == set(TABLE) and len(wc.ALL_CASES) == len(TABLE) == 23
    for c in wc.ALL_CASES:
        p = wc.plan(c.M, c.N, c.K)
        route, splits, mps, empty, stages, tail, ncol, kskip, nchunk, nt, kblocks = TABLE[(c.M, c.N, c.K)]
        assert (p.route, p.splits, p.mps, p.empty, p.min_stages, p.tail, p.ncol, p.kskip, p.nchunk, p.nt, p.kblocks) == \
            (route, splits, mps, empty, stages, tail, ncol, kskip, nchunk, nt, kblocks), (wc.case_id(c), p)
        per = c.N * c.K + c.N
        assert p.floats == ((splits + 1) * per if route == 'w16' else splits * per)
        assert p.mps % 16 == 0 and p.splits * p.mps >= c.M and (route != 'w16' or splits % 8 == 0)
    assert [wc.plan(c.M, c.N, c.K).route for c in wc.W16_CASES] == ['w16'] * 7
    assert [wc.plan(c.M, c.N, c.K).route for c in wc.OFF_W16_CASES + wc.GEN_CASES] == ['gen1'] * 16


def test_every_case_sits_on_the_edge_it_is_named_for():
    for c in wc.ALL_CASES:
        assert c.edge and c.holds(wc.plan(c.M, c.N, c.K)), (wc.case_id(c), c.edge)
    # ... and a plan that moved would be noticed: another fill rule, another narrow target
    moved = [c for c in wc.W16_CASES if not c.holds(wc.plan(c.M, c.N, c.K, rounds=1)._replace(splits=8))]
    assert {wc.case_id(c) for c in moved} >= {'8200-416-96', '16385-416-64', '20488-416-96'}
    assert not wc.GEN_CASES[-1].holds(wc.plan(4609, 128, 32, narrow=8))
    # the edges the matrix is there for, over all cases
    w16 = [wc.plan(c.M, c.N, c.K) for c in wc.W16_CASES]
    assert {p.splits for p in w16} == {8, 16, 32, 40} and {p.kskip for p in w16} == {0, 32} and {p.nchunk for p in w16} == {1, 2}
    assert {p.ncol for p in w16} == {1, 2, 4, 7, 13} and {p.tail for p in w16} == {0, 1, 4, 8}
    assert any(p.empty and p.kskip for p in w16) and any(p.min_stages == 1 for p in w16)
    gen = [wc.plan(c.M, c.N, c.K) for c in wc.OFF_W16_CASES + wc.GEN_CASES]
    assert {p.nt for p in gen} == {1, 2, 3, 5, 9, 13} and any(p.empty for p in gen) and any(p.kblocks == 2 for p in gen)
    ks = {c.K for c in wc.GEN_CASES}
    for below, limit in ((0, 32), (32, 64), (64, 96), (96, 160), (160, 288)):   # K inside every NT's range and just above its limit
        assert any(below < k <= limit for k in ks) and any(limit < k <= limit + 4 for k in ks), limit
    assert {32, 64, 96, 288, 416} <= ks and any(k > 416 for k in ks)           # ... and at the full width of NT 1, 2, 3, 9, 13
    assert max(c.M * max(c.N, c.K) for c in wc.ALL_CASES) == 20488 * 416


def test_the_restated_plan_is_the_one_in_the_source():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'occlusions-4d_amd', 'csrc', 'wgrad16.hip')) as f:
        w16 = f.read()
    with open(os.path.join(root, 'occlusions-4d_amd', 'csrc', 'backward.hip')) as f:
        bwd = f.read()
    for text in ('constexpr int WN = 416;', 'constexpr int WBM = 16;', 'if (N % WN != 0 || K % 32 != 0 || K < 64 || M < 4096) return false;',
                 'return e ? atoi(e) : 3; }();', 'const int cap = M / 512 > 8 ? M / 512 : 8;', 'for (int cand = 8; cand <= cap; cand += 8) {',
                 'if (rounds > max_rounds) break;', 'if (fill > best + 1e-9) { best = fill; s = cand; }',
                 'int mps = cdiv(cdiv(M, s), WBM) * WBM;', 'const int k0 = min(col * 64, a.K - 64), kskip = col * 64 - k0;',
                 'const int z = (j / cc_n) * 8 + xcd;', 'const int m_full = M / WBM * WBM;'):
        assert text in w16, 'csrc/wgrad16.hip no longer says: ' + text
    for text in ('*floats_out = (int64_t)(s16 + 1) * N * K + (int64_t)(s16 + 1) * N;',
                 'const int tiles = occ4d::cdiv(N, 128) * occ4d::cdiv(K, 416);', 'return e ? atoi(e) : 2048; }();',
                 'int splits = occ4d::cdiv(K <= 64 ? narrow_target : 512, tiles);', 'const int cap = M / 256 > 1 ? M / 256 : 1;',
                 '*floats_out = (int64_t)(*splits_out) * N * K + (int64_t)(*splits_out) * N;',
                 'const int mps = occ4d::cdiv(occ4d::cdiv(M, splits), WG_BM) * WG_BM;', 'if (K <= 32) OCC4D_WGRAD(1);',
                 'else if (K <= 64) OCC4D_WGRAD(2);', 'else if (K <= 96) OCC4D_WGRAD(3);', 'else if (K <= 160) OCC4D_WGRAD(5);',
                 'else if (K <= 288) OCC4D_WGRAD(9);', 'else OCC4D_WGRAD(13);', 'for (; z + 28 < splits; z += 32) {'):
        assert text in bwd, 'csrc/backward.hip no longer says: ' + text


@pytest.mark.skipif(wc.pinning_is_off(), reason='OCC4D_W16_ROUNDS / OCC4D_WGRAD_NARROW_WGS move the plan')
def test_the_library_plans_what_the_restatement_says():
    """occ4d_linear_wgrad_workspace on the host, over the cases and a sweep around every threshold of the plan."""
    shapes = [(c.M, c.N, c.K) for c in wc.ALL_CASES]
    shapes += [(M, N, K) for M in (1, 255, 256, 4095, 4096, 8191, 8192, 12288, 40000, 68812, 458752) for N in (4, 128, 132, 416, 832, 1248)
               for K in (4, 32, 36, 64, 96, 100, 160, 288, 416, 420, 704, 832)]
    routes = set()
    for M, N, K in shapes:
        p = wc.plan(M, N, K)
        assert wc.library_plan(pk, M, N, K) == (p.splits, p.floats), (M, N, K, p)
        routes.add(p.route)
    assert routes == {'w16', 'gen1'}


# ---------------------------------------------------------------------------------------------------------------- inputs
def test_integer_inputs_have_headroom_and_their_special_columns():
    assert max(wc.integer_headroom(c.M) for c in wc.ALL_CASES) == 12 * 20488 < 2 ** 24
    assert 12 * 20488 + 1000 < 2 ** 24                                       # ... and under the integer base of the accumulate calls
    for n in (256 * c + r for c in wc.COLSUM_CHUNKS for r in (1, 255)):
        assert 4 * n < 2 ** 24
    for c in wc.ALL_CASES:
        g, x = wc.inputs(c.M, c.N, c.K, 'int')
        gc, xc = wc.special_columns(c.N, c.K)
        assert g.dtype == F32 and x.dtype == F32 and g.shape == (c.M, c.N) and x.shape == (c.M, c.K)
        assert np.array_equal(g, np.rint(g)) and np.array_equal(x, np.rint(x)) and np.abs(g).max() <= 3 and np.abs(x).max() <= 4
        assert not g[:, gc].any() and x[:, xc].max() <= 0
        for relu_x in (False, True):
            ref = wc.reference(c.M, c.N, c.K, 'int', relu_x)
            assert ref.dw.dtype == np.int64 and ref.db.dtype == np.int64
            assert ref.mag_w.max() <= wc.integer_headroom(c.M) and ref.mag_b.max() <= 3 * c.M
            assert not ref.dw[gc].any() and ref.db[gc] == 0 and (not relu_x or not ref.dw[:, xc].any())
        if c.M >= 16 and c.N * c.K >= 16:
            assert wc.reference(c.M, c.N, c.K, 'int', False).dw[:, xc].any()  # (only the relu zeroes that column)
    # the float64 product the reference uses against plain int64 arithmetic
    g, x = wc.inputs(300, 132, 32, 'int')
    ref = wc.reference(300, 132, 32, 'int', True)
    assert np.array_equal(ref.dw, g.astype(np.int64).T @ np.maximum(x, 0).astype(np.int64))
    assert np.array_equal(ref.db, g.astype(np.int64).sum(axis=0))


def test_real_inputs_have_one_cancellation_free_column():
    for c in (wc.W16_CASES[0], wc.GEN_CASES[2]):
        g, _ = wc.inputs(c.M, c.N, c.K, 'real')
        gc, _ = wc.special_columns(c.N, c.K)
        ref = wc.reference(c.M, c.N, c.K, 'real', True)
        assert g[:, gc].min() > 40 and ref.db[gc] == ref.mag_b[gc] and np.allclose(ref.dw[gc], ref.mag_w[gc])
        assert np.abs(ref.db).argmax() == gc


# ---------------------------------------------------------------------------------------------------------------- bounds
def _orders(c, relu_x):
    """float32 dW, db of the real inputs in four orders: numpy's blocked product; the rows reversed; the kernel's slicing (one
    float32 product per M slice, the partials added in slice order); a plain row-by-row accumulation (small cases only)."""
    g, x = wc.inputs(c.M, c.N, c.K, 'real')
    a = np.maximum(x, F32(0)) if relu_x else x
    p = wc.plan(c.M, c.N, c.K)
    yield 'blocked', g.T @ a, g.sum(axis=0, dtype=F32)
    gr, ar = np.ascontiguousarray(g[::-1]), np.ascontiguousarray(a[::-1])          # (a copy: negative strides leave the BLAS path)
    yield 'reversed', gr.T @ ar, gr.sum(axis=0, dtype=F32)
    dw, db = np.zeros((c.N, c.K), F32), np.zeros((c.N,), F32)
    for z in range(p.splits):
        rows = slice(z * p.mps, min(c.M, (z + 1) * p.mps))
        dw, db = dw + g[rows].T @ a[rows], db + g[rows].sum(axis=0, dtype=F32)
    yield 'slices', dw, db
    if c.M * c.N * c.K <= 1000 * 124 * 292:
        dw, db = np.zeros((c.N, c.K), F32), np.zeros((c.N,), F32)
        for m in range(c.M):
            dw, db = dw + g[m][:, None] * a[m][None, :], db + g[m]
        yield 'serial', dw, db


def test_float32_sums_in_several_orders_hold_the_bound():
    worst, differ = {}, 0
    for c in wc.ALL_CASES:
        p = wc.plan(c.M, c.N, c.K)
        for relu_x in (True, False):
            ref = wc.reference(c.M, c.N, c.K, 'real', relu_x)
            bw, bb = wc.bounds(c.M, p.splits, ref)
            got = list(_orders(c, relu_x))
            for name, dw, db in got:
                assert dw.dtype == F32 and db.dtype == F32
                r = max(wc.within(dw, ref.dw, bw, '%s %s dW' % (name, wc.case_id(c))), wc.within(db, ref.db, bb, '%s %s db' % (name, wc.case_id(c))))
                worst[p.route] = max(worst.get(p.route, 0.0), r)
            differ += not np.array_equal(got[0][1], got[2][1])
    assert differ > len(wc.ALL_CASES)                                         # (the orders are different computations)
    print('\n[wgrad] float32 restatements, worst error / bound: %s' % ', '.join('%s %.4f' % kv for kv in sorted(worst.items())))
    assert max(worst.values()) <= 1.0
    for n, d in ((256 * 512 + 1, 65), (256 * 29 + 255, 63), (257, 1)):
        x = wc.colsum_inputs(n, d, 'real')
        chunks, rpc, _ = wc.colsum_chunks(n)
        x64 = x.astype(np.float64)
        bound = (n + chunks + 3) * U * np.abs(x64).sum(axis=0)
        parts = np.zeros((d,), F32)
        for z in range(chunks):
            parts = parts + x[z * rpc:(z + 1) * rpc].sum(axis=0, dtype=F32)
        for got in (x.sum(axis=0, dtype=F32), x[::-1].sum(axis=0, dtype=F32), parts):
            assert wc.within(got, x64.sum(axis=0), bound, 'colsum %d %d' % (n, d)) <= 1.0


def test_the_checks_reject_small_faults():
    c = wc.GEN_CASES[2]                                                       # (1000, 36, 36)
    p = wc.plan(c.M, c.N, c.K)
    ref = wc.reference(c.M, c.N, c.K, 'real', True)
    bw, bb = wc.bounds(c.M, p.splits, ref)
    assert wc.within(ref.dw.astype(F32), ref.dw, bw) <= 0.01 and wc.within(ref.db.astype(F32), ref.db, bb) <= 0.01
    gc, _ = wc.special_columns(c.N, c.K)
    for scale in (1 + 1e-4, 1 - 1e-4):                                        # (the bound at M = 1000 is 6e-5 of sum|term|)
        with pytest.raises(AssertionError, match='outside the bound'):
            wc.within((ref.dw * scale).astype(F32), ref.dw, bw)
        with pytest.raises(AssertionError, match='outside the bound'):
            wc.within((ref.db * scale).astype(F32), ref.db, bb)
    # one row of M left out of one element: far outside
    g, x = wc.inputs(c.M, c.N, c.K, 'real')
    off = ref.dw.copy()
    off[gc, 0] -= float(g[-1, gc]) * max(float(x[-1, 0]), 0.0) or 50.0
    with pytest.raises(AssertionError, match='outside the bound'):
        wc.within(off.astype(F32), ref.dw, bw)
    # under accumulate the base's own rounding is allowed, not more
    base = np.full((c.N, c.K), 1e6)
    assert np.array_equal(wc.bounds(c.M, p.splits, ref, base_w=base)[0], bw + U * 1e6)
    # the integer comparison: one unit in one element, a negative zero, a NaN nobody wrote
    iref = wc.reference(c.M, c.N, c.K, 'int', True)
    good = iref.dw.astype(F32)
    wc.same_bits(good, iref.dw, 'good')
    for at, value in (((5, 7), good[5, 7] + 1), ((gc, 0), F32(-0.0)), ((0, 0), wc.sentinel(1)[0])):
        bad = good.copy()
        bad[at] = value
        with pytest.raises(AssertionError, match='differ from the integer reference'):
            wc.same_bits(bad, iref.dw, 'bad')
    # a canary
    import torch
    t = torch.from_numpy(wc.sentinel(10 + wc.GUARD).copy())
    wc.guard_intact(t, 10, 'fresh')
    t[10 + 3] = 0.0
    with pytest.raises(AssertionError, match='canary'):
        wc.guard_intact(t, 10, 'written')


def test_reached_kernels_cover_every_instantiation_and_reduce():
    seen = set()
    for c in wc.ALL_CASES:
        for relu_x, bias in wc.combos(c):
            seen.update(wc.reached(c, relu_x, bias))
    seen.update(wc.reached(wc.W16_CASES[0], True, True, aligned=False))
    want = {'wgrad16_kernel<4, %s, %s>' % (r, b) for r in ('true', 'false') for b in ('true', 'false')}
    want |= {'wgrad_kernel<%d>' % nt for nt in (1, 2, 3, 5, 9, 13)}
    want |= {'tail_partial_kernel', 'wgrad_reduce4_kernel', 'wgrad_reduce_kernel', 'short_reduce_kernel'}
    assert seen == want
    for c in wc.ALL_CASES:
        p = wc.plan(c.M, c.N, c.K)
        print('[wgrad] %-14s %-4s splits %2d: %s -- %s' % (wc.case_id(c), p.route, p.splits, wc.reached(c, True, True)[0], c.edge))
    # the column sums: wave w of short_reduce_kernel runs its 8-deep loop while z + 28 < chunks, z = w, w + 32, ...: no wave at
    # 28 chunks, wave 0 alone at 29, all four at 32, wave 0 with a remainder at 33, all with one at 36, 16 rounds at 512
    def deep(chunks):
        return [sum(1 for z in range(w, chunks, 32) if z + 28 < chunks) for w in range(4)]
    assert deep(28) == [0] * 4 and deep(29) == [1, 0, 0, 0] and deep(32) == [1] * 4 and deep(36) == [1] * 4 and deep(512) == [16] * 4
    assert max(max(deep(c)) for c in (1, 3, 4, 5)) == 0
    for chunks in wc.COLSUM_CHUNKS:
        for n in wc.colsum_rows(chunks):
            assert wc.colsum_chunks(n)[0] == chunks
    assert wc.colsum_chunks(256 * 512 + 1) == (512, 257, 1) and 256 * 512 + 1 - 510 * 257 == 3
