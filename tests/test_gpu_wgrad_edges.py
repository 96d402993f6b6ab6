"""GPU: the weight-gradient GEMMs (wgrad16_kernel of csrc/wgrad16.hip, wgrad_kernel<NT> of csrc/backward.hip) and the reduce
kernels behind them at the edges of their launch plan -- the smallest shapes at which each path exists, named in
tests/wgrad_cases.py and pinned against occ4d_linear_wgrad_workspace, so that a change of the fill heuristic fails a case
loudly instead of sliding it off its edge.  Every case runs twice: integer inputs whose every partial sum is exact in fp32, so
dW and db must equal the integer reference BIT FOR BIT (a dropped, duplicated or mispaired row, column, tile or slice cannot
hide), and real inputs against fp64 element by element within (M + splits + 3) 2^-24 sum|term| (derived in
tests/wgrad_cases.py, proved on the references by tests/test_wgrad_host.py).  Then the C ABI directly: row strides above the
widths with poisoned padding, accumulate together with the bias gradient, an unaligned dW (the scalar reduce), a NaN-filled
workspace with canaries behind it (the zero-fill of an empty slice), the argument contract; the column sums of ops.colsum
across short_reduce_kernel's unrolled loop; and the autograd nodes at n = 4112, where they take rowlin and the w16 route.

Worst error / bound measured on the MI355X (every case prints its own): w16 0.0015 (4100-416-832; the bound grows with M, the
error with sqrt(M)), gen1 0.198 (17-260-420), accumulate 0.013, colsum 0.0047.  The integer inputs are what makes a fault in a
few elements visible at these M.  Autograd nodes against fp64: at most 5.7e-7 of the 2e-5 allowed.

Mutation check (on scratch copies of the two sources, not kept), four in-bounds faults in one library: the bias sum of
wgrad16_kernel<4, true, true> alone skipping one tile row in one of four steps; the zero-fill of an empty slice leaving out one
column of dW and one element of db; the scalar wgrad_reduce_kernel dropping its last remainder partial.  26 tests of this file
fail -- every w16 case on db under (relu, bias) with integer and real inputs, the NaN-workspace calls of 20488-416-96 on dW
(through ops.linear_wgrad the same fault read allocator memory that happened to be clean), the unaligned-dW calls alone for the
scalar reduce, the autograd test on db -- while test_weight_gradient_random, test_weight_gradient_training_shapes,
test_short_vector_reduce_of_the_bias_gradient, test_linear_backward, the residual-block test and test_decoder_gradients all pass."""
import ctypes

import numpy as np
import pytest
import torch

import wgrad_cases as wc
from grad_checks import rel_err

pytestmark = pytest.mark.gpu

DEV = 'cuda'
W16 = {wc.case_id(c): c for c in wc.W16_CASES}
GEN = {wc.case_id(c): c for c in wc.OFF_W16_CASES + wc.GEN_CASES}


@pytest.fixture(scope='module')
def pk():
    import occlusions4d_amd
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    occlusions4d_amd._lib.lib()
    return occlusions4d_amd


# ---------------------------------------------------------------------------------------------------------------- 1. the plan
@pytest.mark.skipif(wc.pinning_is_off(), reason='OCC4D_W16_ROUNDS / OCC4D_WGRAD_NARROW_WGS move the plan')
@pytest.mark.parametrize('case', wc.ALL_CASES, ids=wc.case_id)
def test_the_plan_is_pinned_and_the_case_is_on_its_edge(pk, case):
    p = wc.plan(case.M, case.N, case.K)
    splits, floats = wc.library_plan(pk, case.M, case.N, case.K)
    assert (splits, floats) == (p.splits, p.floats), (wc.case_id(case), p)
    per = case.N * case.K + case.N
    assert floats == ((splits + 1) * per if p.route == 'w16' else splits * per)
    assert case.holds(p), '%s is no longer on its edge (%s): %s' % (wc.case_id(case), case.edge, p)


# ---------------------------------------------------------------------------------------------------------------- 2, 3. the cases
@pytest.mark.parametrize('case', wc.ALL_CASES, ids=wc.case_id)
def test_integer_inputs_equal_the_integer_reference_bit_for_bit(pk, case):
    wc.check_exact(pk, DEV, case)


@pytest.mark.parametrize('case', wc.ALL_CASES, ids=wc.case_id)
def test_real_inputs_within_the_summation_bound(pk, case):
    p = wc.plan(case.M, case.N, case.K)
    ratio = wc.check_real(pk, DEV, case)
    print('\n[wgrad] %s %s splits %d (%s): error / bound %.4f' % (p.route, wc.case_id(case), p.splits,
                                                                 ', '.join(wc.reached(case, True, True)), ratio))


# ---------------------------------------------------------------------------------------------------------------- 4. the C ABI
@pytest.mark.parametrize('cid,relu_x,bias', [('4104-832-224', True, True), ('4104-832-224', False, False), ('20488-416-96', True, True),
                                             ('5003-832-100', True, True), ('17-260-420', False, True), ('4609-128-32', True, False)])
def test_row_strides_above_the_widths_and_canaries(pk, cid, relu_x, bias):
    """ldg = N + 4, ldx = K + 8 with 1e30 in the padding columns (the LDS-DMA row offsets of wgrad16, its shifted last K column, the
    clamped loads of the generic kernel); the workspace starts as NaN, so the zero-fill of an empty slice is what keeps dW finite."""
    case = W16.get(cid) or GEN[cid]
    wc.check_abi(pk, DEV, case, relu_x, bias, pad_g=4, pad_x=8)


@pytest.mark.parametrize('cid', ['4096-416-64', '20488-416-96', '4104-832-224', '4609-128-32', '17-260-420', '1000-36-36'])
@pytest.mark.parametrize('dw_off', [0, 1])
def test_accumulate_with_the_bias_gradient_aligned_and_not(pk, cid, dw_off):
    """accumulate = 1 with db non-null onto integer seeds: the accumulate branches of wgrad_reduce4_kernel and short_reduce_kernel;
    dW four bytes off alignment: the scalar wgrad_reduce_kernel (8 partials per round and the remainder: 9, 41, 18, 1, 3 partials)."""
    case = W16.get(cid) or GEN[cid]
    wc.check_abi(pk, DEV, case, True, True, accumulate=True, dw_off=dw_off)
    if dw_off:
        wc.check_abi(pk, DEV, case, False, False, accumulate=False, dw_off=dw_off)


@pytest.mark.parametrize('cid', ['4104-832-224', '1000-36-36'])
def test_real_inputs_accumulate_within_the_bound_of_the_base(pk, cid):
    case = W16.get(cid) or GEN[cid]
    a = wc.Abi(pk, DEV, case, 'real', pad_g=4, pad_x=8)
    rng = np.random.default_rng(case.M)
    base_w, base_b = (1e3 * rng.normal(size=(case.N, case.K))).astype(wc.F32), (1e3 * rng.normal(size=(case.N,))).astype(wc.F32)
    a.seed(base_w, base_b)
    assert a.call(True, True, True) == pk._lib.OK
    ref = wc.reference(case.M, case.N, case.K, 'real', True)
    want_w, want_b = ref.dw + base_w.astype(np.float64), ref.db + base_b.astype(np.float64)
    bw, bb = wc.bounds(case.M, a.splits, ref, base_w, base_b)              # (the final add rounds once: U |base| + slack of the sum)
    dw, db = a.results()
    ratio = max(wc.within(dw, want_w, bw, cid + ' dW'), wc.within(db, want_b, bb, cid + ' db'))
    a.guards_intact(cid)
    print('\n[wgrad] accumulate %s: error / bound %.4f' % (cid, ratio))


@pytest.mark.parametrize('cid', ['4096-416-64', '1000-36-36'])
def test_argument_contract(pk, cid):
    """Every rejected call returns EINVAL and writes nothing -- not the outputs, not the workspace, not a canary."""
    case = W16.get(cid) or GEN[cid]
    a = wc.Abi(pk, DEV, case, 'int', pad_g=4, pad_x=8)
    EINVAL, null = pk._lib.EINVAL, ctypes.c_void_p(0)
    off4 = lambda t: ctypes.c_void_p(t.data_ptr() + 4)      # noqa: E731
    rejected = [dict(N=case.N - 2), dict(K=case.K - 2), dict(ldg=a.ldg + 2), dict(ldx=a.ldx + 2), dict(g=off4(a.g)), dict(x=off4(a.x)),
                dict(ldg=case.N - 4), dict(ldx=case.K - 4), dict(splits=0), dict(M=0), dict(g=null), dict(x=null), dict(dw=null),
                dict(ws=null)]
    if wc.plan(case.M, case.N, case.K).route == 'w16':
        # 16 rows x ld x 4 bytes no longer fit the 32-bit tile offsets of the LDS-DMA plan: a number only, nothing is read
        rejected += [dict(ldg=1 << 25), dict(ldx=1 << 25)]
    for over in rejected:
        assert a.call(True, True, False, **over) == EINVAL, over
    assert a.call(True, True, True, N=case.N - 2) == EINVAL
    torch.cuda.synchronize()
    a.untouched(cid)
    assert a.call(True, True, False) == pk._lib.OK                          # ... and the same operands, unchanged, are accepted
    wc.same_bits(a.results()[0], wc.reference(case.M, case.N, case.K, 'int', True).dw, cid + ' after the rejected calls')
    a.guards_intact(cid)


# ---------------------------------------------------------------------------------------------------------------- 5. column sums
@pytest.mark.parametrize('chunks', wc.COLSUM_CHUNKS)
def test_column_sums_across_the_short_reduce_loop(pk, chunks):
    worst = 0.0
    for n in wc.colsum_rows(chunks):
        assert wc.colsum_chunks(n)[0] == chunks
        for d in wc.COLSUM_WIDTHS:
            worst = max(worst, wc.check_colsum(pk, DEV, n, d))
    assert chunks != 512 or wc.colsum_chunks(wc.colsum_rows(chunks)[0])[2] == 1      # (131073 rows: the last chunk is empty)
    print('\n[wgrad] colsum %d chunks: error / bound %.4f' % (chunks, worst))


# ---------------------------------------------------------------------------------------------------------------- 6. autograd
class _Spies:
    """Records the (M, N, K) of every ops.linear_wgrad and the (mask, skip) of every ops.rowlin the autograd nodes issue."""

    def __init__(self, pk, monkeypatch):
        self.wgrad, self.rowlin = [], []
        real_wgrad, real_rowlin = pk.ops.linear_wgrad, pk.ops.rowlin

        def wgrad(g, x, *a, **k):
            self.wgrad.append((g.shape[0], g.shape[1], x.shape[1], bool(k.get('bias')), bool(k.get('relu_x'))))
            return real_wgrad(g, x, *a, **k)

        def rowlin(*a, **k):
            self.rowlin.append((k.get('mask') is not None, k.get('skip') is not None))
            return real_rowlin(*a, **k)
        monkeypatch.setattr(pk.ops, 'linear_wgrad', wgrad)
        monkeypatch.setattr(pk.ops, 'rowlin', rowlin)

    def took_the_trained_route(self, pk, n_wgrad, relu_x, masks):
        assert len(self.wgrad) == n_wgrad and all(w[3] and w[4] == relu_x for w in self.wgrad), self.wgrad
        for M, N, K, _, _ in self.wgrad:
            p = wc.plan(M, N, K)
            assert p.route == 'w16' and (M, N, K) == (4112, 416, 416)
            if not wc.pinning_is_off():
                assert wc.library_plan(pk, M, N, K) == (p.splits, (p.splits + 1) * (N * K + N))
        assert [r for r in self.rowlin if r[0]] == masks, self.rowlin       # the data gradients: (masked, skip added)
        self.wgrad, self.rowlin = [], []


def _T(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


def test_autograd_nodes_on_the_trained_route(pk, monkeypatch):
    """LinearFn in three forms and ResBlockFn at n = 4112, d = 416: forward on rowlin, data gradient on rowlin (masked; with the
    skip gradient in the block), weight and bias gradients on wgrad16_kernel<4, RELU, true> -- every gradient against fp64 torch
    at the 2e-5 of tests/test_gpu_training.py::test_linear_backward."""
    n, d = 4112, 416
    rng = np.random.default_rng(n + d)
    x, res, go = (_T(rng.normal(size=(n, d))) for _ in range(3))
    ws = [_T(rng.normal(size=(d, d)) / np.sqrt(d)) for _ in range(2)]
    bs = [_T(rng.normal(size=(d,))) for _ in range(2)]
    spies = _Spies(pk, monkeypatch)
    ag = pk.autograd
    assert ag.ROWLIN_IN_TRAINING and pk.ops.TRUNK_WIDTH == d
    with pk.kernels(train_precision='f32'):
        for relu_in, relu_out, use_res in [(True, False, False), (True, False, True), (False, True, False)]:
            xr, wr, br, rr = [t.clone().double().requires_grad_(True) for t in (x, ws[0], bs[0], res)]
            y = torch.nn.functional.linear(torch.relu(xr) if relu_in else xr, wr, br)
            y = torch.relu(y) if relu_out else y
            y = y + rr if use_res else y
            y.backward(go.double())
            xg, wg, bg, rg = [t.clone().cuda().requires_grad_(True) for t in (x, ws[0], bs[0], res)]
            out = ag.LinearFn.apply(xg, wg, bg, relu_in, relu_out, rg if use_res else None)
            out.backward(go.cuda())
            what = (relu_in, relu_out, use_res)
            assert rel_err(out, y) < 1e-5, what
            errs = [rel_err(a.grad, b.grad) for a, b in ((xg, xr), (wg, wr), (bg, br))]
            print('\n[wgrad] LinearFn %s: dx %.2e dw %.2e db %.2e' % ((what,) + tuple(errs)))
            assert max(errs) < 2e-5, (what, errs)
            if use_res:
                assert rel_err(rg.grad, rr.grad) < 1e-6
            assert len(spies.rowlin) == (1 if relu_out else 2), spies.rowlin      # (a relu_out forward is on the generic Linear)
            spies.took_the_trained_route(pk, 1, relu_in, [(True, False)] if relu_in else [])
        xd = x.double().requires_grad_(True)
        wd, bd = [t.double().requires_grad_(True) for t in ws], [t.double().requires_grad_(True) for t in bs]
        yd = xd + torch.relu(torch.relu(xd) @ wd[0].t() + bd[0]) @ wd[1].t() + bd[1]
        yd.backward(go.double())
        leaves = [t.clone().cuda().requires_grad_(True) for t in (x, ws[0], bs[0], ws[1], bs[1])]
        out = ag.ResBlockFn.apply(leaves[0] * 1.0, *leaves[1:])
        out.backward(go.cuda())
        assert rel_err(out, yd) < 1e-5
        errs = [rel_err(a.grad, b.grad) for a, b in zip(leaves, (xd, wd[0], bd[0], wd[1], bd[1]))]
        print('\n[wgrad] ResBlockFn: dx %.2e dw0 %.2e db0 %.2e dw1 %.2e db1 %.2e' % tuple(errs))
        assert max(errs) < 2e-5, errs
        assert len(spies.rowlin) == 4, spies.rowlin
        spies.took_the_trained_route(pk, 2, True, [(True, False), (True, ag.ROWLIN_HALF_CU)])
