"""No GPU: what tests/test_gpu_forward_edges.py rests on, checked on the host first.  The restated launch rule of the fp32
Linear against the text of csrc/linear.hip; the coverage of its case matrix (all 7 x 3 (NT, EPI) pairs, the swish subset); the
bound helpers (they reject a result off by one part in 10^5); numpy float32 restatements of every reduction in two summation
orders, both inside the bound; and every check_* of tests/forward_cases.py over its full case matrix on the g++ twin -- an
independent implementation (Linear in plain fp32 loops, the statistics of mean_rows and layernorm in double), so references
and bounds are validated before any device is involved."""
import numpy as np
import pytest

import forward_cases as fc
import occlusions4d_amd as pk

F32, U = np.float32, fc.U


@pytest.fixture
def twin():
    pk.cpu_twin.enable()
    try:
        yield pk
    finally:
        pk.cpu_twin.disable()


# ---------------------------------------------------------------------------------------------------------------- the launch rule
def test_the_restated_launch_rule_is_the_one_in_the_source():
    fc.launch_rule_in_source()
    with open(fc.LINEAR_HIP) as f:
        text = f.read()
    for edit in (('{13, 9, 5, 4, 3, 2, 1}', '{13, 9, 6, 4, 3, 2, 1}'), ('constexpr int BM = 128;', 'constexpr int BM = 64;'),
                 ('kNT[pick]) < 128)', 'kNT[pick]) < 256)')):
        assert edit[0] in text
        with pytest.raises(AssertionError, match='no longer says'):
            fc.launch_rule_in_source(text.replace(*edit))


def test_picked_nt_on_the_shapes_the_matrix_is_built_from():
    table = {(16257, 416): 13, (8065, 420): 13, (5377, 836): 13, (6000, 832): 9, (16257, 288): 9, (16300, 286): 9,
             (16257, 160): 5, (16257, 130): 5, (16257, 128): 4, (16257, 98): 4, (16257, 96): 3, (16257, 66): 3,
             (16257, 64): 2, (16257, 34): 2, (16257, 32): 1, (16257, 5): 1, (16256, 416): 9, (16300, 416): 13}
    for (M, N), nt in table.items():
        assert fc.picked_nt(M, N) == nt, (M, N)
    # the shapes of the existing direct tests stay below the large tilings, which is why this file exists
    assert {fc.picked_nt(M, N) for M in (1, 129, 4097) for N in (5, 36, 64, 144, 288, 416, 832)} <= {1, 2, 4, 5}


def test_linear_cases_reach_every_tiling_every_epilogue_and_the_swish_subset():
    reached = {}
    for c in fc.LINEAR_CASES:
        reached.setdefault((fc.picked_nt(c.M, c.N), fc.case_epi(c)), []).append(fc.lin_id(c))
    want = {(nt, epi) for nt in fc.NT_TABLE for epi in (0, 1, 2)}
    assert len(want) == 21 and set(reached) == want, sorted(want - set(reached))
    swish = [c for c in fc.LINEAR_CASES if c.relu_in == 2]
    assert {fc.case_epi(c) for c in swish} == {0, 1, 2}
    assert {1, 13} <= {fc.picked_nt(c.M, c.N) for c in swish}
    assert {c.relu_in for c in fc.LINEAR_CASES} == {0, 1, 2}
    print('\n[forward] (NT, EPI) pairs reached: %s' % ', '.join('%d/%d x%d' % (k + (len(v),)) for k, v in sorted(reached.items())))
    print('[forward] swish cases: %s' % ', '.join('NT %d EPI %d' % (fc.picked_nt(c.M, c.N), fc.case_epi(c)) for c in swish))
    # EPI 2 with each of residual, add_rows, sub_rows alone and all together; both add_div; every layout, aliasing under EPI 2 and 0
    epi2 = [c for c in fc.LINEAR_CASES if fc.case_epi(c) == 2]
    assert {'r', 'a', 's', 'ars'} <= {''.join(sorted(set(c.terms) & set('ars'))) for c in epi2}
    assert {c.add_div for c in epi2 if 'a' in c.terms} == {1, 14}
    assert {c.layout for c in fc.LINEAR_CASES} == {'plain', 'strided', 'out1', 'res1', 'alias', 'alias1'}
    assert {fc.case_epi(c) for c in fc.LINEAR_CASES if c.layout in ('alias', 'alias1')} == {0, 2}
    # the k loop: one k-tile, a partial k-tile, 26 k-tiles, K % 4 != 0; the last row tile holds one row; 4 live columns
    ks = {c.K for c in fc.LINEAR_CASES}
    assert {4, 8, 36, 68, 416, 832} <= ks and any(k % 4 for k in ks)
    assert any(c.M % fc.BM == 1 for c in fc.LINEAR_CASES) and any(c.N % (32 * 13) == 4 for c in fc.LINEAR_CASES)
    assert max(c.M * c.K * c.N for c in fc.LINEAR_CASES) == 16300 * 68 * 416
    assert len({fc.lin_id(c) for c in fc.LINEAR_CASES}) == len(fc.LINEAR_CASES)


def test_reduction_cases_reach_every_kernel_and_edge():
    kinds = {(fc.interp_kernel(c), c.cvec) for c in fc.INTERP_CASES}
    assert kinds == {(k, v) for k in ('scalar', 'float4 k=8', 'float4 runtime k') for v in (False, True)}, kinds
    assert {c.k for c in fc.INTERP_CASES} == {1, 3, 8, 12, 16}
    assert {(c.n, c.d) for c in fc.INTERP_CASES} == {(n, d) for n in (1, 63, 65, 1000) for d in (4, 36, 38, 416)}
    assert {(c.layout, fc.interp_kernel(c) == 'scalar') for c in fc.INTERP_CASES} >= {('plain', True), ('plain', False), ('strided', True),
                                                                                     ('strided', False), ('off1', True)}
    assert {(c.n, c.d) for c in fc.MEAN_CASES} == {(n, d) for n in (1, 7, 8, 9, 531, 20000) for d in (1, 31, 32, 33, 288)}
    assert {c.strided for c in fc.MEAN_CASES} == {False, True}
    assert {(c.n, c.d) for c in fc.NORM_CASES} == {(n, d) for n in (1, 3, 4, 5, 1000) for d in (1, 2, 63, 64, 65, 416, 600)}
    assert {(c.affine, c.relu, c.strided) for c in fc.NORM_CASES} == {(a, r, s) for a in (False, True) for r in (False, True)
                                                                     for s in (False, True)}
    assert {c.kind0 for c in fc.NORM_CASES if c.n == 1} == set(range(len(fc.NORM_KINDS)))


# ---------------------------------------------------------------------------------------------------------------- bounds
def test_swish_allowance_is_measured_and_floored():
    measured, allowed = fc.swish_allowance()
    print('\n[forward] swish: numpy fp32 against fp64 %.2f units of 2^-24; the kernel is allowed %.2f per term' % (measured, allowed))
    assert 0.5 < measured < 16 and allowed == max(4 * measured, 8.0)


def _off_by_1e5(ref):
    return (ref * (1 + 1e-5)).astype(F32)


def test_bounds_reject_one_part_in_1e5():
    # Linear: every activation, with and without epilogue terms.  (K <= 68: at K = 832 the worst case of 832 roundings is itself
    # 5 parts in 10^5 of sum|term|.)
    for c in (fc.L(300, 36, 40, 0, 'r'), fc.L(300, 8, 36, 1, 'b'), fc.L(129, 68, 33, 2, 'br'), fc.L(40, 4, 36, 0, '')):
        ref, bound = fc.linear_reference(c, fc.linear_inputs(c))
        assert fc.within(ref.astype(F32), ref, bound) <= 0.5
        with pytest.raises(AssertionError, match='outside the bound'):
            fc.within(_off_by_1e5(ref), ref, bound)
    h = fc.interp_inputs(fc.Interp(65, 36, 8, True, 'plain'))
    ref, bound = fc.interp_reference(h)
    with pytest.raises(AssertionError, match='outside the bound'):
        fc.within(_off_by_1e5(ref), ref, bound)
    x = fc.mean_inputs(fc.Mean(9, 33, False))
    ref, bound = fc.mean_reference(x)
    with pytest.raises(AssertionError, match='outside the bound'):
        fc.within(_off_by_1e5(ref), ref, bound)
    for c in (fc.Norm(5, 64, True, False, False, 0), fc.Norm(5, 2, False, False, False, 0)):     # (at d = 600: 308 roundings)
        x, gamma, beta, _ = fc.norm_inputs(c)
        ref, bound = fc.norm_reference(x, gamma, beta, c.relu)
        with pytest.raises(AssertionError, match='outside the bound'):
            fc.within(_off_by_1e5(ref), ref, bound)
    # a NaN (an output element that was never written) is outside any bound; a zero bound asks for exactly the reference
    ref, bound = np.ones((2, 2)), np.full((2, 2), 1e-3)
    with pytest.raises(AssertionError):
        fc.within(np.array([[1, np.nan], [1, 1]], F32), ref, bound)
    assert fc.within(np.zeros((2, 2), F32), np.zeros((2, 2)), np.zeros((2, 2))) == 0.0
    with pytest.raises(AssertionError):
        fc.within(np.full((2, 2), 1e-30, F32), np.zeros((2, 2)), np.zeros((2, 2)))


def test_float32_restatements_hold_the_bounds_in_two_orders():
    worst = dict(linear=0.0, interp=0.0, mean=0.0, norm=0.0)
    # Linear: numpy's float32 matrix product (blocked, another order again than the twin's loops and the kernel's k map)
    for c in (fc.L(300, 36, 40, 0, 'r'), fc.L(257, 832, 68, 1, 'r'), fc.L(129, 68, 33, 2, 'r')):
        h = fc.linear_inputs(c)
        x = h['x']
        with np.errstate(over='ignore'):                                  # (exp(104) = inf: the sigmoid is 0, as on the device)
            a = np.maximum(x, F32(0)) if c.relu_in == 1 else x * (F32(1) / (F32(1) + np.exp(-x))) if c.relu_in == 2 else x
        got = a @ h['w'].T + h['residual']
        assert got.dtype == F32
        worst['linear'] = max(worst['linear'], fc.within(got, *fc.linear_reference(c, h), fc.lin_id(c)))
    orders_differ = 0
    for c in fc.INTERP_CASES:
        h = fc.interp_inputs(c)
        ref, bound = fc.interp_reference(h)
        dev, twin = fc.restate_interp(h, 'device'), fc.restate_interp(h, 'twin')
        worst['interp'] = max(worst['interp'], fc.within(dev, ref, bound, 'device order'), fc.within(twin, ref, bound, 'twin order'))
        orders_differ += not np.array_equal(dev, twin)
        assert c.cvec or np.array_equal(dev, twin)                        # (without a cvec the two orders are one)
    assert orders_differ > 0
    for c in fc.MEAN_CASES:
        x = fc.mean_inputs(c)
        ref, bound = fc.mean_reference(x)
        serial, groups = fc.restate_mean(x, 'serial'), fc.restate_mean(x, 'groups')
        worst['mean'] = max(worst['mean'], fc.within(serial, ref, bound, 'serial'), fc.within(groups, ref, bound, 'groups'))
        if c.n <= 2:
            assert np.array_equal(serial, groups)
    differ = 0
    for c in fc.NORM_CASES:
        x, gamma, beta, kind = fc.norm_inputs(c)
        ref, bound = fc.norm_reference(x, gamma, beta, c.relu)
        for order in ('serial', 'lanes'):
            got = fc.restate_norm(x, gamma, beta, c.relu, order)
            worst['norm'] = max(worst['norm'], fc.within(got, ref, bound, '%s %s' % (order, c)))
            fc.norm_exact_rows(x, gamma, beta, c.relu, kind, got, '%s %s' % (order, c))
        differ += not np.array_equal(fc.restate_norm(x, gamma, beta, c.relu, 'serial'), got)
    assert differ > len(fc.NORM_CASES) // 2                               # (the two orders are different computations)
    print('\n[forward] float32 restatements, worst error / bound: %s' % ', '.join('%s %.3f' % kv for kv in sorted(worst.items())))
    assert max(worst.values()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- the twin
CPU = 'cpu'


@pytest.mark.parametrize('case', fc.LINEAR_CASES, ids=fc.lin_id)
def test_linear_on_the_twin(twin, case):
    ratio = fc.check_linear(twin, CPU, case)
    print('\n[forward] twin linear %s NT %d EPI %d: error / bound %.3f' % (fc.lin_id(case), fc.picked_nt(case.M, case.N),
                                                                          fc.case_epi(case), ratio))


def test_interp_add_on_the_twin(twin):
    """The twin adds cvec first: held to ITS order bit for bit (which is the device's where there is no cvec)."""
    worst = max(fc.check_interp(twin, CPU, c, 'twin') for c in fc.INTERP_CASES)
    print('\n[forward] twin interp_add: worst error / bound %.3f' % worst)


def test_mean_rows_on_the_twin(twin):
    worst = max(fc.check_mean(twin, CPU, c) for c in fc.MEAN_CASES)
    print('\n[forward] twin mean_rows: worst error / bound %.3f' % worst)


def test_layernorm_on_the_twin(twin):
    worst = max(fc.check_norm(twin, CPU, c) for c in fc.NORM_CASES)
    print('\n[forward] twin layernorm: worst error / bound %.3f' % worst)
