"""CPU: the fp64 statement of the fused-attention contract (tests/attention_contract.py) against the reference's own
results (tests/golden), and the tolerances of the direct kernel tests (tests/test_gpu_attention_contract.py) against
the chain tolerance -- both without a GPU."""
import numpy as np
import pytest

import attention_contract as ac
import golden_cases as gc
from conftest import load_golden
from oracle import path as op

T = gc.as_tensor
TOL = 2e-5   # tests/test_oracle_golden.py


def close(a, b, tol=TOL):
    assert a.shape == b.shape
    np.testing.assert_allclose(a, b, rtol=0, atol=tol)

PTL = [c for c in gc.PTL_CASES if c['name'] in ('cross_d416_e288_k14', 'self_d36_k16')]


def _statement(case):
    x, pos, x2, pos2, sd = gc.ptl_inputs(case)
    if x2 is None:
        x2, pos2 = x, pos
    idx = op.knn_indices(T(pos)[None], T(pos2)[None], case['k'])[0].numpy()
    return ac.attention_reference(ac.merged_operands(sd, x, pos, x2, pos2, idx))['agg']


@pytest.mark.parametrize('case', PTL, ids=lambda c: c['name'])
def test_fp64_statement_reproduces_the_reference_layer(case):
    """Weights merged in fp64, the contract's formula in fp64: the reference's fp32 layer at the
    tolerance tests/test_oracle_golden.py uses for the restatement."""
    close(_statement(case), load_golden('g2_ptl_' + case['name'])['agg'].astype(np.float64))


@pytest.mark.parametrize('case', gc.PTL_REGIME_CASES, ids=lambda c: c['name'])
def test_fp64_statement_reproduces_the_reference_regimes(case):
    """Saturated softmax, equal logits, one dominant neighbour: against the reference's fp32 run at the scaled oracle
    tolerance and against its fp64 run at the bound of test_g2r_pt_layer_regimes."""
    agg = _statement(case)
    g = load_golden('g2r_ptl_' + case['name'])
    close(agg, g['agg'].astype(np.float64), TOL * max(1.0, float(np.abs(g['agg']).max())))
    close(agg, g['agg64'], gc.regime_bound(g, 'agg'))


@pytest.mark.parametrize('case', ac.ALL_CASES, ids=lambda c: c['name'])
def test_kernel_test_bounds_stay_within_the_chain_tolerance(case):
    """bound = max(4 E32, 16 2^-24 S) of every operand set <= 2e-5 max(1, S), for every compared tensor, and the
    regime each set claims holds on the reference."""
    pairs = case['kernel'] == '16p' and case['n'] != 'rounds'
    opnd, r64, r32, bounds = ac.case_bounds(case, want_pairs=pairs)
    ac.check_regime(case, opnd, r64, r32)
    for key, (e32, s, b) in bounds.items():
        print('[%s] %s: E32 %.3g  S %.3g  bound %.3g  limit %.3g' % (case['name'], key, e32, s, b, ac.CHAIN_TOL * max(1.0, s)))
        assert b <= ac.CHAIN_TOL * max(1.0, s), (key, e32, s, b)
