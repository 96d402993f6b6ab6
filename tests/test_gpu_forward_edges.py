"""GPU: the fp32 Linear (csrc/linear.hip) at every column-tile count NT x every epilogue EPI its launcher can pick, with the
swish-on-load template, and the forward reductions of csrc/pointops.hip (interp_add's three kernels, mean_rows, layernorm) at
the edges of their tilings -- each against an fp64 statement of the same operation on the same fp32 inputs, element by element,
within a bound derived from the sum's length and sum|term|.  The case matrices, references, bounds and their derivations are in
tests/forward_cases.py; tests/test_forward_host.py runs the same checks on the g++ twin and proves the coverage claims (which
NT a shape reaches is restated from the launcher and tied to its source text there).

Worst error / bound measured on the MI355X (every case prints its own):
    Linear        0.467 over all cases; by epilogue EPI 0 / 1 / 2: 0.437 / 0.467 / 0.463; by NT 1, 2, 3, 4, 5, 9, 13: 0.395, 0.388,
                  0.434, 0.382, 0.399, 0.439, 0.467 (the g++ twin: 0.496)
    interp_add    scalar 0.419, float4 runtime k 0.405, float4 k = 8 0.392; all three equal the restated order bit for bit
    mean_rows     0.234
    layernorm     0.463
Swish: numpy float32 against fp64 is 3.89 units of 2^-24 per term over the 200 000 samples of [-20, 20], which allows the kernel
15.54, added to c; the worst error / bound of a swish case was 0.319.  Per term (Linear against an identity weight, where the
output is the kernel's swish itself) the kernel against fp64 is 2.6 units for x >= 0, 5.7 on [-5, 0), 9.6 on [-10, -5) and 17.4 on
[-20, -10): __expf is exp2(log2(e) x) with the product rounded, so its relative error grows with |x| -- on values below 5e-4.

Mutation check (on scratch copies of csrc/linear.hip, not kept): skipping the last, partial chunk of the staged epilogue under
NT = 13 fails the six NT = 13 cases of EPI 1 and 2; taking the bias of every chunk from the first one for NT >= 9 fails five cases;
leaving the fourth component of each float4 of x without its swish fails all eleven swish cases.  The older direct Linear tests
(test_gpu_kernels_random, test_gpu_parity, test_gpu_training::test_linear_backward, test_gpu_contracts) pass on all three."""
import pytest
import torch

import forward_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pk():
    import occlusions4d_amd
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    occlusions4d_amd._lib.lib()
    return occlusions4d_amd


@pytest.mark.parametrize('case', fc.LINEAR_CASES, ids=fc.lin_id)
def test_linear_tile_variants_within_the_summation_bound(pk, case):
    ratio = fc.check_linear(pk, 'cuda', case)
    swish = ''
    if case.relu_in == 2:
        swish = ' (swish: numpy fp32 %.2f units, allowed %.2f)' % fc.swish_allowance()
    print('\n[forward] linear %s NT %d EPI %d: error / bound %.3f%s' % (fc.lin_id(case), fc.picked_nt(case.M, case.N),
                                                                     fc.case_epi(case), ratio, swish))


@pytest.mark.parametrize('case', fc.INTERP_CASES, ids=lambda c: '%d-%d-k%d-%s-%s' % (c.n, c.d, c.k, 'cvec' if c.cvec else 'nocvec', c.layout))
def test_interp_add_three_kernels_bound_and_documented_order(pk, case):
    ratio = fc.check_interp(pk, 'cuda', case, 'device')
    print('\n[forward] interp_add %s: error / bound %.3f' % (fc.interp_kernel(case), ratio))


@pytest.mark.parametrize('case', fc.MEAN_CASES, ids=lambda c: '%d-%d-%s' % (c.n, c.d, 'strided' if c.strided else 'plain'))
def test_mean_rows_within_the_summation_bound(pk, case):
    print('\n[forward] mean_rows: error / bound %.3f' % fc.check_mean(pk, 'cuda', case))


@pytest.mark.parametrize('case', fc.NORM_CASES, ids=lambda c: '%d-%d-%s%s%s-kind%d' % (c.n, c.d, 'a' if c.affine else '_', 'r' if c.relu else '_',
                                                                                     's' if c.strided else '_', c.kind0))
def test_layernorm_within_the_conditioned_bound(pk, case):
    print('\n[forward] layernorm: error / bound %.3f' % fc.check_norm(pk, 'cuda', case))
