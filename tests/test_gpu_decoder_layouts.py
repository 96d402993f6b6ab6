"""GPU: the decoder over the layouts and kernel selections its contract admits (check_decoder in csrc/path.hip), where every
other decoder test builds configs.model_args(kind): the cross_after walk of decoder_forward, the bookkeeping of
OCC4D_PATH_FUSED_INTERP, the n_cross == 0 branches (local_mode='feature'), the dg == 0 branch of the per-scene tables, the
n_freq == 0 copy path, the generic-Linear trunk of d_hidden != 416 and the attention fallbacks for k > 14 and d = 288 -- against
oracle/path.py in fp64, within golden_cases.regime_bound = max(1e-4, 2 max|ref32 - ref64|) per case and tensor.  The case
tables, references, bound and checks are in tests/decoder_layout_cases.py; tests/test_decoder_layouts_host.py runs the layout
matrix on the g++ twin and proves what the tables cover.

Every element of the selection product is held to the same bound, the split-precision ones included, and to the launch counts
of the library's event hook.  fused_interp with a split-precision trunk used to lose the lin_z term of every block without a
cross layer right before it (fuse_ok in decoder_forward did not look at which kernel takes the block): with the library built
from that csrc/path.hip those elements are off by 0.20 .. 0.86 (output) and 0.68 .. 2.8 (penult) on every product layout but
(2, 2), where each block follows a layer; here they pass, equal bit for bit to the selection without fused_interp.

Measured on the MI355X: 435 tests in 9 s.  Worst |hip - ref64|, output / penult: layouts under the default selection 9.2e-6 /
2.4e-5 (the oracle's own fp32 run: 8.9e-6 / 1.9e-5), the scaled (7, 3) case 1.6e-5 / 5.3e-5 (5.9e-6 / 2.1e-5); the selection
product 6.7e-6 / 2.4e-5, its split-precision elements no worse than the fp32 ones.  All bounds are 1e-4.

Every case prints its own errors (-s); the worst per family are recorded in DESIGN.md section 2."""
import pytest
import torch

import decoder_layout_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pk():
    import occlusions4d_amd
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    occlusions4d_amd._lib.lib()
    return occlusions4d_amd


@pytest.mark.parametrize('case', dc.LAYOUT_CASES, ids=dc.case_id)
def test_decoder_layouts(pk, case):
    dc.check_forward(pk, 'cuda', case)


@pytest.mark.parametrize('sel', dc.SELECTIONS, ids=dc.selection_id)
@pytest.mark.parametrize('name', dc.PRODUCT_LAYOUTS)
def test_decoder_selection_product(pk, name, sel):
    dc.check_selection(pk, 'cuda', dc.BY_NAME[name], sel)


@pytest.mark.parametrize('trunk_precision', dc.SPLIT)
@pytest.mark.parametrize('name', dc.PRODUCT_LAYOUTS)
def test_fused_interp_changes_nothing_where_the_split_trunk_takes_the_block(pk, name, trunk_precision):
    """Only the fp32 fused block adds the next block's lin_z term in its epilogue: under a split-precision trunk the flag is
    without effect, bit for bit."""
    case = dc.BY_NAME[name]
    r = dc.reference(case)
    net = dc.shared_net(pk, 'cuda', case)
    args = (dc.dev(r['q'], 'cuda'), dc.dev(r['abstract'], 'cuda'), dc.dev(r['fglob'], 'cuda'), None)
    with torch.no_grad():
        with pk.kernels(trunk_precision=trunk_precision, fused_interp=False):
            out, pen = net(*args)
        with pk.kernels(trunk_precision=trunk_precision, fused_interp=True):
            out_f, pen_f = net(*args)
    assert torch.equal(out, out_f) and torch.equal(pen, pen_f)


@pytest.mark.parametrize('name', dc.ENTRY_LAYOUTS)
def test_decoder_entry_forms(pk, name):
    dc.check_entry_forms(pk, 'cuda', dc.BY_NAME[name])


@pytest.mark.parametrize('case', dc.TRAIN_CASES, ids=dc.case_id)
def test_decoder_layout_gradients(pk, case):
    dc.check_training(pk, 'cuda', case)
