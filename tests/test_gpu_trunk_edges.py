"""GPU: the fp32 trunk kernels -- csrc/trunk.hip (occ4d_resblock_f32, _addrows, _chain, occ4d_rowlin_f32, _linz, _masked),
csrc/trunk4.hip (occ4d_resblock4_f32, occ4d_rowlin4_f32, _masked, _masked_skip) and occ4d_interp_dense_f32 -- through the
pk.ops wrappers, held to tests/trunk_cases.py: every row operand a framed view with a row stride of its own (nothing outside
an output view written, everything inside written, every input bit-identical afterwards), the derived per-element bounds of
that module's docstring against numpy fp64 over seven operand regimes, exact integer cases held to `==`, dead hidden layers
and masked cells held to their exact values, and bit-for-bit metamorphic checks (row position, row homogeneity, the half-CU
tail split against the same rows run alone).  tests/test_trunk_cases_host.py validates the references, the bounds and the
checks themselves without a device.  Nothing here measures time; only the two tail-split cases are above 300 rows."""
import numpy as np
import pytest
import torch

import occlusions4d_amd as pk
import trunk_cases as tc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ids = lambda v: tc.call_id(v) if isinstance(v, tc.Call) else str(v)       # noqa: E731


@pytest.mark.parametrize('entry,pack,n', tc.FRAME_CALLS, ids=ids)
def test_frames_and_bounds(entry, pack, n):
    """Every form of the entry point at n rows, every operand a view."""
    calls = tc.entry_calls(entry, pack, n)
    worst = max(tc.run_and_check(pk.ops, DEV, c) for c in calls)
    print('\n[trunk] %s %s n=%d: %d calls, worst error / bound %.3f' % (entry, pack, n, len(calls), worst))


@pytest.mark.parametrize('entry,pack', sorted({(e, p) for e, p, _ in tc.FRAME_CALLS}), ids=ids)
def test_exact_integer_cases(entry, pack):
    """Operands whose every sum is exact in fp32 in any order: the device equals fp64, no tolerance."""
    for n in tc.EDGE_ROWS[pack]:
        for c in tc.entry_calls(entry, pack, n, 'exact'):
            tc.run_and_check(pk.ops, DEV, c, 'exact')


@pytest.mark.parametrize('c', tc.dead_calls(), ids=ids)
def test_dead_hidden_layer(c):
    """b0 = -2^20: relu(h) = 0, y = f32(x + b1) [+ addrows as one more fp32 addition], bit for bit."""
    tc.run_and_check(pk.ops, DEV, c, 'dead')


@pytest.mark.parametrize('regime', tc.REGIMES)
def test_regimes(regime):
    """(The masked cells -- exactly 0.0, exactly skip -- are checked by every masked call of test_frames_and_bounds and of
    test_exact_integer_cases: tc.check_masked.)"""
    calls = tc.regime_calls(regime)
    worst = max(tc.run_and_check(pk.ops, DEV, c) for c in calls)
    print('\n[trunk] regime %s: %d calls, worst error / bound %.3f' % (regime, len(calls), worst))


@pytest.mark.parametrize('c', tc.METAMORPHIC, ids=ids)
def test_a_row_does_not_depend_on_its_position(c):
    tc.row_position(pk.ops, DEV, c, tc.bits_equal)


@pytest.mark.parametrize('c', tc.HOMOGENEOUS, ids=ids)
def test_rows_are_homogeneous(c):
    tc.homogeneity(pk.ops, DEV, c, tc.bits_equal)


@pytest.mark.parametrize('opts', ['interp res', 'mask skip'])
def test_half_cu_tail_split(opts):
    """The split changes a row's workgroup, never its k order (tests/test_gpu_trunk.py::test_half_cu_rowlin_tail_split says
    so): with an interpolation term, and with mask + skip (res_post)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count           # as rowlin4_grid reads it
    ratio = tc.tail_split(pk.ops, DEV, cus, opts, tc.bits_equal)
    print('\n[trunk] tail split, %d CUs, n=%d, %s: worst error / bound %.3f' % (cus, tc.tail_split_rows(cus), opts, ratio))


def test_rowlin_rejects_y_overlapping_x():
    """A split row tile's workgroups each read whole rows of x and write a share of y: no rowlin runs in place.  Rejected by
    the library (an AssertionError of _lib.check), not launched: the buffer is bit-identical afterwards."""
    n = 17
    rng = np.random.default_rng(5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()      # noqa: E731
    big = dev(rng.normal(size=(n, tc.H + 8)))
    keep = big.clone()
    x = big[:, :tc.H]
    mask, skip = dev(rng.normal(size=(n, tc.H))), dev(rng.normal(size=(n, tc.H)))
    idx, zw = dev(np.zeros((n, 8))).int(), dev(rng.uniform(size=(n, 8)))
    tab, zc = dev(rng.normal(size=(tc.TABLE_ROWS, tc.H))), dev(rng.normal(size=tc.H))
    for pack in (tc.FULL, tc.HALF):
        for n_out, y in ((tc.H, x), (tc.H, big[:, 4:4 + tc.H]), (32, big[:, 64:96]), (32, big[:, tc.H - 24:tc.H + 8])):
            w, b = tc.weight('init', 'lin', n_out)
            p, b = getattr(pk.ops, tc.PACKERS[pack][0])(dev(w)), dev(b)
            forms = [dict(), dict(relu_in=True), dict(mask=mask[:, :n_out])]
            if pack == tc.HALF:
                forms.append(dict(mask=mask[:, :n_out], skip=skip[:, :n_out]))
            for kw in forms:
                with pytest.raises(AssertionError, match='y must not overlap x'):
                    pk.ops.rowlin(x, p, b, n_out, out=y, **kw)
            if pack == tc.FULL:
                with pytest.raises(AssertionError, match='must not overlap'):
                    pk.ops.rowlin_linz(x, p, b, n_out, idx, zw, term=(zc[:n_out], tab[:, :n_out]), out=y)
            torch.cuda.synchronize()
            assert torch.equal(big.view(torch.int32), keep.view(torch.int32)), (pack, n_out)
    # res may alias y, as before; and the rows right behind x's last row are no overlap
    two = dev(rng.normal(size=(2 * n, tc.H)))
    w, b = tc.weight('init', 'lin', tc.H)
    for pack in (tc.FULL, tc.HALF):
        p = getattr(pk.ops, tc.PACKERS[pack][0])(dev(w))
        want = pk.ops.rowlin(two[:n], p, dev(b), tc.H, residual=two[n:].clone())
        got = pk.ops.rowlin(two[:n], p, dev(b), tc.H, residual=two[n:], out=two[n:])
        assert got is not None and torch.equal(two[n:], want)
