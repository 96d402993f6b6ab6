"""GPU: the decoder's lin_z terms inside the trunk kernels (include/ext/occ4d_linz.h, csrc/trunk.hip).

occ4d_rowlin_linz_f32 gathers up to two interpolation terms under the stages' MFMAs (the first added to the output rows, the
second stored as dense rows), occ4d_resblock_addrows_f32 adds such dense rows under its last hidden chunk, and the decoder
routes its terms through them by default.  All three are held to `torch.equal` against what they replace -- the plain
launch followed by the stand-alone ops.interp_add pass (or an fp32 row add) -- because both sides add the same
s = (..((0 + w0 t0) + w1 t1) + ..) + zconst last onto the same row; the row kernel is also held to an fp64 evaluation within
the bound tests/test_gpu_trunk.py::test_rowlin_matches_fp64 uses for it on the same input distributions (2e-5 absolute: that
file states it as a literal, so it is named here once, as TRUNK_BOUND, beside the helpers imported from it).

Shapes: rows one short of, at and one past the 16-row wave tile and the 128-row workgroup tile, and 300 (three workgroups);
n_out 32 (one stage), 96 (an odd stage count), 416 (the decoder's); tables of 8 rows (= k: every row is a neighbour of every
query) and 37; weights with zeros and negative entries, neighbour lists that repeat an index.  k = 3: the new entry point
holds a row's list in registers and takes k = 8 only -- its contract rejects every other count, which is what the test
asserts (the runtime-k order stays with ops.interp_add behind the plain launch).  No test here measures time."""
import numpy as np
import pytest
import torch

import decoder_layout_cases as lc
import occlusions4d_amd as pk
from test_gpu_trunk import H, _weights

pytestmark = pytest.mark.gpu
TRUNK_BOUND = 2e-5          # tests/test_gpu_trunk.py: `assert float((got.double() - want).abs().max()) < 2e-5`
ROWS = [1, 15, 16, 17, 127, 128, 129, 300]


def _terms(rng, n, n_out, m, k=8):
    """Two tables side by side in one (m, 2 n_out + 4) buffer (row views of one stride), two constants, lists and weights."""
    tab = torch.from_numpy(rng.normal(size=(m, 2 * n_out + 4)).astype(np.float32)).cuda()
    zc = torch.from_numpy(rng.normal(size=(2, n_out)).astype(np.float32)).cuda()
    idx = rng.integers(0, m, size=(n, k)).astype(np.int32)
    idx[:, 1] = idx[:, 0]                                    # every list repeats an index
    w = rng.uniform(-0.5, 1.0, size=(n, k)).astype(np.float32)
    w[:, 2] = 0.0                                            # a zero weight in every row
    w[0, :] = 0.0
    w /= np.abs(w).sum(1, keepdims=True).clip(1e-12)
    return (zc[0], tab[:, :n_out]), (zc[1], tab[:, n_out:2 * n_out]), torch.from_numpy(idx).cuda(), torch.from_numpy(w).cuda()


def _term64(term, idx, w):
    return term[0].double() + (w.double()[:, :, None] * term[1].double()[idx.long()]).sum(1)


@pytest.mark.parametrize('n_out', [32, 96, 416])
@pytest.mark.parametrize('n', ROWS)
def test_rowlin_terms_equal_the_plain_launch_and_the_pass(n, n_out):
    rng = np.random.default_rng(1000 * n_out + n)
    x = torch.from_numpy(rng.normal(size=(n, H)).astype(np.float32)).cuda()
    wt, b = _weights(rng, n_out)
    p = pk.ops.pack_trunk_rows(wt)
    res = torch.from_numpy(rng.normal(size=(n, n_out)).astype(np.float32)).cuda()
    lin64 = x.double() @ wt.double().T + b.double()
    for m in (8, 37):
        t1, t2, idx, w = _terms(rng, n, n_out, m)
        zero_plus_t2 = pk.ops.interp_add(torch.zeros((n, n_out), device='cuda'), t2[0], t2[1], idx, w)
        for residual in (None, res):
            plain = pk.ops.rowlin(x, p, b, n_out, residual=residual)
            want = pk.ops.interp_add(plain.clone(), t1[0], t1[1], idx, w)
            want64 = lin64 + (residual.double() if residual is not None else 0.0) + _term64(t1, idx, w)
            for first, second in ((True, False), (False, True), (True, True)):
                what = 'n=%d n_out=%d m=%d residual=%s terms=%d%d' % (n, n_out, m, residual is not None, first, second)
                got, dense = pk.ops.rowlin_linz(x, p, b, n_out, idx, w, term=t1 if first else None, term2=t2 if second else None,
                                                residual=residual)
                assert torch.equal(got, want if first else plain), what
                err = float((got.double() - (want64 if first else want64 - _term64(t1, idx, w))).abs().max())
                assert err < TRUNK_BOUND, (what, err)
                if second:
                    assert torch.equal(dense, zero_plus_t2), what
                    err2 = float((dense.double() - _term64(t2, idx, w)).abs().max())
                    assert err2 < TRUNK_BOUND, (what, err2)
                else:
                    assert dense is None
        # in place on the residual rows, as the decoder's layer3 runs (res aliases out)
        buf = res.clone()
        got, dense = pk.ops.rowlin_linz(x, p, b, n_out, idx, w, term=t1, term2=t2, residual=buf, out=buf)
        assert got is buf and torch.equal(buf, want) and torch.equal(dense, zero_plus_t2)


def test_rowlin_terms_contract():
    rng = np.random.default_rng(5)
    n, n_out = 17, 96
    x = torch.from_numpy(rng.normal(size=(n, H)).astype(np.float32)).cuda()
    wt, b = _weights(rng, n_out)
    p = pk.ops.pack_trunk_rows(wt)
    t1, t2, idx, w = _terms(rng, n, n_out, 37)
    with pytest.raises(AssertionError, match='kz = 8'):      # k = 3: the runtime-k order is the stand-alone pass's alone
        pk.ops.rowlin_linz(x, p, b, n_out, idx[:, :3].contiguous(), w[:, :3].contiguous(), term=t1)
    with pytest.raises(AssertionError, match='no interpolation term'):
        pk.ops.rowlin_linz(x, p, b, n_out, idx, w)
    out = torch.zeros((n, n_out), device='cuda')
    with pytest.raises(AssertionError, match='must not alias'):
        pk.ops.rowlin_linz(x, p, b, n_out, idx, w, term=t1, term2=t2, out=out, dense=out)
    with pytest.raises(AssertionError, match='without ztab2'):
        pk.ops.rowlin_linz(x, p, b, n_out, idx, w, term=t1, dense=out)
    # the older entry point keeps its interpolation arguments, any k: the term is the pass behind the plain launch
    full = _terms(rng, n, H, 37, k=3)
    pw, pb = _weights(rng, H)
    got = pk.ops.rowlin(x, pk.ops.pack_trunk_rows(pw), pb, H, interp=(full[0][0], full[0][1], full[2], full[3]))
    want = pk.ops.interp_add(pk.ops.rowlin(x, pk.ops.pack_trunk_rows(pw), pb, H), full[0][0], full[0][1], full[2], full[3])
    assert torch.equal(got, want)
    for name in ('occ4d_rowlin_linz_f32', 'occ4d_resblock_addrows_f32'):
        assert name in pk._lib.ADDON_SIGNATURES and name in pk._lib.LINZ_SIGNATURES and hasattr(pk._lib.lib(), name)
    assert pk._lib.ADDON_HEADERS['LINZ'] == 'ext/occ4d_linz.h'


@pytest.mark.parametrize('n', ROWS)
def test_resblock_addrows_equals_the_block_and_a_row_add(n):
    rng = np.random.default_rng(n)
    x = torch.from_numpy(rng.normal(size=(n, H)).astype(np.float32)).cuda()
    w0, b0 = _weights(rng, H)
    w1, b1 = _weights(rng, H)
    p0, p1 = pk.ops.pack_trunk_rows(w0), pk.ops.pack_trunk_cols(w1)
    add = torch.from_numpy(rng.normal(size=(n, H + 4)).astype(np.float32)).cuda()[:, :H]      # a row view, stride 420
    want = pk.ops.resblock(x, p0, b0, p1, b1) + add
    got = pk.ops.resblock(x, p0, b0, p1, b1, addrows=add)
    assert torch.equal(got, want)
    x2 = x.clone()                                            # y aliasing x
    assert pk.ops.resblock(x2, p0, b0, p1, b1, out=x2, addrows=add) is x2 and torch.equal(x2, want)
    keep = add.clone()
    with pytest.raises(AssertionError, match='addrows must not alias y'):
        pk.ops.resblock(x, p0, b0, p1, b1, out=add, addrows=add)
    assert torch.equal(add, keep)                             # rejected, not run


# ---------------------------------------------------------------------------------------------------------------- decoder
def _case(name, use_at, seed, nq=300):
    """The published block / cross-layer layout (6 blocks, 2 layers) with 300 queries -- three workgroups of the trunk
    kernels -- against 20 abstract points.  A cross layer without layer3 (post_w) is not among the cases: check_decoder
    rejects such a decoder, so that fall-back of the routing cannot be reached through the decoder's entry points."""
    return lc.C(name, 'override' if use_at else 'formula', lc._ia(6, 2), seed, use_at=use_at, nq=nq)


DECODER_CASES = [_case('linz-b6c2', None, 102),                       # the constructor's positions
                 _case('linz-b6-at01', {0: 0, 1: 1}, 500),            # a layer directly behind block 0, the next directly behind block 1
                 _case('linz-b6-at04', {0: 0, 4: 1}, 510)]            # ... and one whose second term would be the last block's


def _inputs(case, m=20):
    """lc.inputs with 20 abstract points.  No tie screening: both sides of every comparison here run the same searches."""
    ia = case.ia
    rng = np.random.default_rng(case.seed)
    (x0, x1), (y0, y1), (z0, z1) = lc.cfg.input_cuboid('greater')
    lo, hi = np.array([x0, y0, z0]), np.array([x1, y1, z1])
    xyz = rng.uniform(lo, hi, size=(m, 3)).astype(np.float32)
    feats = (0.5 * rng.normal(size=(m, ia['d_latent_local']))).astype(np.float32)
    fglob = (0.3 * rng.normal(size=(ia['d_latent'] - ia['d_latent_local'],))).astype(np.float32)
    q = np.concatenate([rng.uniform(lo, hi, size=(case.nq, 3)), rng.integers(0, 12, size=(case.nq, 1))], axis=1).astype(np.float32)
    sd = lc.cfg.fill_state_dict(lc.cfg.decoder_param_shapes(ia), case.seed + 1000)
    return dict(q=np.ascontiguousarray(q[:, :ia['d_in']]), abstract=np.concatenate([xyz, feats], axis=1), fglob=fglob, sd=sd)


def _net(case, device):
    h = _inputs(case)
    net = pk.implicit.LocalPclResnetFC(**case.ia)
    net.load_state_dict(h['sd'])
    if case.use_at is not None:
        net.use_pt_inds = dict(case.use_at)
    net = net.to(device).eval()
    q, ab, fg = (lc.dev(h[k], device) for k in ('q', 'abstract', 'fglob'))
    assert ab.shape[0] == 20 and q.shape[0] == 300
    return net, q, ab, fg


@pytest.mark.parametrize('case', DECODER_CASES, ids=lc.case_id)
def test_decoder_default_routing_equals_the_standalone_passes(case):
    device = torch.device('cuda:0')
    net, q, ab, fg = _net(case, device)
    nan = lambda: torch.full((q.shape[0], case.ia['d_out']), float('nan'), device=device)
    outs = {}
    with torch.no_grad():
        for shadow in (True, False):
            with pk.kernels(linz_shadow=shadow):
                outs[shadow] = net.forward_output_only(q, ab, fg, None, nan())
                # the penult output keeps every term on the stand-alone pass, whatever the selection
                outs[shadow, 'pen'] = net(q, ab, fg, None)
    assert torch.isfinite(outs[True]).all()
    assert torch.equal(outs[True], outs[False])
    assert torch.equal(outs[True, 'pen'][0], outs[False, 'pen'][0]) and torch.equal(outs[True, 'pen'][1], outs[False, 'pen'][1])
    assert torch.equal(outs[True, 'pen'][0], outs[True])


def test_selection_bit_and_workspace():
    """The opt-out is one bit beside the OCC4D_PATH_* table; the default selection's flags stay 0; fused_interp is accepted
    and changes no result; the workspace query sees the dense slice of the default routing, and only there."""
    import ctypes as C
    K, L = pk.kernels, pk._lib
    bit = L.LINZ_CONSTANTS['PATH_STANDALONE']
    assert K.Selection().flags() == 0 and K.Selection(linz_shadow=False).flags() == bit
    assert bit & (bit - 1) == 0 and not any(bit & v for k, v in L.CONSTANTS.items() if k.startswith('PATH_'))
    case = DECODER_CASES[0]
    device = torch.device('cuda:0')
    net, q, ab, fg = _net(case, device)
    nan = lambda: torch.full((q.shape[0], case.ia['d_out']), float('nan'), device=device)
    with torch.no_grad():
        base = net.forward_output_only(q, ab, fg, None, nan())
        with pk.kernels(fused_interp=True):
            assert torch.equal(net.forward_output_only(q, ab, fg, None, nan()), base)
    n, m = q.shape[0], ab.shape[0]
    size = lambda w, flags: int(L.lib().occ4d_decoder_query_workspace_floats(C.byref(w), n, m, flags))
    w = net.path_weights()[0]
    assert size(w, 0) == size(w, bit) + n * 416
    assert size(w, L.PATH_TRUNK4) == size(w, L.PATH_TRUNK4 | bit)          # (no placement under trunk4: no slice)
