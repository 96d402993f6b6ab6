"""GPU: consecutive residual blocks of the decoder trunk as one launch (include/ext/occ4d_chain.h, csrc/trunk.hip).

occ4d_resblock_chain_f32 runs up to three residual blocks (and optionally the "rows"-packed Linear behind them) over rows that
stay in registers, occ4d_interp_dense_f32 forms the lin_z terms of such a run in one pass, and the decoder routes maximal runs
of blocks through them by default.  All of it is held to `torch.equal` against the launches it replaces -- ops.resblock
(with and without addrows), ops.rowlin, ops.interp_add -- because the chain runs their loop bodies in their order.

Shapes: rows one short of, at and one past the 16-row wave tile and the 128-row workgroup tile, and 300 (three workgroups);
tails of 32 (one stage), 96 (an odd stage count) and 832 outputs (the decoder's merged query projection); tables of 8 rows
(= k: every row is a neighbour of every query) and 37.  No test here measures time."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import decoder_layout_cases as lc
import occlusions4d_amd as pk
from test_gpu_trunk import H, _weights

pytestmark = pytest.mark.gpu
ROWS = [1, 15, 16, 17, 127, 128, 129, 300]
TAILS = [None] + [(n_out, relu_in) for n_out in (32, 96, 832) for relu_in in (0, 1)]
_SHARED = {}


def _blocks():
    """Three residual blocks' packed weights and the three tail Linears: made once, read-only."""
    if 'blocks' not in _SHARED:
        rng = np.random.default_rng(90)
        blocks = []
        for _ in range(3):
            w0, b0 = _weights(rng, H)
            w1, b1 = _weights(rng, H)
            blocks.append((pk.ops.pack_trunk_rows(w0), b0, pk.ops.pack_trunk_cols(w1), b1))
        tails = {}
        for n_out in (32, 96, 832):
            wt, bt = _weights(rng, n_out)
            tails[n_out] = (pk.ops.pack_trunk_rows(wt), bt)
        _SHARED['blocks'] = (blocks, tails)
    return _SHARED['blocks']


@pytest.mark.parametrize('n', ROWS)
def test_chain_equals_the_launches_it_replaces(n):
    blocks, tails = _blocks()
    rng = np.random.default_rng(n)
    x = torch.from_numpy(rng.normal(size=(n, H)).astype(np.float32)).cuda()
    # dense rows as row views of stride 420, one set per position
    adds = [torch.from_numpy(rng.normal(size=(n, H + 4)).astype(np.float32)).cuda()[:, :H] for _ in range(3)]
    for nb in (1, 2, 3):
        for pattern in itertools.product((False, True), repeat=nb):
            want = x
            for i in range(nb):
                want = pk.ops.resblock(want, *blocks[i], addrows=adds[i] if pattern[i] else None)
            chain = [blocks[i] + (adds[i] if pattern[i] else None,) for i in range(nb)]
            for tail in TAILS:
                what = 'n=%d nb=%d addrows=%s tail=%s' % (n, nb, pattern, tail)
                if tail is None:
                    got = pk.ops.resblock_chain(x, chain)
                    assert torch.equal(got, want), what
                    buf = x.clone()                                 # y aliasing x
                    assert pk.ops.resblock_chain(buf, chain, out=buf) is buf and torch.equal(buf, want), what
                    continue
                n_out, relu_in = tail
                wt, bt = tails[n_out]
                want_tail = pk.ops.rowlin(want, wt, bt, n_out, relu_in=bool(relu_in))
                got, got_tail = pk.ops.resblock_chain(x, chain, tail=(wt, bt, n_out, relu_in))
                assert torch.equal(got, want) and torch.equal(got_tail, want_tail), what
                buf = x.clone()
                got, got_tail = pk.ops.resblock_chain(buf, chain, out=buf, tail=(wt, bt, n_out, relu_in))
                assert got is buf and torch.equal(buf, want) and torch.equal(got_tail, want_tail), what
    assert torch.isfinite(want).all()


def _terms(rng, n, d, m):
    """Three tables side by side in one (m, 3 d + 4) buffer (row views of one stride), three constants, lists that repeat an
    index, weights with zeros and negative entries, an all-zero weight row."""
    tab = torch.from_numpy(rng.normal(size=(m, 3 * d + 4)).astype(np.float32)).cuda()
    zc = torch.from_numpy(rng.normal(size=(3, d)).astype(np.float32)).cuda()
    idx = rng.integers(0, m, size=(n, 8)).astype(np.int32)
    idx[:, 1] = idx[:, 0]
    w = rng.uniform(-0.5, 1.0, size=(n, 8)).astype(np.float32)
    w[:, 2] = 0.0
    w[0, :] = 0.0
    w /= np.abs(w).sum(1, keepdims=True).clip(1e-12)
    return [(zc[t], tab[:, t * d:(t + 1) * d]) for t in range(3)], torch.from_numpy(idx).cuda(), torch.from_numpy(w).cuda()


@pytest.mark.parametrize('n', ROWS)
def test_interp_dense_equals_the_passes(n):
    for d, m in ((H, 8), (H, 37), (96, 37)):
        rng = np.random.default_rng(1000 * m + d + n)
        terms, idx, w = _terms(rng, n, d, m)
        x = torch.from_numpy(rng.normal(size=(n, d)).astype(np.float32)).cuda()
        want_x = pk.ops.interp_add(x.clone(), terms[0][0], terms[0][1], idx, w)
        want_d = [pk.ops.interp_add(torch.zeros((n, d), device='cuda'), t[0], t[1], idx, w) for t in terms]
        for present in itertools.product((False, True), repeat=3):
            if not any(present):
                continue
            what = 'n=%d d=%d m=%d terms=%s' % (n, d, m, present)
            buf = x.clone() if present[0] else None
            got = pk.ops.interp_dense(buf, [terms[t] if present[t] else None for t in range(3)], idx, w)
            if present[0]:
                assert got[0] is buf and torch.equal(buf, want_x), what
            for t in (1, 2):
                if present[t]:
                    assert torch.equal(got[t], want_d[t]), what
                else:
                    assert got[t] is None, what
        # dense rows as row views of wider buffers
        wide = [torch.zeros((n, d + 8), device='cuda') for _ in range(2)]
        buf = x.clone()
        pk.ops.interp_dense(buf, terms, idx, w, dense=(wide[0][:, :d], wide[1][:, 8:]))
        assert torch.equal(buf, want_x) and torch.equal(wide[0][:, :d], want_d[1]) and torch.equal(wide[1][:, 8:], want_d[2])
        assert not wide[0][:, d:].any() and not wide[1][:, :8].any()


def test_contracts():
    """Each violation is rejected with the library's message (an AssertionError of _lib.check), not launched."""
    blocks, tails = _blocks()
    rng = np.random.default_rng(7)
    n = 17
    x = torch.from_numpy(rng.normal(size=(n, H)).astype(np.float32)).cuda()
    add = torch.from_numpy(rng.normal(size=(n, H)).astype(np.float32)).cuda()
    blk = blocks[0] + (None,)
    for bad in ([], [blk] * 4):
        with pytest.raises(AssertionError, match='nb = %d blocks' % len(bad)):
            pk.ops.resblock_chain(x, bad)
    out = torch.zeros((n, H), device='cuda')
    with pytest.raises(AssertionError, match='addrows must not alias y'):
        pk.ops.resblock_chain(x, [blk, blocks[1] + (out,)], out=out)
    assert not out.any()                                        # rejected, not run
    keep = x.clone()
    with pytest.raises(AssertionError, match='addrows must not alias y'):       # in place: y is x
        pk.ops.resblock_chain(x, [blocks[0] + (x,)], out=x)
    assert torch.equal(x, keep)
    odd = torch.zeros((n, H + 4), device='cuda')[:, 1:H + 1]    # 4 bytes off a 16-byte boundary
    with pytest.raises(AssertionError, match='16-byte aligned'):
        pk.ops.resblock_chain(odd, [blk])
    with pytest.raises(AssertionError, match='16-byte aligned'):
        pk.ops.resblock_chain(x, [blocks[0] + (odd,)])
    wt, bt = tails[96]
    with pytest.raises(AssertionError, match='n_tail = 48 must be a multiple of 32'):
        pk.ops.resblock_chain(x, [blk], tail=(wt, bt, 48, 0))
    # n ld_add >= 2^30 (32-bit row offsets): through the C ABI, with a row stride no tensor of this size has
    L = pk._lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    b0, b1 = blocks[0][1].contiguous(), blocks[0][3].contiguous()
    none6 = (None, None, None, None, None, 0)
    rc = L.occ4d_resblock_chain_f32(p(x), H, p(out), H, 1, p(blocks[0][0]), p(b0), p(blocks[0][2]), p(b1), p(add), ((1 << 30) // n + 4) // 4 * 4,
                                    *none6, *none6, None, None, 0, 0, None, 0, n, None)
    assert rc == pk._lib.EINVAL and b'below 2^30' in L.occ4d_last_error()
    assert not out.any()

    terms, idx, w = _terms(rng, n, H, 37)
    with pytest.raises(AssertionError, match='kz = 8'):
        pk.ops.interp_dense(x.clone(), terms[:1], idx[:, :3].contiguous(), w[:, :3].contiguous())
    with pytest.raises(AssertionError, match='no interpolation term'):
        pk.ops.interp_dense(None, [None, None, None], idx, w)
    buf = x.clone()
    with pytest.raises(AssertionError, match='must not alias'):
        pk.ops.interp_dense(buf, terms[:2], idx, w, dense=(buf, None))
    assert torch.equal(buf, x)
    with pytest.raises(AssertionError, match='16-byte aligned'):
        pk.ops.interp_dense(odd, terms[:1], idx, w)
    with pytest.raises(AssertionError, match='without its table'):
        pk.ops.interp_dense(x.clone(), terms[:1], idx, w, dense=(out, None))
    rc = L.occ4d_interp_dense_f32(p(buf), H, p(terms[0][0].contiguous()), p(terms[0][1]), None, None, None, 0, None, None, None, 0,
                                  1 << 26, 37, p(idx), p(w), 8, n, H, None)
    assert rc == pk._lib.EINVAL and b'below 2^30' in L.occ4d_last_error() and torch.equal(buf, x)
    for name in ('occ4d_resblock_chain_f32', 'occ4d_interp_dense_f32'):
        assert name in pk._lib.ADDON_SIGNATURES and name in pk._lib.CHAIN_SIGNATURES and hasattr(L, name)
    assert pk._lib.ADDON_HEADERS['CHAIN'] == 'ext/occ4d_chain.h'
    K = pk.kernels
    bit = pk._lib.CHAIN_CONSTANTS['PATH_SEPARATE']
    assert bit == 1024 and K.Selection().flags() == 0 and K.Selection(trunk_chain=False).flags() == bit
    assert not any(bit & v for k, v in pk._lib.CONSTANTS.items() if k.startswith('PATH_')) and bit != pk._lib.LINZ_CONSTANTS['PATH_STANDALONE']


# ---------------------------------------------------------------------------------------------------------------- decoder
def _case(name, n_blocks, layers, use_at, seed):
    return lc.C(name, 'override', lc._ia(n_blocks, layers), seed, use_at=use_at, nq=300)


DECODER_CASES = [
    lc.C('chain-b6c2', 'formula', lc._ia(6, 2), 102, nq=300),       # the published layout: runs of 3, 2 and 1 blocks
    lc.C('chain-b5c0', 'feature', lc._feature(5), 601, nq=300),      # no cross layer: a run of 5 splits into 3 + 2
    _case('chain-b6-at01', 6, 2, {0: 0, 1: 1}, 610),                # adjacent cross layers, then four blocks in a row: 3 + 1
    _case('chain-b6-at25', 6, 2, {2: 0, 5: 1}, 620),                # a cross layer behind the last block
    lc.C('chain-b1c1', 'formula', lc._ia(1, 1), 630, nq=300),       # one block
    lc.C('chain-b16c0', 'feature', lc._feature(16), 640, nq=300),    # more than three blocks in a row, five times over
]
M = 37


def _net(case, device):
    """The case's module on 37 abstract points (no tie screening: both sides of every comparison run the same searches)."""
    ia = case.ia
    rng = np.random.default_rng(case.seed)
    (x0, x1), (y0, y1), (z0, z1) = lc.cfg.input_cuboid('greater')
    lo, hi = np.array([x0, y0, z0]), np.array([x1, y1, z1])
    xyz = rng.uniform(lo, hi, size=(M, 3)).astype(np.float32)
    feats = (0.5 * rng.normal(size=(M, ia['d_latent_local']))).astype(np.float32)
    fglob = (0.3 * rng.normal(size=(ia['d_latent'] - ia['d_latent_local'],))).astype(np.float32)
    q = np.concatenate([rng.uniform(lo, hi, size=(case.nq, 3)), rng.integers(0, 12, size=(case.nq, 1))], axis=1).astype(np.float32)
    net = pk.implicit.LocalPclResnetFC(**ia)
    net.load_state_dict(lc.cfg.fill_state_dict(lc.cfg.decoder_param_shapes(ia), case.seed + 1000))
    if case.use_at is not None:
        net.use_pt_inds = dict(case.use_at)
    net = net.to(device).eval()
    return net, lc.dev(np.ascontiguousarray(q[:, :ia['d_in']]), device), lc.dev(np.concatenate([xyz, feats], axis=1), device), \
        lc.dev(fglob, device)


@pytest.mark.parametrize('case', DECODER_CASES, ids=lc.case_id)
def test_decoder_chains_equal_the_separate_launches(case):
    device = torch.device('cuda:0')
    net, q, ab, fg = _net(case, device)
    assert q.shape[0] == 300 and ab.shape[0] == M
    nan = lambda: torch.full((q.shape[0], case.ia['d_out']), float('nan'), device=device)
    outs = {}
    with torch.no_grad():
        for name, fields in (('default', {}), ('separate', dict(trunk_chain=False)), ('standalone', dict(linz_shadow=False))):
            with pk.kernels(**fields):
                outs[name] = net.forward_output_only(q, ab, fg, None, nan())
    assert torch.isfinite(outs['default']).all()
    assert torch.equal(outs['default'], outs['separate'])
    assert torch.equal(outs['default'], outs['standalone'])

    # the forward inside exactly the workspace the query function reports for the same flags: a guard behind it stays intact
    L = pk._lib.lib()
    guard = 4096
    for fields in ({}, dict(trunk_chain=False)):
        with torch.no_grad(), pk.kernels(**fields):
            sc = net.prepare_scene(ab, fg, None)
            w, prepared, flags = net.path_weights()
            n, m = q.shape[0], sc['m']
            size = int(L.occ4d_decoder_query_workspace_floats(C.byref(w), n, m, flags))
            assert size > 0
            ws = torch.full((size + guard,), -7.0, device=device)
            out = nan()
            p = lambda t: C.c_void_p(t.data_ptr())
            pk._lib.check(L.occ4d_decoder_query_fwd_f32(C.byref(w), p(prepared), p(sc['scene']), m, p(q), q.stride(0), n, None, None,
                                                        p(out), out.stride(0), None, 0, p(ws), flags, None,
                                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
        assert torch.equal(out, outs['default']), fields
        assert bool((ws[size:] == -7.0).all()), fields
