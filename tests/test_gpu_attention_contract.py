"""The four fused vector-attention entry points of include/occ4d.h, called directly (ops.pt_cross_attn, ops.pt_cross_attn16p;
occ4d_pt_self_attn16_f32 and occ4d_pt_cross_attn16p_logits_f32 through the header-derived ctypes signatures), against the
fp64 statement of their contract (tests/attention_contract.py) at the edges the path-level callers never reach: padded row
strides cut out of buffers of noise, neighbour lists no kNN produces, every k, ragged n, more than one dispatch round,
saturated / underflowing / uniform softmax, and the exact footprint of every output.

Tolerance of a case: max(4 E32, 16 2^-24 S) with E32 = max|fp32-CPU - fp64| and S = max|fp64| from the reference alone
(attention_contract.bound; tests/test_attention_contract_reference.py pins it below 2e-5 max(1, S) without a GPU).

Measured on an MI355X (agg: E32, bound, kernel error, kernel error with permuted lists; then the worst kernel error / bound
over logits, a_out, pe_out of the _logits entry).  No margin was widened.

    case                                                 E32     bound    kernel  permuted  pairs
    16p_d416_n1_m76_k14_uniform_init                2.61e-07  2.12e-06   2.5e-07  2.47e-07  0.43
    16p_d416_n8_m14_k13_repeat_init                 1.01e-06  4.85e-06  7.34e-07  8.24e-07  0.28
    16p_d416_n9_m531_k8_uniform_saturated           1.21e-06  4.84e-06  1.81e-06   1.8e-06  0.49
    16p_d416_n10_m4096_k5_ends_init                 7.01e-07  3.64e-06  6.81e-07  6.81e-07  0.44
    16p_d416_n17_m76_k2_one_init                    7.15e-07  6.12e-06  9.75e-07  9.75e-07  0.49
    16p_d416_n19_m1_k1_one_init                     5.34e-07  4.96e-06  6.34e-07  6.34e-07  0.82
    16p_d416_n19_m14_k14_one_init                   1.17e-06  6.61e-06  1.33e-06  1.33e-06  0.32
    16p_d416_n130_m531_k14_uniform_saturated        1.85e-06  7.39e-06  2.81e-06   2.8e-06  0.37
    16p_d416_n1003_m76_k13_distinct_underflow       1.31e-06  7.44e-06  1.31e-06  1.31e-06  0.62
    16p_d416_n1003_m76_k5_one_init                  1.34e-06  6.96e-06  1.35e-06  1.35e-06  0.42
    16p_d416_n10_m4096_k8_uniform_equal             3.95e-07  3.88e-06  3.95e-07  3.51e-07  0.20
    16p_d416_n17_m531_k5_distinct_underflow         7.13e-07   5.5e-06  1.03e-06  1.03e-06  0.52
    16p_d416_n9_m1_k14_one_init                     1.23e-06   5.2e-06  8.45e-07  8.45e-07  0.25
    16p_d416_n8_m14_k2_ends_saturated               2.26e-07  9.05e-07  6.21e-07  6.21e-07  0.61
    16p_d416_n19_m76_k14_repeat_init                7.23e-07  3.62e-06  5.28e-07  5.21e-07  0.38
    16p_d416_nrounds_m4099_k14_uniform_init            1e-06  5.15e-06  8.49e-07  7.34e-07  -
    first_d288_n19_m76_k14_uniform_init             6.88e-07  3.39e-06  5.34e-07  4.84e-07  -
    first_d288_n10_m531_k5_uniform_saturated        1.06e-06  4.23e-06   1.1e-06   1.1e-06  -
    first_d288_n10_m14_k5_repeat_init               5.66e-07  4.11e-06  4.26e-07  4.86e-07  -
    first_d288_n1003_m14_k13_one_init               1.86e-06  7.42e-06  1.64e-06  1.64e-06  -
    first_d288_n9_m1_k1_one_init                    4.25e-07  5.32e-06  5.23e-07  5.23e-07  -
    first_d416_n17_m76_k8_uniform_init               5.7e-07  4.74e-06  7.77e-07  7.12e-07  -
    first_d416_n1003_m531_k14_distinct_underflow    1.26e-06     8e-06  1.28e-06  1.28e-06  -
    first_d416_n1_m4096_k2_ends_equal               3.12e-07  4.06e-06  3.14e-07  3.14e-07  -
    first_d416_n8_m76_k13_one_init                  1.18e-06  4.71e-06  8.95e-07  8.95e-07  -
    self_d4_n1_m1_k16_one_init                      2.49e-07  2.21e-06  9.55e-08  9.55e-08  -
    self_d20_n3_m76_k16_uniform_saturated           1.42e-07  5.68e-07  2.13e-07  2.13e-07  -
    self_d36_n4_m76_k16_repeat_init                  5.4e-07  3.35e-06  2.63e-07  2.27e-07  -
    self_d72_n5_m5_k16_uniform_equal                 2.9e-07   2.6e-06  2.42e-07  2.42e-07  -
    self_d100_n16_m16_k16_distinct_underflow        6.24e-07  6.78e-06  7.25e-07  7.25e-07  -
    self_d144_n1001_m1001_k16_uniform_init           6.2e-07  3.55e-06  4.95e-07  5.38e-07  -
    self_d260_n16_m531_k16_uniform_saturated        9.13e-07  3.65e-06  1.81e-06  1.83e-06  -
    self_d20_n3_m3_k16_ends_init                    4.29e-07  3.73e-06  3.61e-07  3.61e-07  -
    self_d288_n16_m76_k16_uniform_saturated         1.51e-06  6.03e-06  2.44e-06  2.43e-06  -
    self_d288_n1001_m76_k16_uniform_init            9.93e-07  4.29e-06  5.53e-07  6.15e-07  -
    self_d36_n1001_m1001_k16_distinct_underflow     7.39e-07  6.53e-06  7.94e-07  7.94e-07  -
    self_d288_n5_m4096_k16_uniform_init             3.78e-07  2.67e-06  3.62e-07  3.82e-07  -
    self_d4_n1001_m14_k16_one_init                  9.68e-07  3.92e-06  7.02e-07  7.02e-07  -
"""
import numpy as np
import pytest
import torch

import attention_contract as ac

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FA5C3D1          # a NaN bit pattern no kernel computes: what every float outside an output must still hold
GUARD_ROWS = 12


@pytest.fixture(scope='module')
def pk():
    import occlusions4d_amd
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    occlusions4d_amd._lib.lib()
    return occlusions4d_amd


def _cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _sentinel(rows, cols):
    return torch.full((rows, cols), SENTINEL, dtype=torch.int32, device='cuda').view(torch.float32)


def _untouched(buf, rows, off, cols):
    """Every float of `buf` outside [0, rows) x [off, off + cols) still holds the sentinel."""
    bits = (buf.view(torch.int32) != SENTINEL)
    bits[:rows, off:off + cols] = False
    return not bool(bits.any())


def _cut(arr, ld, off, rng):
    """`arr` as a view (row stride ld, first column `off`) of a wider buffer of noise with rows of noise behind it."""
    rows, w = arr.shape
    assert off + w <= ld
    wide = rng.normal(size=(rows + 3, ld)).astype(np.float32)
    wide[:rows, off:off + w] = arr
    return torch.from_numpy(wide).cuda()[:rows, off:off + w]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Laid:
    """The operands of a case on the device in a strided layout, and a fresh guarded output per run."""

    def __init__(self, op, layout, aligned_values):
        rng = np.random.default_rng(5)
        pa, pk_, pv, self.pad_agg, qs, as_ = layout
        n, d = op['aq'].shape[0], op['vt'].shape[1]
        self.n, self.m, self.k, self.d = n, op['kt'].shape[0], op['idx'].shape[1], d
        self.ld = dict(aq=2 * d + pa, kt=2 * d + pk_, vt=d + pv, agg=d + self.pad_agg, qpos=qs, apos=as_)
        self.off_v = 4 if aligned_values else 1                   # first column of vt / agg inside their buffers
        self.aq = _cut(op['aq'], self.ld['aq'], 4, rng)
        self.kt = _cut(op['kt'], self.ld['kt'], 4, rng)
        self.vt = _cut(op['vt'], self.ld['vt'], min(self.off_v, pv), rng)
        self.qpos = _cut(op['qpos'], qs, 0, rng)
        self.apos = _cut(op['apos'], as_, 0, rng)
        assert self.aq.data_ptr() % 16 == 0 and self.kt.data_ptr() % 16 == 0
        self.divisor = op['divisor']
        self.w = {k: _dev(op[k]) for k in ('P1', 'c1', 'wp', 'w2', 'p2', 'c2')}
        self.w['b2'] = _dev(op['b2']) if op.get('b2') is not None else None
        self.idx = _dev(op['idx'])

    def out(self):
        off = min(self.off_v, self.pad_agg)
        buf = _sentinel(self.n + GUARD_ROWS, self.ld['agg'])
        return buf, buf[:self.n, off:off + self.d], off


def _err(got, ref):
    return float(np.abs(got.double().cpu().numpy() - ref).max())


def _layout(case, layouts):
    return layouts[ac.ALL_CASES.index(case) % len(layouts)]


def _permuted(op, seed=3):
    rng = np.random.default_rng(seed)
    idx = np.stack([row[rng.permutation(row.size)] for row in op['idx']])
    return dict(op, idx=np.ascontiguousarray(idx, dtype=np.int32))


def _report(name, what, e32, b, err):
    print('\n[attn-contract] %-46s %-12s E32 %.3g  bound %.3g  kernel %.3g' % (name, what, e32, b, err))


def _check_regime_outputs(case, got, r64, b):
    assert torch.isfinite(got).all()
    if case['regime'] == 'underflow' or case['lists'] == 'one':
        # one neighbour carries the whole weight (or all of them are the same point): agg = vt[j] + pe
        assert _err(got, r64['dom']) <= b


# ------------------------------------------------------------------------------------------ cross attention, d = 416 / 288
def _run_cross(pk, case, L, idx=None, skew=None, ws=None):
    buf, out, off = L.out()
    idx = L.idx if idx is None else idx
    w = L.w
    if case['kernel'] == '16p':
        pk.ops.pt_cross_attn16p(L.aq, L.qpos, L.apos, idx, L.kt, L.vt, w['P1'], w['c1'], ws, out=out, skew=skew)
    else:
        pk.ops.pt_cross_attn(L.aq, L.qpos, L.apos, idx, L.kt, L.vt, w['P1'], w['c1'], w['wp'], w['w2'], w['b2'], w['p2'],
                             w['c2'], out=out)
    torch.cuda.synchronize()
    assert _untouched(buf, L.n, off, L.d), 'the kernel wrote outside its (n, d) output'
    return out


def _run_logits(pk, L, ws, pairs, skew=6):
    """occ4d_pt_cross_attn16p_logits_f32 through the header-derived signature; every output with guard rows behind it."""
    lib, P = pk._lib.lib(), pk.ops._ptr
    nk = L.n * L.k
    buf, out, off = L.out()
    lg = _sentinel(nk + GUARD_ROWS, L.d)
    a = _sentinel(nk + GUARD_ROWS, 2 * L.d) if pairs else None
    pe = _sentinel(nk + GUARD_ROWS, L.d) if pairs else None
    w = L.w
    pk._lib.check(lib.occ4d_pt_cross_attn16p_logits_f32(
        P(L.aq), L.ld['aq'], P(L.qpos), L.ld['qpos'], P(L.apos), L.ld['apos'], P(L.idx), P(L.kt), L.ld['kt'], P(L.vt),
        L.ld['vt'], P(w['P1']), P(w['c1']), P(ws), P(out), L.ld['agg'], P(lg), P(a), P(pe), P(w['c2'] if pairs else None),
        L.n, L.m, L.k, L.d, L.divisor, skew, pk.ops._stream()))
    torch.cuda.synchronize()
    assert _untouched(buf, L.n, off, L.d), 'agg: written outside (n, d)'
    assert _untouched(lg, nk, 0, L.d), 'logits: written behind row n k'
    if pairs:
        assert _untouched(a, nk, 0, 2 * L.d) and _untouched(pe, nk, 0, L.d), 'a_out / pe_out: written behind row n k'
    return out, lg[:nk], (a[:nk] if pairs else None), (pe[:nk] if pairs else None)


@pytest.mark.parametrize('case', ac.CROSS_CASES, ids=lambda c: c['name'])
def test_cross_attention_entry_points_match_the_fp64_contract(pk, case):
    op = ac.make_operands(case, _cu_count())
    if case['n'] == 'rounds':
        assert -(-op['aq'].shape[0] // 9) > 2 * _cu_count() and op['aq'].shape[0] % 9
    pairs_ref = case['kernel'] == '16p' and case['n'] != 'rounds'
    op, r64, r32, bounds = ac.case_bounds(case, op, want_pairs=pairs_ref)
    ac.check_regime(case, op, r64, r32)
    e32, s, b = bounds['agg']
    assert b <= ac.CHAIN_TOL * max(1.0, s)
    L = Laid(op, _layout(case, ac.CROSS_LAYOUTS), aligned_values=False)
    w = L.w
    ws = pk.ops.pack_attn16p_stream(w['w2'], None, w['wp'], w['p2'], None) if case['kernel'] == '16p' else None
    got = _run_cross(pk, case, L, ws=ws)
    err = _err(got, r64['agg'])
    _report(case['name'], 'agg', e32, b, err)
    assert err <= b
    _check_regime_outputs(case, got, r64, b)
    # a row's neighbours in another order: the same sum (the 9th query's slots move between waves and passes)
    perm = _run_cross(pk, case, L, idx=_dev(_permuted(op)['idx']), ws=ws)
    err_p = _err(perm, r64['agg'])
    _report(case['name'], 'agg permuted', e32, b, err_p)
    assert err_p <= b
    if case['kernel'] != '16p':
        return
    # skew is performance only
    for skew in (0, 6, 64):
        assert torch.equal(_run_cross(pk, case, L, skew=skew, ws=ws), got), 'skew = %d changes agg' % skew
    # the training forward: the same agg bit for bit, with and without the pair tensors
    agg1, lg1, _, _ = _run_logits(pk, L, ws, pairs=False)
    agg2, lg2, a2, pe2 = _run_logits(pk, L, ws, pairs=True)
    assert torch.equal(agg1, got) and torch.equal(agg2, got)
    assert torch.equal(lg1, lg2)
    if pairs_ref:
        for key, t in (('logits', lg2), ('a', a2), ('pe', pe2)):
            e32_t, s_t, b_t = bounds[key]
            assert b_t <= ac.CHAIN_TOL * max(1.0, s_t)
            err_t = _err(t, r64[key])
            _report(case['name'], key, e32_t, b_t, err_t)
            assert err_t <= b_t, key


# ------------------------------------------------------------------------------------------ self attention, k = 16
def _run_self(pk, L, idx=None):
    lib, P = pk._lib.lib(), pk.ops._ptr
    buf, out, off = L.out()
    w = L.w
    for t in (L.aq, L.kt, L.vt, out, w['wp'], w['w2'], w['p2'], w['c2']):
        assert t.data_ptr() % 16 == 0
    pk._lib.check(lib.occ4d_pt_self_attn16_f32(
        P(L.aq), L.ld['aq'], P(L.qpos), L.ld['qpos'], P(L.apos), L.ld['apos'], P(L.idx if idx is None else idx), P(L.kt),
        L.ld['kt'], P(L.vt), L.ld['vt'], P(w['P1']), P(w['c1']), P(w['wp']), P(w['w2']), P(w['p2']), P(w['c2']), P(out),
        L.ld['agg'], L.n, L.m, 16, L.d, L.divisor, pk.ops._stream()))
    torch.cuda.synchronize()
    assert _untouched(buf, L.n, off, L.d), 'the kernel wrote outside its (n, d) output'
    return out


@pytest.mark.parametrize('case', ac.SELF_CASES, ids=lambda c: c['name'])
def test_self_attention_entry_point_matches_the_fp64_contract(pk, case):
    op, r64, r32, bounds = ac.case_bounds(case)
    ac.check_regime(case, op, r64, r32)
    e32, s, b = bounds['agg']
    assert b <= ac.CHAIN_TOL * max(1.0, s)
    L = Laid(op, _layout(case, ac.SELF_LAYOUTS), aligned_values=True)
    got = _run_self(pk, L)
    err = _err(got, r64['agg'])
    _report(case['name'], 'agg', e32, b, err)
    assert err <= b
    _check_regime_outputs(case, got, r64, b)
    err_p = _err(_run_self(pk, L, idx=_dev(_permuted(op)['idx'])), r64['agg'])
    _report(case['name'], 'agg permuted', e32, b, err_p)
    assert err_p <= b


# ------------------------------------------------------------------------------------------ 32-bit row offsets
def test_16p_entries_reject_rows_beyond_32_bit_byte_offsets(pk):
    """The 16p kernels address aq / kt rows by 32-bit byte offsets: n * ld_aq * 4 B or m * ld_kt * 4 B of 4 GiB and more is
    OCC4D_EINVAL (chunk the queries), not a silent read of wrapped rows.  Every buffer has its true size, so a call that
    slipped through would still compute in bounds."""
    free = torch.cuda.mem_get_info()[0]
    if free < 12 * 2 ** 30:
        pytest.skip('needs about 12 GiB of free device memory (a true-size 4 GiB operand), %.1f GiB free' % (free / 2 ** 30))
    lib, P, d, k = pk._lib.lib(), pk.ops._ptr, 416, 14
    rng = np.random.default_rng(9)
    w = {key: _dev(rng.normal(size=shape).astype(np.float32))
         for key, shape in (('P1', (32, 3)), ('c1', (32,)), ('wp', (2 * d, 32)), ('w2', (d, 2 * d)), ('p2', (d, 32)), ('c2', (d,)))}
    ws = pk.ops.pack_attn16p_stream(w['w2'], None, w['wp'], w['p2'], None)
    big, ld_big = 32768, 32768                                         # 32768 rows x 32768 floats x 4 B = 4 GiB exactly
    for n, m, ld_aq, ld_kt in ((big, 16, ld_big, 2 * d), (16, big, 2 * d, ld_big)):
        aq = torch.zeros((n, ld_aq), device='cuda')
        kt = torch.zeros((m, ld_kt), device='cuda')
        vt = torch.zeros((m, d), device='cuda')
        qpos, apos = torch.zeros((n, 3), device='cuda'), torch.zeros((m, 3), device='cuda')
        idx = torch.zeros((n, k), dtype=torch.int32, device='cuda')
        agg = torch.zeros((n, d), device='cuda')
        logits = torch.zeros((n * k, d), device='cuda')
        head = (P(aq), ld_aq, P(qpos), 3, P(apos), 3, P(idx), P(kt), ld_kt, P(vt), d, P(w['P1']), P(w['c1']), P(ws), P(agg), d)
        tail = (n, m, k, d, float(np.sqrt(np.float32(d))), 0, pk.ops._stream())
        for rc in (lib.occ4d_pt_cross_attn16p_f32(*head, *tail),
                   lib.occ4d_pt_cross_attn16p_logits_f32(*head, P(logits), None, None, None, *tail)):
            assert rc == pk._lib.EINVAL
            msg = lib.occ4d_last_error().decode()
            assert '4 GiB' in msg and 'chunk' in msg, msg
        torch.cuda.synchronize()
        del aq, kt
