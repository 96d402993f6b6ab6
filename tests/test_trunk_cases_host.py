"""No GPU: what tests/test_gpu_trunk_edges.py rests on, checked on the host first.  The case matrix reaches every entry point,
row count and width it claims; the exact cases satisfy their preconditions (sum|term| < 2^24 at every layer, integer results);
no regime leaves the range it promises; a numpy float32 evaluation of every case (tc.HostOps, numpy's blocked matrix product --
another summation order than the kernels') passes the driver, the frame check and the bound of every case, so the references
alone stay inside the bounds; and every check rejects the mutants of the reference it is there to catch: no check_* of
tests/trunk_cases.py can pass vacuously."""
import numpy as np
import pytest

import trunk_cases as tc

F32, U, H = np.float32, tc.U, tc.H
CPU = 'cpu'
OPS = tc.HostOps()


# ---------------------------------------------------------------------------------------------------------------- the matrix
def test_the_matrix_reaches_what_it_claims():
    calls = [c for e, p, n in tc.FRAME_CALLS for c in tc.entry_calls(e, p, n)]
    assert len({tc.call_id(c) for c in calls}) == len(calls)
    by = lambda e, p: [c for c in calls if c.entry == e and c.pack == p]       # noqa: E731
    for pack in (tc.FULL, tc.HALF):
        assert {c.n for c in by('resblock', pack)} == set(tc.ROWS[pack]) == {c.n for c in by('rowlin', pack)}
        assert {c.n_out for c in by('rowlin', pack)} == set(tc.WIDTHS[pack])
        assert {c.opts for c in by('resblock', pack)} >= {(), ('inplace',), ('interp8',), ('interp3',)}
        opts = {c.opts for c in by('rowlin', pack)}
        assert opts >= {(), ('relu',), ('res',), ('alias', 'res'), ('interp', 'res'), ('mask',)}
        assert (('mask', 'skip') in opts) == (pack == tc.HALF)
    assert ('addrows',) in {c.opts for c in by('resblock', tc.FULL)}
    linz = by('linz', tc.FULL)
    assert {c.opts for c in linz} == {('term',), ('term2',), ('res', 'term', 'term2'), ('alias', 'res', 'term', 'term2')}
    assert {c.n_out for c in linz} == set(tc.WIDTHS[tc.FULL]) and {c.n for c in linz} == set(tc.ROWS[tc.FULL])
    chain = by('chain', tc.FULL)
    assert {(c.nb, 'adds' in c.opts, c.tail, 'inplace' in c.opts) for c in chain} == {
        (nb, a, t, i) for nb in (1, 2, 3) for a in (False, True) for t in (0, 32, 832) for i in (False, True)}
    assert {'trelu' in c.opts for c in chain if c.tail} == {False, True}
    assert {c.n for c in by('dense', tc.FULL)} == set(tc.ROWS[tc.FULL])
    # every operand of a call has a row stride of its own
    assert len({tc.SLOT[k] for k in ('x', 'y', 'res', 'mask', 'addrows', 'ztab', 'dense', 'y_tail')}) == 8
    for regime in tc.REGIMES:
        rc = tc.regime_calls(regime)
        assert {(c.entry, c.pack) for c in rc} >= {('rowlin', tc.FULL), ('rowlin', tc.HALF), ('linz', tc.FULL), ('resblock', tc.FULL)}
        assert any('addrows' in c.opts for c in rc) and {c.n for c in rc} == {17, 65, 129}
        plain = ('interp8',) if regime == 'cancel' else ()
        assert {c.pack for c in rc if c.entry == 'resblock' and c.opts == plain} == {tc.FULL, tc.HALF}


def _operands(h):
    out = [h['x']] + [a for l in h['layers'] for a in l[:2]] + [a for a in h['adds'] if a is not None]
    return out + [h[k] for k in ('res', 'skip', 'tabs', 'zc', 'zw') if k in h]


@pytest.mark.parametrize('regime', tc.REGIMES)
def test_no_regime_leaves_its_range(regime):
    """Every non-zero operand has a magnitude in [2^-40, 2^40] (no subnormal can arise from two of them), the regime does what
    its name says, and the fp64 results are finite."""
    for c in tc.regime_calls(regime):
        h = tc.inputs(c)
        for a in _operands(h):
            nz = np.abs(a[a != 0]).astype(np.float64)
            assert a.dtype == F32 and (nz.size == 0 or (nz.min() >= 2.0 ** -40 and nz.max() <= 2.0 ** 40)), tc.call_id(c)
        refs, _ = tc.reference(c, h)
        assert all(np.isfinite(r.ref).all() and np.isfinite(r.bound).all() and (r.bound >= 0).all() for r in refs.values())
        base = tc.inputs(c._replace(regime='init'))
        if regime in ('small_x', 'big_x'):
            s = F32(2.0 ** (-12 if regime == 'small_x' else 12))
            assert np.array_equal(h['x'], base['x'] * s) and ('res' not in h or np.array_equal(h['res'], base['res'] * s))
        if regime == 'big_w':
            assert all(np.array_equal(a[0], b[0] * F32(64)) and np.array_equal(a[1], b[1]) for a, b in zip(h['layers'], base['layers']))
        if regime == 'mixed_rows':
            e = np.log2(np.abs(h['x'][:, 0] / base['x'][:, 0]))
            assert e.min() == -12 and e.max() == 12 and np.abs(np.diff(e[:16])).max() == 24
        if regime == 'dead_rows':
            assert (h['x'][::3] <= 0).all() and (h['x'][1::3] > 0).any()
        if regime == 'cancel':
            y = refs['y']
            live = y.bound > 0
            full = tc.reference(c._replace(regime='init'), base)[0]['y']
            # the output is rounding residue: orders of magnitude below the terms it is the sum of, and the bound stays theirs
            # (rowlin_linz adds its first term to res + W a + b = residue: what is left is the term and that residue)
            left = y.ref - tc.term64(h, 0)[0] if c.entry == 'linz' else y.ref
            assert np.median(np.abs(left[live])) < 1e-5 * np.median(np.abs(full.ref[live])), tc.call_id(c)
            assert np.median(y.bound[live]) > 0.5 * np.median(full.bound[live])


def test_exact_cases_are_exact():
    """sum|term| < 2^24 at every layer and integer results: every fp32 evaluation, in any order, gives the fp64 value."""
    worst = {}
    for c in tc.exact_calls():
        h = tc.dense_inputs(c, tc.inputs(c))
        refs, mags = tc.reference(c, h)
        assert mags and all(m.max() < 2.0 ** 24 for m in mags), tc.call_id(c)
        for name, r in refs.items():
            assert np.array_equal(r.ref, np.rint(r.ref)) and np.abs(r.ref).max() < 2.0 ** 24, (tc.call_id(c), name)
        key = (c.entry, c.nb if c.entry == 'chain' else 0, c.tail)
        worst[key] = max(worst.get(key, 0.0), max(m.max() for m in mags))
        if c.entry in ('resblock', 'chain') and not c.opts:
            assert 0.2 < (refs['y'].ref != h['x']).mean()                    # the block does something: hidden units are alive
    print('\n[trunk] exact cases, largest sum|term| per (entry, blocks, tail): %s' % sorted(worst.items()))
    for c in tc.dead_calls():
        h = tc.inputs(c)
        hidden = tc.f64(np.maximum(h['x'], 0)) @ tc.f64(h['layers'][0][0]).T + tc.f64(h['layers'][0][1])
        assert hidden.max() < -2.0 ** 19, tc.call_id(c)
        if c.nb == 1 and h['adds'][0] is None:               # one rounding: the exact sum x + b1, rounded
            assert np.array_equal(tc.dead_expected(c, h), tc.reference(c, h)[0]['y'].ref.astype(F32)), tc.call_id(c)


# ---------------------------------------------------------------------------------------------------------------- float32 evaluations
@pytest.mark.parametrize('entry,pack,n', tc.FRAME_CALLS, ids=lambda v: str(v))
def test_float32_evaluation_passes_frames_and_bounds(entry, pack, n):
    worst = max(tc.run_and_check(OPS, CPU, c) for c in tc.entry_calls(entry, pack, n))
    print('\n[trunk] numpy float32 %s %s n=%d: worst error / bound %.3f' % (entry, pack, n, worst))
    assert worst <= 1.0


@pytest.mark.parametrize('regime', tc.REGIMES)
def test_float32_evaluation_holds_every_regime(regime):
    worst = max(tc.run_and_check(OPS, CPU, c) for c in tc.regime_calls(regime))
    print('\n[trunk] numpy float32, regime %s: worst error / bound %.3f' % (regime, worst))
    assert worst <= 1.0


def test_float32_evaluation_of_the_exact_cases():
    for c in tc.exact_calls():
        tc.run_and_check(OPS, CPU, c, 'exact')
    for c in tc.dead_calls():
        tc.run_and_check(OPS, CPU, c, 'dead')


def test_metamorphic_drivers_run():
    """The drivers of the bit-for-bit device checks, on the float32 evaluation (numpy's matrix product promises no order per row,
    so here the comparison is to fp32 rounding only; on the device it is tc.bits_equal)."""
    def close(a, b, what):
        assert a.shape == b.shape and np.abs(a.astype(np.float64) - b).max() <= 1e-4 * max(1.0, np.abs(b).max()), what
    for c in tc.METAMORPHIC:
        tc.row_position(OPS, CPU, c._replace(n=40), close)
    for c in tc.HOMOGENEOUS:
        def rel(a, b, what):
            scale = np.abs(b).max(axis=1, keepdims=True)
            assert (np.abs(a.astype(np.float64) - b) <= 1e-4 * scale).all(), what
        tc.homogeneity(OPS, CPU, c._replace(n=40), rel)
    with pytest.raises(AssertionError, match='depends on its position'):
        tc.row_position(OPS, CPU, tc.METAMORPHIC[0]._replace(n=40), lambda a, b, what: tc.bits_equal(a, a + F32(1), what))
    assert tc.tail_split_rows(256) == 32768 + 197
    for opts in ('interp res', 'mask skip'):
        assert tc.tail_split(OPS, CPU, 1, opts, close) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- mutants
def _mutants(c, h, refs):
    """Mutants of the fp64 reference of a rowlin_linz call with a residual and both terms, each of relative size 1."""
    (w, b, _), y = h['layers'][0], refs['y'].ref
    x64, w64, res = tc.f64(h['x']), tc.f64(w), tc.f64(h['res'])
    out = {}
    m = y.copy()
    m[:, [5, 37]] = y[:, [37, 5]]
    out['two output channels swapped'] = m
    m = y.copy()
    m[70] -= x64[70, 48:64] @ w64[:, 48:64].T
    out['a 16-wide k-group left out of one row'] = m
    out['the residual of row i + 1 used for row i'] = y - res + np.roll(res, -1, axis=0)
    m = y.copy()
    m[:, 64:96] -= tc.f64(b)[64:96]
    out['the bias of one 32-channel stage left out'] = m
    out['one neighbour weighted twice'] = y + tc.f64(h['zw'])[:, 3:4] * tc.f64(h['tabs'][0])[h['idx'][:, 3]]
    m = y.copy()
    m[128] = y[127]
    out['the last row of 129 equal to row 127'] = m
    return out


@pytest.mark.parametrize('regime', ['init', 'small_x'])
def test_value_checks_reject_the_mutants(regime):
    c = tc.call('linz', tc.FULL, 129, H, 'term term2 res', regime)
    h = tc.inputs(c)
    refs, _ = tc.reference(c, h)
    good = {name: r.ref.astype(F32) for name, r in refs.items()}
    assert tc.check_values(c, h, good, refs) <= 0.5                            # the rounded reference itself passes
    for what, m in _mutants(c, h, refs).items():
        with pytest.raises(AssertionError, match='outside the bound'):
            tc.check_values(c, h, dict(good, y=m.astype(F32)), refs)
        print('\n[trunk] %s, %s: rejected' % (regime, what))
    # the dense rows of the second term are checked too, every element of them
    bad = good['dense'].copy()
    bad[128, 415] += F32(1) * max(F32(1e-3), abs(bad[128, 415]))
    with pytest.raises(AssertionError, match='outside the bound'):
        tc.check_values(c, h, dict(good, dense=bad), refs)
    # a residual block: channels swapped, a hidden k-group of one row left out, b1 of one stage left out, the last row
    c = tc.call('resblock', tc.HALF, 129, H, '', regime)
    h = tc.inputs(c)
    refs, _ = tc.reference(c, h)
    y = refs['y'].ref
    hid = np.maximum(tc.f64(np.maximum(h['x'], 0)) @ tc.f64(h['layers'][0][0]).T + tc.f64(h['layers'][0][1]), 0)
    muts = [y.copy() for _ in range(4)]
    muts[0][:, [0, 415]] = y[:, [415, 0]]
    muts[1][3] -= hid[3, 32:48] @ tc.f64(h['layers'][1][0])[:, 32:48].T
    muts[2][:, 384:416] -= tc.f64(h['layers'][1][1])[384:416]
    muts[3][128] = y[127]
    assert tc.check_values(c, h, dict(y=y.astype(F32)), refs) <= 0.5
    for m in muts:
        with pytest.raises(AssertionError, match='outside the bound'):
            tc.check_values(c, h, dict(y=m.astype(F32)), refs)


def test_exact_checks_reject_one_ulp_and_a_wrong_cell():
    c = tc.call('rowlin', tc.HALF, 65, 112, 'mask skip', 'exact')
    h = tc.inputs(c)
    refs, _ = tc.reference(c, h)
    good = dict(y=refs['y'].ref.astype(F32))
    tc.check_exact(c, h, good)
    tc.check_masked(c, h, good)
    live = np.argwhere((h['mask'] > 0) & (good['y'] != 0))[0]
    bad = good['y'].copy()
    bad[tuple(live)] = np.nextafter(bad[tuple(live)], F32(np.inf))
    with pytest.raises(AssertionError, match='differ from the exact result'):
        tc.check_exact(c, h, dict(y=bad))
    bad = good['y'].copy()
    bad[c.n // 2, 7] += F32(1)                                               # a cell of the masked row that is not skip
    with pytest.raises(AssertionError, match='not exactly skip'):
        tc.check_masked(c, h, dict(y=bad))
    c = tc.call('resblock', tc.FULL, 17, H, 'addrows', 'dead')
    h = tc.inputs(c)
    want = tc.dead_expected(c, h)
    tc.check_dead(c, h, dict(y=want))
    # adding the rows in the other order, f32(x + add) + b1, is off by an ulp somewhere: rejected
    other = (h['x'] + h['adds'][0]) + h['layers'][1][1]
    assert other.dtype == F32 and not np.array_equal(other, want)
    with pytest.raises(AssertionError, match='not f32'):
        tc.check_dead(c, h, dict(y=other))


def test_frame_check_rejects_a_write_outside_the_view_and_a_hole_inside():
    c = tc.call('rowlin', tc.FULL, 17, 96, 'res')
    got, rec = tc.run_call(OPS, CPU, c, tc.inputs(c))
    tc.check_frames(rec, 'intact')
    name, bits, rows, off, cols = rec['outputs'][0]
    assert bits.shape == (17 + tc.GUARD_ROWS, 96 + 12) and (rows, off, cols) == (17, 4, 96)
    for at, why in (((5, off + cols), 'a padding column'), ((5, off - 1), 'the padding in front'), ((rows, off + 3), 'a guard row'),
                    ((rows + 1, 0), 'the last guard row')):
        bad = bits.copy()
        bad[at] = 0
        with pytest.raises(AssertionError, match='outside the view were written'):
            tc.check_frame(bad, rows, off, cols, why)
    bad = bits.copy()
    bad[rows - 1, off + cols - 1] = tc.SENTINEL
    with pytest.raises(AssertionError, match='were not written'):
        tc.check_frame(bad, rows, off, cols, 'the last element')
    # a written input: one float of the residual's frame, one of a bias
    for i, (name, before, after) in enumerate(rec['inputs']):
        changed = after.copy()
        changed.flat[changed.size - 1] ^= 1
        broken = dict(rec, inputs=rec['inputs'][:i] + [(name, before, changed)] + rec['inputs'][i + 1:])
        with pytest.raises(AssertionError, match='the input %s was written' % name):
            tc.check_frames(broken, 'written input')
    assert {name for name, _, _ in rec['inputs']} == {'x', 'res', 'w', 'b'}
    # the strides: x 416 + 8, y 96 + 12, res 96 + 16
    assert [b.shape[1] for _, b, _ in rec['inputs'][:1]] == [H + 8] and dict((n, b.shape) for n, b, _ in rec['inputs'])['res'] == (17, 96 + 16)
