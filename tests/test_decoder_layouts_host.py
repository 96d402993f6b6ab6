"""No GPU: what tests/test_gpu_decoder_layouts.py rests on, checked on the host first, and the decoder layouts through the g++ twin
(an independent implementation: plain fp32 loops over the reference's statements).  The restated reference against
oracle.path.decoder_forward bit for bit; the coverage of the case tables; the no-tie assertion and the bound rejecting what
they must; the three findings that can be shown without a device -- two cross layers behind one block (the later one shadows the
earlier one, as in the reference, instead of an AssertionError in path_weights), use_pt_inds decided after construction, and a
decoder without a global part on the twin."""
import numpy as np
import pytest
import torch

import decoder_layout_cases as dc
import occlusions4d_amd as pk
from oracle import path as op


@pytest.fixture
def twin():
    pk.cpu_twin.enable()
    try:
        yield pk
    finally:
        pk.cpu_twin.disable()


# ---------------------------------------------------------------------------------------------------------------- the reference
FORMULA_CASES = [c for c in dc.LAYOUT_CASES + dc.TRAIN_CASES if c.use_at is None]


@pytest.mark.parametrize('case', FORMULA_CASES, ids=dc.case_id)
def test_restated_reference_is_the_oracle_bit_for_bit(case):
    h = dc.inputs(case)
    for dtype in (torch.float32, torch.float64):
        sd = {k: v.to(dtype) for k, v in h['sd'].items()}
        q, ab, fg = (dc.T(h[k]).to(dtype) for k in ('q', 'abstract', 'fglob'))
        with torch.no_grad(), op.stable_ties():
            want = op.decoder_forward(sd, case.ia, q, ab, fg)
            got = dc.decoder_reference(sd, case.ia, dc.formula_map(case.ia), q, ab, fg)
        assert want[0].dtype == dtype and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), case.name
    # the shared reference is these runs
    r = dc.reference(case)
    assert np.array_equal(r['output64'], want[0].numpy()) and np.array_equal(r['penult64'], want[1].numpy())


def test_an_explicit_map_moves_the_layers():
    """The restatement follows its map: other positions give another result, and a map that names a layer twice runs it twice."""
    case = dc.BY_NAME['b6-at125']
    h = dc.inputs(case)
    args = [dc.T(h[k]) for k in ('q', 'abstract', 'fglob')]
    with torch.no_grad():
        a = dc.decoder_reference(h['sd'], case.ia, {1: 0, 2: 1, 5: 2}, *args)[0]
        b = dc.decoder_reference(h['sd'], case.ia, dc.formula_map(case.ia), *args)[0]
        c = dc.decoder_reference(h['sd'], case.ia, {1: 0, 2: 1}, *args)[0]
    assert dc.formula_map(case.ia) == {1: 0, 3: 1, 4: 2}
    assert float((a - b).abs().max()) > 1e-3 and float((a - c).abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------------------------- the tables
def test_case_tables_hold_every_layout_of_the_matrix():
    by = dc.BY_NAME
    layouts = {(c.ia['n_blocks'], c.ia['cross_attn_layers'], c.ia['local_mode']) for c in dc.LAYOUT_CASES if c.use_at is None}
    assert layouts >= {(6, 2, 'attention'), (5, 1, 'attention'), (1, 1, 'attention'), (2, 2, 'attention'), (7, 3, 'attention'),
                       (16, 4, 'attention'), (1, 0, 'feature'), (16, 0, 'feature'), (2, 3, 'attention'), (3, 4, 'attention')}
    assert dc.formula_map(by['b6c2'].ia) == {2: 0, 4: 1} and dc.formula_map(by['b5c1'].ia) == {2: 0}
    assert dc.formula_map(by['b1c1'].ia) == {0: 0} and dc.formula_map(by['b2c2'].ia) == {0: 0, 1: 1}
    assert len(dc.formula_map(by['b16c4'].ia)) == 4 and len(dc.formula_map(by['b7c3'].ia)) == 3
    assert dc.formula_map(by['b2c3-collision'].ia) == {0: 0, 1: 2} and dc.shadowed_layers(by['b2c3-collision']) == [1]
    assert dc.formula_map(by['b3c4-collision'].ia) == {0: 0, 1: 2, 2: 3} and dc.shadowed_layers(by['b3c4-collision']) == [1]
    overrides = [c.use_at for c in dc.LAYOUT_CASES if c.use_at is not None]
    assert overrides == [{0: 0}, {5: 0}, {0: 0, 1: 1, 2: 2, 3: 3}, {1: 0, 2: 1, 5: 2}]
    assert all(c.ia['n_blocks'] == 6 and c.use_at != dc.formula_map(c.ia) for c in dc.LAYOUT_CASES if c.use_at is not None)
    widths = {(c.ia['d_hidden'], c.ia['d_latent'], c.ia['d_latent_local'], c.ia['local_mode']) for c in dc.LAYOUT_CASES}
    assert widths >= {(64, 64, 32, 'attention'), (36, 36, 20, 'attention'), (288, 288, 288, 'attention'), (64, 416, 288, 'feature')}
    assert {c.ia['pos_encoding_freqs'] for c in dc.LAYOUT_CASES} == {0, 8} and {c.ia['d_in'] for c in dc.LAYOUT_CASES} == {3, 4}
    assert 1 in {c.ia['d_out'] for c in dc.LAYOUT_CASES}
    ks = {(c.ia['num_local_features'], c.ia['cross_attn_neighbors']) for c in dc.LAYOUT_CASES}
    assert ks == {(8, 14), (1, 1), (16, 16)} and pk.ops.FUSED_ATTN_MAX_K < 16
    assert (5, 1, 'swish') in {(c.ia['n_blocks'], c.ia['cross_attn_layers'], c.ia['activation']) for c in dc.LAYOUT_CASES}
    regime = [c for c in dc.LAYOUT_CASES if c.attn_wscale is not None]
    assert [(c.ia['n_blocks'], c.ia['cross_attn_layers'], c.attn_wscale, c.fscale) for c in regime] == [(7, 3, 4.0, 4.0)]
    assert sorted(c.nq for c in dc.LAYOUT_CASES if c.nq != dc.NQ) == [1, 1] and dc.NQ == 2 * 64 + 2
    assert all(by[n].ia['d_hidden'] == pk.ops.TRUNK_WIDTH and by[n].nq == dc.NQ for n in dc.PRODUCT_LAYOUTS)
    assert [(by[n].ia['n_blocks'], len(dc.live_map(by[n]))) for n in dc.PRODUCT_LAYOUTS] == [(6, 2), (2, 2), (7, 3), (6, 4), (16, 0)]
    train = [(c.ia['n_blocks'], c.ia['cross_attn_layers'], c.ia['d_hidden'], c.nq) for c in dc.TRAIN_CASES]
    assert train == [(1, 1, 416, 96), (2, 2, 416, 96), (7, 3, 416, 96), (2, 3, 416, 96), (2, 1, 64, 96)]


def test_selection_product_is_every_legal_combination():
    assert len(dc.SELECTIONS) == 3 * 2 * (5 + 4 + 4) == 78 and len({dc.selection_id(s) for s in dc.SELECTIONS}) == 78
    for trunk, fi, tp, attn in dc.SELECTIONS:
        assert not (tp != 'f32' and attn in dc.SPLIT and attn != tp)
        sel = pk.kernels.Selection(**dc.selection_fields(trunk, fi, tp, attn))
        assert sel.fused_interp == fi and sel.trunk_precision == tp
    assert ('default', True, 'bf16x6', 'attn16p') in dc.SELECTIONS and ('default', True, 'f16x3', 'f16x3') in dc.SELECTIONS
    assert ('default', False, 'bf16x6', 'f16x3') not in dc.SELECTIONS
    by = dc.BY_NAME
    on = dc.selection_fields('default', False, 'f32', 'attn16p')
    assert dc.expected_launches(pk, by['b6-at0123'], on) == (6, 4) and dc.expected_launches(pk, by['b16c0-feature'], on) == (16, 0)
    assert dc.expected_launches(pk, by['b7c3'], dc.selection_fields('generic', False, 'f32', 'chain')) == (0, 0)
    assert dc.expected_launches(pk, by['b2c3-collision'], on) == (2, 2)          # per LIVE layer


# ---------------------------------------------------------------------------------------------------------------- ties, bound
def test_every_case_is_free_of_neighbour_ties():
    for case in dc.LAYOUT_CASES + dc.TRAIN_CASES:
        h = dc.inputs(case)                                             # (asserts)
        assert h['q'].shape == (case.nq, case.ia['d_in']) and h['abstract'].shape == (dc.M_ABSTRACT, 3 + case.ia['d_latent_local'])
        assert h['fglob'].shape == (case.ia['d_latent'] - case.ia['d_latent_local'],)


def test_the_tie_assertion_rejects_a_tie():
    case = dc.BY_NAME['b6c2']
    h = dc.inputs(case)
    xyz = h['abstract'][:, :3].copy()
    q = h['q'].copy()
    dc.assert_no_ties(q, xyz, case.ia)
    # one query, so that the moved point makes this tie and no other: the 9th neighbour at the 8th one's distance, elsewhere
    one = q[7:8]
    order = np.argsort(np.linalg.norm(one[0, :3] - xyz, axis=1))
    moved = xyz.copy()
    moved[order[8]] = one[0, :3] + (xyz[order[7]] - one[0, :3])[[1, 2, 0]]
    with pytest.raises(AssertionError, match='interpolation search'):
        dc.assert_no_ties(one, moved, case.ia)
    # ... and a tie of the attention search alone (k = 14)
    moved = xyz.copy()
    moved[order[14]] = one[0, :3] + (xyz[order[13]] - one[0, :3])[[1, 2, 0]]
    with pytest.raises(AssertionError, match='attention search'):
        dc.assert_no_ties(one, moved, case.ia)
    dc.assert_no_ties(one, moved, dict(case.ia, local_mode='feature', cross_attn_layers=0))
    assert dc.tie_gaps(one, xyz[:8], 8, False)[0] == np.inf            # no 9th point: nothing to tie with


def test_the_bound_is_the_regime_rule_and_rejects_a_lost_term(twin):
    case = dc.BY_NAME['b6c2']
    r = dc.reference(case)
    for key in ('output', 'penult'):
        assert r['bound'][key] == max(1e-4, 2 * r['ref_error'][key]) and r['ref_error'][key] < 1e-4
    # a network whose lin_z[1] bias is lost (what finding 3 does to whole terms) is far outside
    net = dc.build_net(twin, 'cpu', case)
    with torch.no_grad():
        net.lin_z[1].bias.zero_()
    with pytest.raises(AssertionError, match='off by'):
        dc.check_forward(twin, 'cpu', case, net=net)
    assert not r['output64'].flags.writeable


# ---------------------------------------------------------------------------------------------------------------- the twin
@pytest.mark.parametrize('case', dc.LAYOUT_CASES, ids=dc.case_id)
def test_decoder_layouts_on_the_twin(twin, case):
    dc.check_forward(twin, 'cpu', case, tag='twin')


@pytest.mark.parametrize('name', ['b2c3-collision', 'b3c4-collision'])
def test_colliding_positions_shadow_as_in_the_reference(twin, name):
    """Finding 1: path_weights follows use_pt_inds; n_cross counts the distinct positions, cross[j] is the surviving layer."""
    case = dc.BY_NAME[name]
    net = dc.build_net(twin, 'cpu', case)
    assert len(net.pt_blocks) == case.ia['cross_attn_layers'] and net.use_pt_inds == dc.formula_map(case.ia)
    w, _, _ = net.path_weights()
    live = sorted(dc.formula_map(case.ia).items())
    assert w.n_cross == len(live) == case.ia['cross_attn_layers'] - 1
    assert [w.cross_after[j] for j in range(w.n_cross)] == [b for b, _ in live]
    for j, (_, layer) in enumerate(live):
        assert w.cross[j].to_q == net.pt_blocks[layer].layer2.to_q.weight.data_ptr()
    # the shadowed layer's parameters are loaded, and the result does not depend on them
    before = dc.check_forward(twin, 'cpu', case, net=net, tag='twin')
    with torch.no_grad():
        for p in net.pt_blocks[1].parameters():
            p.mul_(3.0)
    assert dc.check_forward(twin, 'cpu', case, net=net, tag='twin, shadowed layer x 3') == before


def test_positions_set_after_construction_are_followed(twin):
    """use_pt_inds is read when the weights are handed to the library, and a later change is seen (it is part of the cache key)."""
    case = dc.BY_NAME['b6-at125']
    net = dc.build_net(twin, 'cpu', case)
    w, _, _ = net.path_weights()
    assert [w.cross_after[j] for j in range(w.n_cross)] == [1, 2, 5]
    dc.check_forward(twin, 'cpu', case, net=net, tag='twin')
    net.use_pt_inds = {1: 0, 3: 1, 4: 2}
    w, _, _ = net.path_weights()
    assert [w.cross_after[j] for j in range(w.n_cross)] == [1, 3, 4]
    with pytest.raises(AssertionError, match='off by'):
        dc.check_forward(twin, 'cpu', case, net=net, tag='twin, the formula positions')
    net.use_pt_inds = {2: 1, 1: 0, 5: 2, 9: 0}
    with pytest.raises(AssertionError):
        net.path_weights()                                              # block 9 of 6


def test_a_decoder_without_a_global_part_on_the_twin(twin):
    """Finding 2: d_latent == d_latent_local hands the library no features_global, as on the device."""
    case = dc.BY_NAME['w288-e288-noglobal']
    assert dc.reference(case)['fglob'].shape == (0,)
    dc.check_forward(twin, 'cpu', case, tag='twin')
