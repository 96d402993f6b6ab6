"""Shared by tests/test_decoder_layouts_host.py (through the g++ twin) and tests/test_gpu_decoder_layouts.py (on the device):
the decoder over the layouts and kernel selections its contract admits (check_decoder in csrc/path.hip: n_blocks 1..16,
0..4 cross-attention layers behind any ascending blocks, any d_hidden % 4 == 0, d_latent >= d_latent_local, n_freq >= 0,
k 1..16), where every other decoder test builds configs.model_args(kind).  The case tables, the input builders, the fp64
references, the bound and the check_* functions; no GPU in here: every check_* takes the package and a torch device.

Inputs: an abstract cloud of 40 points uniform in the GREATER input cuboid with 0.5 N(0, 1) features, a 0.3 N(0, 1) global
embedding, weights configs.fill_state_dict(configs.decoder_param_shapes(ia), seed + 1000), 130 queries (two 64-row tiles and
two rows) or 1.  `assert_no_ties` holds every case to: the k-th and (k + 1)-th neighbour distances of every query differ by
more than 1e-4 relative in fp64, for the interpolation search (Euclidean norm) and the attention search (squared sum) --
a case's `seed` is the first one from its round base that passes (three in four do).

Reference: oracle/path.py in fp64 on the CPU.  `decoder_reference` is op.decoder_forward's loop with an explicit
{block: layer} map in place of the constructor's formula (for the positions the formula cannot produce); the host file
asserts that with the formula's map it equals op.decoder_forward bit for bit in fp32 and fp64.

Bound: golden_cases.regime_bound per case and per tensor (output, penult), max(1e-4, 2 max|ref32 - ref64|) against the fp64
run, ref32 = the same oracle in fp32.  Every kernel selection is held to it, the split-precision ones included."""
import collections
import itertools

import numpy as np
import torch
import torch.nn.functional as F

import golden_cases as gc
import occlusions4d_amd as pk
from grad_checks import KINK_TAU, REL, grad_excess, grad_score, leaf_sd, rel_err, strict_with_kinks
from oracle import path as op

cfg = pk.configs
M_ABSTRACT = 40
NQ = 130
NQ_TRAIN = 96
TIE_GAP = 1e-4
T = gc.as_tensor

# use_at: None = the constructor's positions; a {block: layer} map = net.use_pt_inds is overridden with it after construction
Case = collections.namedtuple('Case', 'name family ia use_at nq seed attn_wscale fscale')


def _ia(n_blocks=6, layers=2, **kw):
    ia = dict(cfg.model_args('greater')[1])
    ia.update(n_blocks=n_blocks, cross_attn_layers=layers, cr_attn_type='c' * layers)
    ia.update(kw)
    return ia


def _feature(n_blocks, **kw):
    return _ia(n_blocks, 0, local_mode='feature', **kw)


def _width(d, e, **kw):
    return dict(d_hidden=d, d_latent=d, d_latent_local=e, **kw)


def C(name, family, ia, seed, use_at=None, nq=NQ, attn_wscale=None, fscale=1.0):
    return Case(name, family, ia, use_at, nq, seed, attn_wscale, fscale)


LAYOUT_CASES = [
    # (n_blocks, cross_attn_layers) through the constructor's formula
    C('b6c2', 'formula', _ia(6, 2), 102),                            # the published layout: cross after blocks 2 and 4
    C('b5c1', 'formula', _ia(5, 1), 112),                            # the constructor's defaults
    C('b1c1', 'formula', _ia(1, 1), 120),                            # cross after the only block
    C('b2c2', 'formula', _ia(2, 2), 133),                            # after blocks 0 and 1: consecutive, and after the last block
    C('b7c3', 'formula', _ia(7, 3), 140),
    C('b16c4', 'formula', _ia(16, 4), 151),                          # both maxima
    C('b1c0-feature', 'feature', _feature(1), 160),
    C('b16c0-feature', 'feature', _feature(16), 170),
    C('b6c2-q1', 'formula', _ia(6, 2), 180, nq=1),
    C('b16c0-feature-q1', 'feature', _feature(16), 190, nq=1),
    # collisions: the formula puts two layers behind one block, the later one shadows the earlier, whose parameters stay in the
    # state dict and are not run (b2c3: {0: 0, 1: 2}; b3c4: {0: 0, 1: 2, 2: 3})
    C('b2c3-collision', 'collision', _ia(2, 3), 200),
    C('b3c4-collision', 'collision', _ia(3, 4), 210),
    # positions the formula cannot produce, n_blocks = 6
    C('b6-at0', 'override', _ia(6, 1), 220, use_at={0: 0}),
    C('b6-at5', 'override', _ia(6, 1), 230, use_at={5: 0}),
    C('b6-at0123', 'override', _ia(6, 4), 240, use_at={0: 0, 1: 1, 2: 2, 3: 3}),
    C('b6-at125', 'override', _ia(6, 3), 250, use_at={1: 0, 2: 1, 5: 2}),
    # widths: the generic-Linear trunk, the attention fallbacks; 288 / 288 has no global part and takes the d = 288 attention kernel
    C('w64-e32', 'width', _ia(6, 2, **_width(64, 32)), 260),
    C('w36-e20', 'width', _ia(6, 2, **_width(36, 20)), 271),
    C('w288-e288-noglobal', 'width', _ia(6, 2, **_width(288, 288)), 280),
    C('w64-l416-feature', 'width', _feature(6, d_hidden=64), 290),
    # other options
    C('freq0', 'option', _ia(6, 2, pos_encoding_freqs=0), 300),
    C('din3', 'option', _ia(6, 2, d_in=3), 311),
    C('dout1', 'option', _ia(6, 2, d_out=1), 321),
    C('k1', 'option', _ia(6, 2, num_local_features=1, cross_attn_neighbors=1), 330),
    C('k16', 'option', _ia(6, 2, num_local_features=16, cross_attn_neighbors=16), 340),      # above FUSED_ATTN_MAX_K
    C('b5c1-swish', 'option', _ia(5, 1, activation='swish'), 350),
    # one scaled regime (golden_cases.DEC_REGIME_CASES) on a layout that is not the published one
    C('b7c3-w4', 'regime', _ia(7, 3), 361, attn_wscale=4.0, fscale=4.0),
]
TRAIN_CASES = [
    C('b1c1-train', 'train', _ia(1, 1), 400, nq=NQ_TRAIN),
    C('b2c2-train', 'train', _ia(2, 2), 412, nq=NQ_TRAIN),
    C('b7c3-train', 'train', _ia(7, 3), 421, nq=NQ_TRAIN),
    C('b2c3-collision-train', 'train', _ia(2, 3), 430, nq=NQ_TRAIN),
    C('w64-e32-b2c1-train', 'train', _ia(2, 1, **_width(64, 32)), 440, nq=NQ_TRAIN),
]
BY_NAME = {c.name: c for c in LAYOUT_CASES + TRAIN_CASES}
assert len(BY_NAME) == len(LAYOUT_CASES) + len(TRAIN_CASES)
PRODUCT_LAYOUTS = ['b6c2', 'b2c2', 'b7c3', 'b6-at0123', 'b16c0-feature']
ENTRY_LAYOUTS = ['b6c2', 'b16c0-feature', 'b2c2']


def case_id(c):
    return c.name


# ---------------------------------------------------------------------------------------------------------------- selections
SPLIT = ('bf16x6', 'f16x3')
TRUNKS = ('default', 'trunk4', 'generic')
ATTENTIONS = ('attn16p', 'first', 'chain') + SPLIT       # a split scheme: the attention GEMMs on it (fused, paired kernel's stream)


def selection_fields(trunk, fused_interp, trunk_precision, attention):
    """The kernels.Selection fields of one element of the product (tests/test_gpu_regimes.py: attention_path, decoder_variant)."""
    return dict(trunk4=trunk == 'trunk4', trunk_kernels=trunk != 'generic', fused_interp=fused_interp,
                trunk_precision=trunk_precision, attn16=attention in ('attn16p',) + SPLIT, fused_attention=attention != 'chain',
                logit_precision=attention if attention in SPLIT else 'f32')


def _legal(sel):
    try:
        pk.kernels.Selection(**selection_fields(*sel))     # one split scheme per module
        return True
    except AssertionError:
        return False


SELECTIONS = [s for s in itertools.product(TRUNKS, (False, True), ('f32',) + SPLIT, ATTENTIONS) if _legal(s)]


def selection_id(s):
    return '%s-%s-%s-%s' % (s[0], 'fusedinterp' if s[1] else 'interp', s[2], s[3])


# ---------------------------------------------------------------------------------------------------------------- inputs
def formula_map(ia):
    """{block: layer} as the reference's constructor builds it (model/implicit.py:264-268): a later layer with the position
    of an earlier one takes its place."""
    n, L = ia['n_blocks'], ia['cross_attn_layers']
    return {int((i + 1) * n / (L + 1)): i for i in range(L)}


def live_map(case):
    return dict(case.use_at) if case.use_at is not None else formula_map(case.ia)


def shadowed_layers(case):
    return sorted(set(range(case.ia['cross_attn_layers'])) - set(live_map(case).values()))


def tie_gaps(q, xyz, k, squared):
    """The relative gap between the k-th and the (k + 1)-th neighbour distance of every query, in fp64 (inf where the cloud
    has no (k + 1)-th point)."""
    d = ((np.asarray(q, np.float64)[:, None, :3] - np.asarray(xyz, np.float64)[None, :, :3]) ** 2).sum(-1)
    d = np.sort(d if squared else np.sqrt(d), axis=1)
    if d.shape[1] <= k:
        return np.full(d.shape[0], np.inf)
    return (d[:, k] - d[:, k - 1]) / d[:, k]


def assert_no_ties(q, xyz, ia, what=''):
    searches = [('interpolation', ia['num_local_features'], False)]
    if ia['cross_attn_layers'] > 0 and ia['local_mode'] == 'attention':
        searches.append(('attention', ia['cross_attn_neighbors'], True))
    for name, k, squared in searches:
        gap = tie_gaps(q, xyz, k, squared)
        assert (gap > TIE_GAP).all(), ('%s: the %s search (k = %d) of query %d has its k-th and (k + 1)-th neighbours within %.3g '
                                       'relative: take another seed' % (what, name, k, int(np.argmin(gap)), float(gap.min())))


def inputs(case):
    """-> dict(q (nq, d_in), abstract (40, 3 + E), fglob (d_latent - E,), sd): float32, seeded by the case alone."""
    ia = case.ia
    rng = np.random.default_rng(case.seed)
    (x0, x1), (y0, y1), (z0, z1) = cfg.input_cuboid('greater')
    lo, hi = np.array([x0, y0, z0]), np.array([x1, y1, z1])
    xyz = rng.uniform(lo, hi, size=(M_ABSTRACT, 3)).astype(np.float32)
    feats = (0.5 * rng.normal(size=(M_ABSTRACT, ia['d_latent_local']))).astype(np.float32)
    fglob = (0.3 * rng.normal(size=(ia['d_latent'] - ia['d_latent_local'],))).astype(np.float32)
    q = np.concatenate([rng.uniform(lo, hi, size=(case.nq, 3)), rng.integers(0, 12, size=(case.nq, 1))], axis=1).astype(np.float32)
    q = np.ascontiguousarray(q[:, :ia['d_in']])
    assert_no_ties(q, xyz, ia, case.name)
    sd = cfg.fill_state_dict(cfg.decoder_param_shapes(ia), case.seed + 1000)
    if case.attn_wscale is not None:
        for name in list(sd):
            if '.layer2.' in name and sd[name].dim() == 2:
                sd[name] = sd[name] * np.float32(case.attn_wscale)
    fs = np.float32(case.fscale)
    return dict(q=q, abstract=np.concatenate([xyz, feats * fs], axis=1), fglob=fglob * fs, sd=sd)


# ---------------------------------------------------------------------------------------------------------------- reference
def decoder_reference(sd, ia, use_at, points_query, points_abstract, features_global):
    """op.decoder_forward (oracle/path.py: D1 - D7) with the explicit {block: layer} map `use_at`, out of the oracle's own
    helpers, statement by statement -> (output (N, G), penult (N, H)) in the dtype of the arguments."""
    features_abstract = points_abstract[..., 3:]
    points_abstract = points_abstract[..., :3]
    act = ia.get('activation', 'relu')
    abstract = torch.cat([points_abstract, features_abstract], dim=-1)
    inds, dists = op.knn_with_dists(points_query, abstract, ia['num_local_features'])
    w = 1.0 / (dists + 1e-4)
    w = F.normalize(w, p=1, dim=-1)
    f_local = torch.einsum('ik,ikf->if', w, features_abstract[inds])
    f_query = torch.cat([features_global[None, :].expand(points_query.shape[0], -1), f_local], dim=-1)
    assert f_query.shape[-1] == ia['d_latent']
    pe = op.positional_encode(points_query, 0.1, ia['pos_encoding_freqs']) if ia['pos_encoding_freqs'] > 0 else points_query
    x = op._lin(sd, 'lin_in', pe)
    p = pe[..., :3][None]
    for i in range(ia['n_blocks']):
        x = x + op._lin(sd, 'lin_z.%d' % i, f_query)
        h = op._lin(sd, 'blocks.%d.fc_0' % i, op._act(act, x))
        x = x + op._lin(sd, 'blocks.%d.fc_1' % i, op._act(act, h))
        if i in use_at:
            bsd = op._sub(sd, 'pt_blocks.%d.' % use_at[i])
            x = op.pt_block(bsd, x[None], p, features_abstract[None], points_abstract[None], ia['cross_attn_neighbors'], None)[0][0]
    return op._lin(sd, 'lin_out', op._act(act, x)), x


def reference_run(case, h, dtype):
    sd = {k: v.to(dtype) for k, v in h['sd'].items()}
    with torch.no_grad(), op.stable_ties():
        out, pen = decoder_reference(sd, case.ia, live_map(case), T(h['q']).to(dtype), T(h['abstract']).to(dtype), T(h['fglob']).to(dtype))
    return out.numpy(), pen.numpy()


_REFERENCES = {}


def reference(case):
    """The inputs of a case, its fp32 and fp64 oracle runs and the two bounds: computed once, shared, read-only."""
    hit = _REFERENCES.get(case.name)
    if hit is None:
        h = inputs(case)
        out32, pen32 = reference_run(case, h, torch.float32)
        out64, pen64 = reference_run(case, h, torch.float64)
        assert out64.dtype == np.float64 and out32.dtype == np.float32
        hit = dict(h, output=out32, penult=pen32, output64=out64, penult64=pen64)
        hit['bound'] = {key: gc.regime_bound(hit, key) for key in ('output', 'penult')}
        hit['ref_error'] = {key: float(np.abs(hit[key].astype(np.float64) - hit[key + '64']).max()) for key in ('output', 'penult')}
        for v in hit.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFERENCES[case.name] = hit
    return hit


# ---------------------------------------------------------------------------------------------------------------- checks
def dev(a, device):
    t = T(np.array(a))
    return t if torch.device(device).type == 'cpu' else t.to(device)


def build_net(pk, device, case, train=False):
    net = pk.implicit.LocalPclResnetFC(**case.ia)
    net.load_state_dict(reference(case)['sd'])
    if case.use_at is not None:
        assert set(case.use_at.values()) <= set(range(len(net.pt_blocks)))
        net.use_pt_inds = dict(case.use_at)
    else:
        assert getattr(net, 'use_pt_inds', {}) == formula_map(case.ia)
    if torch.device(device).type != 'cpu':
        net = net.to(device)
    return net.train() if train else net.eval()


_NETS = {}


def shared_net(pk, device, case):
    """One inference module per (device, case) for the selection product: its prepared weights are cached per flag value."""
    key = (str(device), pk._lib.is_twin(), case.name)
    if key not in _NETS:
        _NETS[key] = build_net(pk, device, case)
    return _NETS[key]


def max_err(got, ref):
    got = got.detach().cpu().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    return float(np.nan_to_num(err, nan=np.inf).max()) if err.size else 0.0


def check_forward(pk, device, case, selection=None, net=None, tag='default'):
    """One case through LocalPclResnetFC.forward under a kernel selection -> dict(output=, penult=) of max|got - ref64|, both
    asserted against the case's bounds after they are printed."""
    r = reference(case)
    net = build_net(pk, device, case) if net is None else net
    with torch.no_grad(), pk.kernels(**(selection or {})):
        out, pen = net(dev(r['q'], device), dev(r['abstract'], device), dev(r['fglob'], device), None)
    assert out.shape == r['output64'].shape and pen.shape == r['penult64'].shape and out.dtype == pen.dtype == torch.float32
    got = dict(output=max_err(out, r['output64']), penult=max_err(pen, r['penult64']))
    print('\n[layouts %s / %s] output: max|x| %.3g |got - ref64| %.3g |ref32 - ref64| %.3g bound %.3g   penult: max|x| %.3g '
          '|got - ref64| %.3g |ref32 - ref64| %.3g bound %.3g'
          % (case.name, tag, float(np.abs(r['output64']).max()), got['output'], r['ref_error']['output'], r['bound']['output'],
             float(np.abs(r['penult64']).max()), got['penult'], r['ref_error']['penult'], r['bound']['penult']))
    for key in ('output', 'penult'):
        assert got[key] <= r['bound'][key], '%s / %s: %s off by %.3g > %.3g' % (case.name, tag, key, got[key], r['bound'][key])
    return got


def expected_launches(pk, case, selection):
    """(fused residual blocks, fused attention kernels) the library's launch-event hook must report for one forward over a
    single row chunk: n_blocks whenever the trunk kernels serve the width, one per LIVE cross layer whenever attention is fused."""
    ia = case.ia
    trunk = selection['trunk_kernels'] and ia['d_hidden'] == pk.ops.TRUNK_WIDTH and ia['activation'] == 'relu'
    fused = (selection['fused_attention'] and ia['d_hidden'] in pk.ops.FUSED_ATTN_DIMS
             and ia['cross_attn_neighbors'] <= pk.ops.FUSED_ATTN_MAX_K)
    return (ia['n_blocks'] if trunk else 0), (len(live_map(case)) if fused else 0)


def check_selection(pk, device, case, sel):
    """One element of the selection product: the bound, and which kernels really ran (tests/test_gpu_parity.py:
    test_decoder_kernel_variants)."""
    fields = selection_fields(*sel)
    net = shared_net(pk, device, case)
    r = reference(case)
    args = (dev(r['q'], device), dev(r['abstract'], device), dev(r['fglob'], device), None)
    counts = {}
    try:
        for fam in ('resblock', 'cross_attn'):
            timer = pk.ops.KernelTimer(lambda name, fam=fam, **shape: name == fam)
            pk.ops.set_kernel_timer(timer)
            with torch.no_grad(), pk.kernels(**fields):
                net(*args)
            pk.ops.set_kernel_timer(None)
            counts[fam] = timer.summary().get(fam, dict(launches=0))['launches']
    finally:
        pk.ops.set_kernel_timer(None)
    got = check_forward(pk, device, case, fields, net=net, tag=selection_id(sel))
    assert (counts['resblock'], counts['cross_attn']) == expected_launches(pk, case, fields), (counts, case.name, selection_id(sel))
    return got


def check_entry_forms(pk, device, case):
    """The batched (1, N, 4) form, forward_output_only, and forward_output_only on the rows of query_prelude with and
    without lin_in's output x0: the same kernels on the same operands, so torch.equal (tests/test_gpu_query_prelude.py)."""
    r = reference(case)
    net = build_net(pk, device, case)
    q, ab, fg = dev(r['q'], device), dev(r['abstract'], device), dev(r['fglob'], device)
    n = q.shape[0]
    with torch.no_grad():
        out, pen = net(q, ab, fg, None)
        out_b, pen_b = net(q[None], ab[None], fg[None], None)
        assert out_b.shape == (1,) + tuple(out.shape) and torch.equal(out_b[0], out) and torch.equal(pen_b[0], pen)
        plain = net.forward_output_only(q, ab, fg, None, torch.full_like(out, float('nan')))
        assert torch.equal(plain, out), 'forward_output_only differs from forward'
        xyz = ab[:, :3].contiguous()
        saved = pk.implicit.PRELUDE_X0_MAX
        try:
            for with_x0 in (True, False):
                pk.implicit.PRELUDE_X0_MAX = saved if with_x0 else 0
                buf = net.query_prelude(q, xyz)
                assert (buf['x0'] is not None) == with_x0 and (buf['idx_cross'] is not None) == bool(live_map(case))
                got = net.forward_output_only(q, ab, fg, None, torch.full_like(out, float('nan')), prelude=(buf, 0, n))
                assert torch.equal(got, out), 'the prelude path (x0 %s) differs from the plain forward' % with_x0
        finally:
            pk.implicit.PRELUDE_X0_MAX = saved
    assert max_err(out, r['output64']) <= r['bound']['output']


class _LiveParameters:
    """named_parameters() of a module without the shadowed cross layers': what grad_excess / grad_score walk."""

    def __init__(self, net, shadowed):
        self.net, self.prefixes = net, tuple('pt_blocks.%d.' % j for j in shadowed)

    def named_parameters(self):
        return [(n, p) for n, p in self.net.named_parameters() if not n.startswith(self.prefixes)]


def check_training(pk, device, case):
    """_forward_train against the oracle's autograd, by the method of tests/test_gpu_training.py::test_decoder_gradients:
    outputs, every parameter gradient, the feature and global-embedding gradients; a shadowed layer's parameters come back
    with no gradient or an all-zero one, on both sides."""
    r = reference(case)
    ia, sd = case.ia, r['sd']
    q, abstract, fglob = T(np.array(r['q'])), T(np.array(r['abstract'])), T(np.array(r['fglob']))
    rng = np.random.default_rng(5)
    go = torch.from_numpy(rng.normal(size=(q.shape[0], ia['d_out'])).astype(np.float32))
    gp = torch.from_numpy(rng.normal(size=(q.shape[0], ia['d_hidden'])).astype(np.float32)) * 0.1
    net = build_net(pk, device, case, train=True)
    ab = abstract.to(device).requires_grad_(True)
    fg = fglob.to(device).requires_grad_(True)
    out, pen = net(q.to(device), ab, fg, None)
    ((out * go.to(device)).sum() + (pen * gp.to(device)).sum()).backward()
    shadowed = shadowed_layers(case)
    live = _LiveParameters(net, shadowed)
    dead = [(n, p) for n, p in net.named_parameters() if n.startswith(live.prefixes)] if shadowed else []
    assert len(dead) == 15 * len(shadowed)
    for name, p in dead:
        assert p.grad is None or not p.grad.any(), 'the shadowed ' + name + ' has a gradient'

    def oracle_run():
        rsd = leaf_sd(sd)
        ab_r = abstract.clone().requires_grad_(True)
        fg_r = fglob.clone().requires_grad_(True)
        with op.stable_ties():
            out_r, pen_r = op.decoder_forward(rsd, ia, q, ab_r, fg_r)
        ((out_r * go).sum() + (pen_r * gp).sum()).backward()
        for name, _ in dead:
            assert rsd[name].grad is None, name
        return rsd, ab_r, fg_r, out_r, pen_r

    def compare(ref):
        rsd, ab_r, fg_r, out_r, pen_r = ref
        assert rel_err(out, out_r) < 2e-5 and rel_err(pen, pen_r) < 2e-5
        return (max(grad_excess(live, rsd)[1], rel_err(ab.grad[:, 3:], ab_r.grad[:, 3:]) / REL, rel_err(fg.grad, fg_r.grad) / REL),
                grad_score(live, rsd))
    n_units, n_flipped = strict_with_kinks(oracle_run, compare)
    print('\n[layouts %s] decoder gradients: %d ReLU inputs within %.0e of zero, %d decided the other way in the product; %d shadowed '
          'parameters without gradient' % (case.name, n_units, KINK_TAU, n_flipped, len(dead)))
