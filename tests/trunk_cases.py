"""Shared by tests/test_trunk_cases_host.py (no GPU) and tests/test_gpu_trunk_edges.py (on the device): the case matrix, the numpy
fp64 references, the derived bounds, the driver that runs one call through the `ops` wrappers with every row operand a framed
view, and the check_* functions of the fp32 trunk kernels -- csrc/trunk.hip (occ4d_resblock_f32, _addrows, _chain,
occ4d_rowlin_f32, _linz, _masked), csrc/trunk4.hip (occ4d_resblock4_f32, occ4d_rowlin4_f32, _masked, _masked_skip) and
occ4d_interp_dense_f32.  The check_* functions are plain numpy over a `got` array: the device tests only produce `got`, the host
test feeds the same checks mutants of the reference and a numpy float32 evaluation of every case (`HostOps`).

Frames.  Every row operand of a call is the view buffer[:n, 4:4 + width] of a buffer whose other floats hold the sentinel NaN of
tests/forward_cases.py; each operand has a row stride of its own, width + 8 + 4 p with p its place in the order x, y, res / skip,
mask, addrows, ztab, dense, y_tail (the addrows of a chain's second and third block take the next two places; tables that must
share a stride lie side by side in one buffer, `width` being their joint width).  Outputs start as sentinels and carry GUARD_ROWS
rows behind row n.  After the call, compared as int32: no float outside an output view was written, every float inside was, and
every input buffer (views, frames, vectors, packed weights) is bit-identical to its state before the call.  ops.resblock_chain
allocates its tail rows itself, so y_tail is the one operand that is never a view.

Bounds are derived, not tuned: U = 2^-24, K = 416, and the argument in the module docstring of tests/test_gpu_backward_edges.py (a
fp32 sum of L terms in ANY order is within (L - 1) U sum|term| of the exact sum to first order; a term that is itself the rounded
result of c fp32 operations adds c more; 2 is constant slack).  All against the fp64 value of the same fp32 operands.

rowlin, per output element, a = [relu](x):

    |got - ref| <= (K + c + 2) U (sum_k |a_k w_k| + |b| + |res| + T)       T = sum_j |zw_j t_j| + |zconst| with a term

c = 1 (the products) + 1 per epilogue term present (b, res) + kz + 1 with an interpolation term (its kz products and additions
and the one that adds it).  The dense rows of a second term take the interp_add bound of tests/forward_cases.py without x_old,
(kz + 3 + 2) U T.  Where mask <= 0 the result is exactly 0.0: bound 0.  skip is added to the masked value by one more rounding:
+ U (|value| + |skip|), and where mask <= 0 the result is exactly skip.

resblock, first order, relu being 1-Lipschitz (j over hidden units, i over outputs):

    A_j = sum_k relu(x)_k |w0_jk| + |b0_j|                      e_j = (K + 3) U A_j   (what the hidden pre-activation is off by)
    B_i = sum_j |w1_ij| relu(h_j) + |x_i| + |b1_i| [+ |add_i|] [+ T_i]
    |got_i - ref_i| <= sum_j |w1_ij| e_j + (K + 5 + t) U B_i

t = 0 without a term, 1 with addrows, kz + 1 with an interpolation term.

chain (consecutive blocks, then optionally the tail Linear): block b + 1 reads rows that are off by d (the bound of block b's
output); relu is 1-Lipschitz and the block is x + W1 relu(W0 relu(x) + b0) + b1, so its output inherits at most
d_i + sum_j |w1_ij| sum_k |w0_jk| d_k, to which its own bound at the reference rows is added; the tail inherits sum_k |w_ik| d_k.

interp_dense: the row term is forward_cases' interp_add bound (kz + 3 + 2) U (T + |x_old|), the dense rows the same without x_old.

These are worst-case bounds: K roundings all of one sign.  A correct kernel's error grows like sqrt(K) U, so it sits near 1e-2
of the rowlin bound and, through the product of two such layers, near 1e-3 of the resblock and chain bounds (the host test
prints the ratios of a numpy float32 evaluation).  The bounds therefore catch errors of the size of a term -- the mutants of
the host test -- in every regime, whatever the operand scale; errors of a few ulp are what the exact cases below, the dead
hidden layer and the bit-for-bit metamorphic checks are for.

Exact cases hold the device to `==`.  Integer operands in [-8, 8] (table rows multiples of 4, interpolation weights in {0, 1/4,
1/2, 1}), weights in {-1, 0, 1} (single layers and blocks) or four entries of +-1 per output row (chains): every partial sum of
every layer is an integer below 2^24 in any order, so every fp32 evaluation gives the fp64 result.  `reference` returns the
sum|term| of every layer so that the host test asserts that precondition instead of trusting this paragraph.  Dead hidden layer
(b0 = -2^20 on random data): relu(h) = 0 and y is f32(x + b1), plus addrows as one more fp32 addition."""
import collections
import functools

import numpy as np
import torch

import forward_cases as fc
from forward_cases import F32, GUARD_ROWS, SENTINEL, U, framed, sentinel, to_device  # noqa: F401

H = 416
K = H
FULL, HALF = 'full', 'half'
ROWS = {FULL: (1, 15, 16, 17, 127, 128, 129, 300), HALF: (1, 63, 64, 65, 130)}
WIDTHS = {FULL: (32, 96, 416, 832), HALF: (16, 112, 416)}
EDGE_ROWS = {FULL: (17, 129), HALF: (17, 65)}
REGIMES = ('init', 'small_x', 'big_x', 'big_w', 'mixed_rows', 'cancel', 'dead_rows')
SLOT = dict(x=0, y=1, res=2, skip=2, mask=3, addrows=4, ztab=5, dense=6, y_tail=7)
TABLE_ROWS = 37
PACKERS = {FULL: ('pack_trunk_rows', 'pack_trunk_cols'), HALF: ('pack_trunk4_rows', 'pack_trunk4_cols')}

# entry: resblock | rowlin | linz | chain | dense.  opts (a sorted tuple of words):
#   resblock  inplace, interp8, interp3, addrows
#   rowlin    relu, res, alias (res is out), interp, mask, skip
#   linz      term, term2, res, alias
#   chain     adds (addrows on every block), inplace; nb blocks, tail = 0 or the tail's width (trelu: relu on its operand)
#   any       zero (all biases, zconst and addrows zero: homogeneity)
# regime: one of REGIMES, or 'exact' (integer operands), 'dead' (b0 = -2^20)
Call = collections.namedtuple('Call', 'entry pack n n_out opts regime nb tail')


def call(entry, pack, n, n_out=H, opts=(), regime='init', nb=1, tail=0):
    opts = tuple(sorted(opts.split() if isinstance(opts, str) else opts))
    assert entry in ('resblock', 'rowlin', 'linz', 'chain', 'dense') and pack in (FULL, HALF)
    assert regime in REGIMES + ('exact', 'dead')
    return Call(entry, pack, n, n_out, opts, regime, nb, tail)


def call_id(c):
    return '%s-%s-n%d-w%d-%s-%s%s' % (c.entry, c.pack, c.n, c.n_out, '+'.join(c.opts) or 'plain', c.regime,
                                      '-nb%d-tail%d' % (c.nb, c.tail) if c.entry == 'chain' else '')


# ---------------------------------------------------------------------------------------------------------------- the case matrix
RESBLOCK_OPTS = {FULL: ('', 'inplace', 'interp8', 'interp3', 'addrows'), HALF: ('', 'inplace', 'interp8', 'interp3')}
ROWLIN_OPTS = {FULL: ('', 'relu', 'res', 'res alias', 'res interp', 'mask', 'mask res relu'),
               HALF: ('', 'relu', 'res', 'res alias', 'res interp', 'mask', 'mask res relu', 'mask skip')}
LINZ_OPTS = ('term', 'term2', 'term term2 res', 'term term2 res alias')
CHAIN_FORMS = [(nb, adds, tail, inplace) for nb in (1, 2, 3) for adds in ('', 'adds') for tail in (0, 32, 832) for inplace in ('', 'inplace')]


def entry_calls(entry, pack, n, regime='init'):
    """Every form of an entry point at n rows (and every output width it has)."""
    if entry == 'resblock':
        return [call(entry, pack, n, H, o, regime) for o in RESBLOCK_OPTS[pack]]
    if entry == 'rowlin':
        return [call(entry, pack, n, w, o, regime) for w in WIDTHS[pack] for o in ROWLIN_OPTS[pack] if 'interp' not in o or w == H]
    if entry == 'linz':
        return [call(entry, FULL, n, w, o, regime) for w in WIDTHS[FULL] for o in LINZ_OPTS]
    if entry == 'chain':
        return [call(entry, FULL, n, H, ' '.join((a, i, 'trelu' if (nb + t) % 3 == 0 else '')), regime, nb, t) for nb, a, t, i in CHAIN_FORMS]
    return [call('dense', FULL, n, w, '', regime) for w in (96, H)]


FRAME_CALLS = [(e, p, n) for e, p in (('resblock', FULL), ('resblock', HALF), ('rowlin', FULL), ('rowlin', HALF), ('linz', FULL),
                                      ('chain', FULL), ('dense', FULL)) for n in ROWS[p]]


def regime_calls(regime):
    """Section 'regimes': resblock on both packings and with addrows, rowlin on both packings with a residual, rowlin_linz with
    both terms.  `cancel` is defined through the residual rows (res = -f32(W a + b)); a residual block has none of its own, so
    there the term added last cancels: addrows = -f32(block(x)), and on both packings an interpolation term that is exactly
    -f32(block(x)) (a table of n rows, row i the only neighbour of query i with weight 1, zconst = 0)."""
    out = []
    for pack in (FULL, HALF):
        for n in EDGE_ROWS[pack]:
            out.append(call('resblock', pack, n, H, 'interp8' if regime == 'cancel' else '', regime))
            out.append(call('rowlin', pack, n, H, 'res relu' if n == 17 else 'res', regime))
            out.append(call('rowlin', pack, n, WIDTHS[pack][1], 'res', regime))
    for n in EDGE_ROWS[FULL]:
        out.append(call('resblock', FULL, n, H, 'addrows', regime))
        out.append(call('linz', FULL, n, H, 'term term2 res', regime))
    return out


def exact_calls():
    out = []
    for e, p in (('resblock', FULL), ('resblock', HALF), ('rowlin', FULL), ('rowlin', HALF), ('linz', FULL), ('chain', FULL), ('dense', FULL)):
        for n in EDGE_ROWS[p]:
            out += entry_calls(e, p, n, 'exact')
    return out


def dead_calls():
    out = []
    for pack in (FULL, HALF):
        for n in EDGE_ROWS[pack]:
            out += [call('resblock', pack, n, H, o, 'dead') for o in ('', 'inplace') + (('addrows',) if pack == FULL else ())]
    for n in EDGE_ROWS[FULL]:
        out += [call('chain', FULL, n, H, 'adds', 'dead', 3, 0), call('chain', FULL, n, H, '', 'dead', 2, 0)]
    return out


# ---------------------------------------------------------------------------------------------------------------- operands
def _rng(*key):
    return fc._rng('trunk', *key)


@functools.lru_cache(maxsize=None)
def weight(kind, role, n_out):
    """(w (n_out, 416), b (n_out)) float32 of a layer: kind init (the scale of tests/test_gpu_trunk.py), big_w (the same values
    times 2^6), exact (entries of {-1, 0, 1}, integer bias), sparse (four entries of +-1 per output row, integer bias)."""
    rng = _rng('weight', role, n_out)
    w = (0.05 * rng.normal(size=(n_out, H))).astype(F32)
    b = (0.1 * rng.normal(size=n_out)).astype(F32)
    if kind == 'big_w':
        w = np.ldexp(w, 6).astype(F32)
    elif kind == 'exact':
        w = rng.integers(-1, 2, size=(n_out, H)).astype(F32)
        b = rng.integers(-8, 9, size=n_out).astype(F32)
    elif kind == 'sparse':
        w = np.zeros((n_out, H), F32)
        for i in range(n_out):
            w[i, rng.choice(H, size=4, replace=False)] = rng.choice([-1.0, 1.0], size=4)
        b = rng.integers(-8, 9, size=n_out).astype(F32)
    else:
        assert kind == 'init', kind
    return w, b                                              # (shared: callers copy before they change one)


def _row_scale(c):
    """The power of two each row of x and res is multiplied by."""
    if c.regime == 'small_x':
        return np.full(c.n, -12)
    if c.regime == 'big_x':
        return np.full(c.n, 12)
    if c.regime == 'mixed_rows':
        e = _rng('mixed', c.n).integers(-12, 13, size=c.n)
        e[:2] = (-12, 12)[:c.n]                              # neighbours of one 16-row tile, 2^24 apart
        return e
    return np.zeros(c.n, np.int64)


def _rows_of(c, name, width, e=None):
    rng = _rng(name, c.n, width)
    if c.regime == 'exact':
        return rng.integers(-8, 9, size=(c.n, width)).astype(F32)
    a = rng.normal(size=(c.n, width)).astype(F32)
    return a if e is None else np.ldexp(a, e[:, None]).astype(F32)


def _lists(c, kz):
    """Neighbour lists that repeat an index, weights with zeros and negative entries, an all-zero weight row."""
    rng = _rng('lists', c.n, kz)
    idx = rng.integers(0, TABLE_ROWS, size=(c.n, kz)).astype(np.int32)
    idx[:, 1] = idx[:, 0]
    if c.regime == 'exact':
        return idx, rng.choice([0.0, 0.25, 0.5, 1.0], size=(c.n, kz)).astype(F32)
    w = rng.uniform(-0.5, 1.0, size=(c.n, kz))
    w[:, 2] = 0.0
    w[0, :] = 0.0
    w /= np.abs(w).sum(1, keepdims=True).clip(1e-12)
    return idx, w.astype(F32)


def _tables(c, count, width):
    """`count` tables of TABLE_ROWS rows and their constants."""
    rng = _rng('tables', count, width, c.regime == 'exact')
    if c.regime == 'exact':
        tabs = (4 * rng.integers(-2, 3, size=(count, TABLE_ROWS, width))).astype(F32)
        zc = rng.integers(-8, 9, size=(count, width)).astype(F32)
    else:
        tabs = rng.normal(size=(count, TABLE_ROWS, width)).astype(F32)
        zc = rng.normal(size=(count, width)).astype(F32)
    if 'zero' in c.opts:
        zc = np.zeros_like(zc)
    return tabs, zc


def inputs(c):
    """Host arrays of a call.  Keys: x; layers = [(w, b, key)] in launch order (a block's two layers, then the tail); res, mask,
    skip, adds = [addrows per block or None]; tabs (count, table rows, width), zc (count, width), idx, zw."""
    kind = {'big_w': 'big_w', 'exact': 'sparse' if c.entry == 'chain' else 'exact'}.get(c.regime, 'init')
    e = _row_scale(c)
    h = dict(x=_rows_of(c, 'x', H, e), layers=[], adds=[])
    if c.regime == 'dead_rows':
        h['x'][::3] = -np.abs(h['x'][::3])
        h['x'][0, :8] = 0.0

    def layer(role, n_out, dead=False):
        w, b = weight(kind, role, n_out)
        if 'zero' in c.opts:
            b = np.zeros_like(b)
        if dead:
            b = np.full_like(b, -2.0 ** 20)
        h['layers'].append((w, b, (kind, role, n_out)))

    if c.entry in ('resblock', 'chain'):
        for i in range(c.nb):
            layer('w0_%d' % i, H, dead=c.regime == 'dead')
            layer('w1_%d' % i, H)
            add = None
            if 'addrows' in c.opts or 'adds' in c.opts:
                add = _rows_of(c, 'add%d' % i, H)
                if 'zero' in c.opts:
                    add = np.zeros_like(add)
            h['adds'].append(add)
        if c.tail:
            layer('tail', c.tail)
    elif c.entry in ('rowlin', 'linz'):
        layer('lin', c.n_out)
    kz = 3 if 'interp3' in c.opts else 8
    n_tab = {'dense': 3, 'linz': 2}.get(c.entry, 1 if {'interp', 'interp8', 'interp3'} & set(c.opts) else 0)
    if n_tab:
        h['tabs'], h['zc'] = _tables(c, n_tab, c.n_out)
        h['idx'], h['zw'] = _lists(c, kz)
    if 'res' in c.opts:
        h['res'] = _rows_of(c, 'res', c.n_out, e)
    if 'mask' in c.opts:
        mask = _rng('mask', c.n, c.n_out).normal(size=(c.n, c.n_out)).astype(F32)
        mask[0, :5] = 0.0                                    # zero counts as "not positive"
        if c.n > 1:
            mask[c.n // 2] = 0.0                             # one whole row
        if c.n_out > 16:
            mask[:, 16:32] = 0.0                             # one whole 16-channel stage
        mask[_rng('cells', c.n).integers(0, c.n, size=7), _rng('cells', c.n_out).integers(0, c.n_out, size=7)] = 0.0
        h['mask'] = mask
    if 'skip' in c.opts:
        h['skip'] = _rows_of(c, 'skip', c.n_out, e)
    if c.regime == 'cancel':
        plain = c._replace(regime='init', opts=tuple(o for o in c.opts if o not in ('res', 'alias', 'addrows', 'term', 'term2', 'interp8')))
        hp = dict(h, adds=[None] * len(h['adds']))
        hp.pop('res', None)
        flat = (resblock_reference(hp, 0) if c.entry == 'resblock' else rowlin_reference(plain, hp, term=None))[0]
        if c.entry == 'resblock' and 'interp8' in c.opts:
            h['tabs'], h['zc'] = (-flat.astype(F32))[None], np.zeros((1, H), F32)
            h['idx'] = np.repeat(np.arange(c.n, dtype=np.int32)[:, None], 8, axis=1)
            h['zw'] = np.repeat(np.array([[1, 0, 0, 0, 0, 0, 0, 0]], F32), c.n, axis=0)
        elif c.entry == 'resblock':
            h['adds'] = [(-flat.astype(F32)).astype(F32)]
        else:
            h['res'] = (-flat.astype(F32)).astype(F32)
    return h


# ---------------------------------------------------------------------------------------------------------------- references
Ref = collections.namedtuple('Ref', 'ref bound')


def f64(a):
    return np.asarray(a, dtype=np.float64)


def term64(h, t):
    """-> (value, sum|term|, kz) of interpolation term t: zc + sum_j zw_j tab[idx_j]."""
    terms = f64(h['zw'])[:, :, None] * f64(h['tabs'][t])[h['idx']]
    return terms.sum(1) + f64(h['zc'][t]), np.abs(terms).sum(1) + np.abs(f64(h['zc'][t])), h['idx'].shape[1]


def rowlin_reference(c, h, term, x=None, layer=-1, relu=None):
    """-> (fp64 result, bound, sum|term|) of [mask] ([res +] W [relu](x) + b [+ term]) [+ skip]."""
    w, b = f64(h['layers'][layer][0]), f64(h['layers'][layer][1])
    x = f64(h['x'] if x is None else x)
    a = np.maximum(x, 0.0) if ('relu' in c.opts if relu is None else relu) else x
    ref, mag, n_ops = a @ w.T + b, np.abs(a) @ np.abs(w).T + np.abs(b), 2
    if h.get('res') is not None:
        ref, mag, n_ops = ref + h['res'], mag + np.abs(f64(h['res'])), n_ops + 1
    if term is not None:
        v, m, kz = term
        ref, mag, n_ops = ref + v, mag + m, n_ops + kz + 1
    bound = (K + n_ops + 2) * U * mag
    if h.get('mask') is not None:
        dead = h['mask'] <= 0
        ref, bound = np.where(dead, 0.0, ref), np.where(dead, 0.0, bound)
        if h.get('skip') is not None:            # one more rounding, of value + skip: U (|value| + |skip|) covers it
            bound = np.where(dead, 0.0, bound + U * (np.abs(ref) + np.abs(f64(h['skip']))))
            ref = ref + h['skip']
    return ref, bound, mag


def resblock_reference(h, i, x=None, term=None):
    """-> (fp64 result, bound, [A, B]) of block i of h['layers'] on the rows x."""
    (w0, b0, _), (w1, b1, _) = h['layers'][2 * i], h['layers'][2 * i + 1]
    w0, b0, w1, b1 = f64(w0), f64(b0), f64(w1), f64(b1)
    x = f64(h['x'] if x is None else x)
    a = np.maximum(x, 0.0)
    A = a @ np.abs(w0).T + np.abs(b0)
    hr = np.maximum(a @ w0.T + b0, 0.0)
    ref, B, t = x + hr @ w1.T + b1, hr @ np.abs(w1).T + np.abs(x) + np.abs(b1), 0
    if h['adds'][i] is not None:
        ref, B, t = ref + h['adds'][i], B + np.abs(f64(h['adds'][i])), 1
    if term is not None:
        ref, B, t = ref + term[0], B + term[1], term[2] + 1
    bound = ((K + 3) * U * A) @ np.abs(w1).T + (K + 5 + t) * U * B
    return ref, bound, [A, B]


def reference(c, h):
    """-> ({output name: Ref(fp64 result, bound)}, [sum|term| of every layer]).  Outputs: y; dense (linz), dense1 / dense2
    (interp_dense); tail (chain)."""
    if c.entry == 'rowlin':
        ref, bound, mag = rowlin_reference(c, h, term64(h, 0) if 'interp' in c.opts else None)
        return dict(y=Ref(ref, bound)), [mag]
    if c.entry == 'linz':
        ref, bound, mag = rowlin_reference(c, h, term64(h, 0) if 'term' in c.opts else None)
        out, mags = dict(y=Ref(ref, bound)), [mag]
        if 'term2' in c.opts:
            v, m, kz = term64(h, 1)
            out['dense'] = Ref(v, (kz + 5) * U * m)
            mags.append(m)
        return out, mags
    if c.entry == 'resblock':
        ref, bound, mags = resblock_reference(h, 0, term=term64(h, 0) if 'tabs' in h else None)
        return dict(y=Ref(ref, bound)), mags
    if c.entry == 'dense':
        out, mags = {}, []
        for t, name in enumerate(('y', 'dense1', 'dense2')):
            v, m, kz = term64(h, t)
            if t == 0:
                v, m = v + h['x'], m + np.abs(f64(h['x']))
            out[name] = Ref(v, (kz + 5) * U * m)
            mags.append(m)
        return out, mags
    cur, delta, mags = f64(h['x']), 0.0, []
    for i in range(c.nb):
        w0, w1 = np.abs(f64(h['layers'][2 * i][0])), np.abs(f64(h['layers'][2 * i + 1][0]))
        ref, bound, m = resblock_reference(h, i, x=cur)
        delta = bound + (delta + (delta @ w0.T) @ w1.T if i else 0.0)
        cur, mags = ref, mags + m
    out = dict(y=Ref(cur, delta))
    if c.tail:
        ref, bound, m = rowlin_reference(c, dict(layers=h['layers']), None, x=cur, relu='trelu' in c.opts)
        out['tail'] = Ref(ref, bound + delta @ np.abs(f64(h['layers'][-1][0])).T)
        mags.append(m)
    return out, mags


def dead_expected(c, h):
    """The float32 result of a call with dead hidden layers: per block f32(x + b1), then + addrows as one more addition."""
    cur = h['x']
    for i in range(c.nb):
        cur = cur + h['layers'][2 * i + 1][1]
        if h['adds'][i] is not None:
            cur = cur + h['adds'][i]
        assert cur.dtype == F32
    return cur


# ---------------------------------------------------------------------------------------------------------------- the driver
_PACKED = {}


def packed(ops, device, pack, cols, key, w):
    """The packed stream of a weight: made once per (ops, device), read-only.  -> (tensor, its bits at pack time)."""
    k = (id(ops), str(device), pack, cols, key)
    if k not in _PACKED:
        wt = to_device(w, device)
        p = getattr(ops, PACKERS[pack][cols])(wt)
        assert np.array_equal(fc.host(wt).view(np.int32), w.view(np.int32)), 'the packer wrote its input'
        _PACKED[k] = (p, fc.host(p).view(np.int32).copy())
    return _PACKED[k]


class Frames:
    """The operands of one call and what they held before it."""

    def __init__(self, device):
        self.device, self.inputs, self.outputs = device, [], []

    def view(self, a, slot, name, shift=0):
        """An input row operand as a framed view."""
        buf, v = framed(a, 4, self.device, 0, pad=8 + 4 * (SLOT[slot] + shift))
        self.inputs.append((name, buf, fc.host(buf).view(np.int32).copy()))
        return v

    def flat(self, a, name):
        """A vector, an index list: contiguous."""
        t = to_device(a, self.device)
        self.inputs.append((name, t, np.ascontiguousarray(a).view(np.int32).copy()))
        return t

    def weights(self, ops, pack, cols, layer, name):
        p, bits = packed(ops, self.device, pack, cols, layer[2], layer[0])
        self.inputs.append((name, p, bits))
        return p

    def out(self, rows, cols, slot, name, init=None):
        """An output row operand: sentinels (or `init` inside the view), GUARD_ROWS rows behind it."""
        buf, v = framed(sentinel(rows, cols) if init is None else init, 4, self.device, GUARD_ROWS, pad=8 + 4 * SLOT[slot])
        self.outputs.append((name, buf, rows, cols))
        return v

    def record(self):
        """-> what check_frames takes: bits of every input before / after, bits of every output buffer."""
        return dict(inputs=[(name, before, fc.host(t).view(np.int32)) for name, t, before in self.inputs],
                    outputs=[(name, fc.host(buf).view(np.int32), rows, 4, cols) for name, buf, rows, cols in self.outputs])


def _got(t):
    return np.ascontiguousarray(fc.host(t))


def run_call(ops, device, c, h):
    """One call through the `ops` wrappers, every row operand a framed view -> ({output name: float32 array}, frame record)."""
    f = Frames(device)
    inplace = 'inplace' in c.opts
    x = f.out(c.n, H, 'x', 'x = y', init=h['x']) if inplace else f.view(h['x'], 'x', 'x')
    got = {}

    def table_views(count):
        """`count` tables side by side in one buffer (one row stride)."""
        both = np.concatenate(list(h['tabs']), axis=1)
        v = f.view(both, 'ztab', 'ztab')
        w = h['tabs'].shape[2]
        return [(f.flat(h['zc'][t], 'zconst%d' % t), v[:, t * w:(t + 1) * w]) for t in range(count)]

    def lists():
        return f.flat(h['idx'], 'idx'), f.flat(h['zw'], 'zw')

    if c.entry == 'resblock':
        l0, l1 = h['layers']
        y = x if inplace else f.out(c.n, H, 'y', 'y')
        interp = None
        if 'tabs' in h:
            (zc, tab), = table_views(1)
            interp = (zc, tab) + lists()
        add = f.view(h['adds'][0], 'addrows', 'addrows') if h['adds'][0] is not None else None
        ret = ops.resblock(x, f.weights(ops, c.pack, 0, l0, 'w0'), f.flat(l0[1], 'b0'), f.weights(ops, c.pack, 1, l1, 'w1'),
                           f.flat(l1[1], 'b1'), out=y, interp=interp, addrows=add)
        assert ret is y
        got['y'] = _got(y)
    elif c.entry == 'rowlin':
        (l0,) = h['layers']
        res = None
        if 'alias' in c.opts:
            y = res = f.out(c.n, c.n_out, 'y', 'y = res', init=h['res'])
        else:
            y = f.out(c.n, c.n_out, 'y', 'y')
            if 'res' in h:
                res = f.view(h['res'], 'res', 'res')
        interp = None
        if 'tabs' in h:
            (zc, tab), = table_views(1)
            interp = (zc, tab) + lists()
        mask = f.view(h['mask'], 'mask', 'mask') if 'mask' in h else None
        skip = f.view(h['skip'], 'skip', 'skip') if 'skip' in h else None
        ret = ops.rowlin(x, f.weights(ops, c.pack, 0, l0, 'w'), f.flat(l0[1], 'b'), c.n_out, relu_in='relu' in c.opts, residual=res,
                         out=y, interp=interp, mask=mask, skip=skip)
        assert ret is y
        got['y'] = _got(y)
    elif c.entry == 'linz':
        (l0,) = h['layers']
        res = None
        if 'alias' in c.opts:
            y = res = f.out(c.n, c.n_out, 'y', 'y = res', init=h['res'])
        else:
            y = f.out(c.n, c.n_out, 'y', 'y')
            if 'res' in h:
                res = f.view(h['res'], 'res', 'res')
        t1, t2 = table_views(2)
        idx, zw = lists()
        dense = f.out(c.n, c.n_out, 'dense', 'dense') if 'term2' in c.opts else None
        ret, d = ops.rowlin_linz(x, f.weights(ops, c.pack, 0, l0, 'w'), f.flat(l0[1], 'b'), c.n_out, idx, zw,
                                 term=t1 if 'term' in c.opts else None, term2=t2 if 'term2' in c.opts else None,
                                 relu_in='relu' in c.opts, residual=res, out=y, dense=dense)
        assert ret is y and d is dense
        got['y'] = _got(y)
        if dense is not None:
            got['dense'] = _got(dense)
    elif c.entry == 'chain':
        y = x if inplace else f.out(c.n, H, 'y', 'y')
        blocks = []
        for i in range(c.nb):
            l0, l1 = h['layers'][2 * i], h['layers'][2 * i + 1]
            add = f.view(h['adds'][i], 'addrows', 'addrows%d' % i, shift=i) if h['adds'][i] is not None else None
            blocks.append((f.weights(ops, FULL, 0, l0, 'w0_%d' % i), f.flat(l0[1], 'b0_%d' % i), f.weights(ops, FULL, 1, l1, 'w1_%d' % i),
                           f.flat(l1[1], 'b1_%d' % i), add))
        if c.tail:
            lt = h['layers'][-1]
            ret, tail = ops.resblock_chain(x, blocks, out=y, tail=(f.weights(ops, FULL, 0, lt, 'w_tail'), f.flat(lt[1], 'b_tail'),
                                                                 c.tail, int('trelu' in c.opts)))
            assert tail.shape == (c.n, c.tail)
            got['tail'] = _got(tail)
        else:
            ret = ops.resblock_chain(x, blocks, out=y)
        assert ret is y
        got['y'] = _got(y)
    else:
        y = f.out(c.n, c.n_out, 'x', 'x (in place)', init=h['x'][:, :c.n_out])
        terms = table_views(3)
        idx, zw = lists()
        d1, d2 = f.out(c.n, c.n_out, 'dense', 'dense1'), f.out(c.n, c.n_out, 'y_tail', 'dense2')
        ret = ops.interp_dense(y, terms, idx, zw, dense=(d1, d2))
        assert ret[0] is y and ret[1] is d1 and ret[2] is d2
        got.update(y=_got(y), dense1=_got(d1), dense2=_got(d2))
    return got, f.record()


def dense_inputs(c, h):
    """interp_dense adds to rows of its own width: the first n_out columns of x."""
    return dict(h, x=np.ascontiguousarray(h['x'][:, :c.n_out])) if c.entry == 'dense' else h


# ---------------------------------------------------------------------------------------------------------------- the checks
def check_frame(bits, rows, off, cols, what):
    """`bits`: an output buffer as int32.  Every float outside [0, rows) x [off, off + cols) still holds the sentinel, none inside."""
    hit = bits != SENTINEL
    inside = np.zeros_like(hit)
    inside[:rows, off:off + cols] = True
    assert not (hit & ~inside).any(), '%s: %d floats outside the view were written' % (what, int((hit & ~inside).sum()))
    assert (hit | ~inside).all(), '%s: %d floats of the view were not written' % (what, int((~hit & inside).sum()))


def check_frames(rec, what):
    for name, before, after in rec['inputs']:
        assert before.shape == after.shape and np.array_equal(before, after), '%s: the input %s was written' % (what, name)
    for name, bits, rows, off, cols in rec['outputs']:
        check_frame(bits, rows, off, cols, '%s: %s' % (what, name))


def check_values(c, h, got, refs=None):
    """Every element of every output within its bound of the fp64 reference -> the worst error / bound."""
    refs = reference(c, dense_inputs(c, h))[0] if refs is None else refs
    assert set(got) == set(refs), (call_id(c), sorted(got), sorted(refs))
    return max(fc.within(got[name], r.ref, r.bound, '%s: %s' % (call_id(c), name)) for name, r in refs.items())


def check_exact(c, h, got, refs=None):
    """Every element of every output equal to the fp64 reference."""
    refs = reference(c, dense_inputs(c, h))[0] if refs is None else refs
    assert set(got) == set(refs), (call_id(c), sorted(got), sorted(refs))
    for name, r in refs.items():
        g = got[name]
        assert g.dtype == F32 and g.shape == r.ref.shape, (call_id(c), name, g.dtype, g.shape)
        bad = ~(g.astype(np.float64) == r.ref)
        assert not bad.any(), '%s: %s: %d elements differ from the exact result, first at %s' % (
            call_id(c), name, int(bad.sum()), tuple(np.argwhere(bad)[0]))


def check_dead(c, h, got):
    want = dead_expected(c, h)
    assert got['y'].dtype == F32 and np.array_equal(got['y'], want), '%s: not f32(x + b1) [+ addrows]' % call_id(c)


def check_masked(c, h, got):
    """Where mask <= 0: exactly 0.0, or exactly skip."""
    dead = h['mask'] <= 0
    want = h['skip'][dead] if 'skip' in h else np.zeros(int(dead.sum()), F32)
    assert dead.any() and not dead.all() and np.array_equal(got['y'][dead], want), '%s: a masked cell is not exactly %s' % (
        call_id(c), 'skip' if 'skip' in h else '0.0')
    assert (c.n == 1 or dead[c.n // 2].all()) and (c.n_out == 16 or dead[:, 16:32].all())


def run_and_check(ops, device, c, how='values'):
    """Inputs, the call, the frame check and the value check of `how` -> the worst error / bound (0.0 for the exact kinds)."""
    h = inputs(c)
    got, rec = run_call(ops, device, c, dense_inputs(c, h))
    check_frames(rec, call_id(c))
    if 'mask' in h:
        check_masked(c, h, got)
    if how == 'exact':
        return check_exact(c, h, got) or 0.0
    if how == 'dead':
        return check_dead(c, h, got) or 0.0
    return check_values(c, h, got)


# ---------------------------------------------------------------------------------------------------------------- metamorphic
METAMORPHIC = [call('resblock', FULL, 300), call('resblock', HALF, 300), call('rowlin', FULL, 300, 832, 'res'),
               call('rowlin', HALF, 300, 416, 'res relu'), call('linz', FULL, 300, 416, 'term term2 res'),
               call('chain', FULL, 300, H, 'adds', nb=3, tail=832)]
HOMOGENEOUS = [call('rowlin', FULL, 300, 416, 'res zero'), call('rowlin', FULL, 300, 96, 'relu res zero'),
               call('rowlin', HALF, 300, 416, 'res zero'), call('rowlin', HALF, 300, 112, 'relu res zero'),
               call('resblock', FULL, 300, H, 'zero'), call('resblock', HALF, 300, H, 'zero'),
               call('chain', FULL, 300, H, 'zero', nb=3, tail=832), call('chain', FULL, 300, H, 'adds zero', nb=2)]
ROW_KEYS = ('x', 'res', 'mask', 'skip', 'idx', 'zw')


def permuted(h, order):
    """The same rows in another order."""
    out = dict(h, adds=[None if a is None else np.ascontiguousarray(a[order]) for a in h['adds']])
    for k in ROW_KEYS:
        if k in h:
            out[k] = np.ascontiguousarray(h[k][order])
    return out


def row_position(ops, device, c, same):
    """A batch and the same rows reversed: after un-reversing `same(a, b, what)` must hold for every output."""
    h = inputs(c)
    order = np.arange(c.n)[::-1]
    got = run_call(ops, device, c, h)[0]
    back = run_call(ops, device, c, permuted(h, order))[0]
    for name in got:
        same(got[name], back[name][order], '%s: %s of a row depends on its position' % (call_id(c), name))


def homogeneity(ops, device, c, same):
    """No bias, zconst or addrows: row i of x and res times 2^e_i gives row i of every output times 2^e_i."""
    h = inputs(c)
    assert all(not l[1].any() for l in h['layers']) and all(a is None or not a.any() for a in h['adds'])
    e = _rng('homogeneity', c.n).integers(-12, 13, size=c.n)
    scaled = dict(h, x=np.ldexp(h['x'], e[:, None]).astype(F32))
    if 'res' in h:
        scaled['res'] = np.ldexp(h['res'], e[:, None]).astype(F32)
    got = run_call(ops, device, c, h)[0]
    big = run_call(ops, device, c, scaled)[0]
    for name in got:
        assert np.isfinite(got[name]).all() and got[name].any()
        same(np.ldexp(got[name], e[:, None]).astype(F32), big[name], '%s: %s is not homogeneous in its rows' % (call_id(c), name))


def bits_equal(a, b, what):
    assert a.dtype == F32 and b.dtype == F32 and np.array_equal(a, b), what


# ---------------------------------------------------------------------------------------------------------------- half-CU tail split
def tail_split_rows(cus):
    return 2 * cus * 64 + 3 * 64 + 5


def tail_split(ops, device, cus, opts, same):
    """occ4d_rowlin4_* with 197 rows behind one full dispatch round (their four row tiles are each split over four workgroups by
    output stage range): the last 64 rows and 4000 random rows within the rowlin bound of fp64, and the 197 rows equal to the
    same rows run as a batch of their own (no full round, so no split) -> the worst error / bound."""
    n = tail_split_rows(cus)
    c = call('rowlin', HALF, n, H, opts)
    h = inputs(c)
    got = run_call(ops, device, c, h)[0]['y']
    rows = _rng('split rows', n).integers(0, n, size=4064)
    rows[:64] = np.arange(n - 64, n)
    part = lambda hh, r: dict(hh, **{k: np.ascontiguousarray(hh[k][r]) for k in ROW_KEYS if k in hh})   # noqa: E731
    ref, bound, _ = rowlin_reference(c, part(h, rows), term64(part(h, rows), 0) if 'interp' in c.opts else None)
    ratio = fc.within(np.ascontiguousarray(got[rows]), ref, bound, call_id(c))
    tail = np.arange(n - 197, n)
    alone = run_call(ops, device, c._replace(n=197), part(h, tail))[0]['y']
    same(np.ascontiguousarray(got[tail]), alone, '%s: a split row tile differs from the same rows run alone' % call_id(c))
    return ratio


# ---------------------------------------------------------------------------------------------------------------- numpy float32 ops
class HostOps:
    """The wrappers of ops.py that the driver calls, evaluated in numpy float32 on CPU tensors (numpy's blocked matrix product:
    another summation order than the kernels').  The host test runs the whole case matrix through it: the references, the
    bounds and the driver are checked before any device is involved.  A "packed" weight is a copy of the weight."""

    def pack_trunk_rows(self, w):
        return w.clone()

    pack_trunk_cols = pack_trunk4_rows = pack_trunk4_cols = pack_trunk_rows

    @staticmethod
    def _np(t):
        return None if t is None else t.detach().numpy().copy()

    @staticmethod
    def _store(y, out):
        assert y.dtype == F32
        if out is None:
            return torch.from_numpy(np.ascontiguousarray(y))
        out.copy_(torch.from_numpy(np.ascontiguousarray(y)))
        return out

    def _term(self, zc, tab, idx, zw):
        zc, tab, idx, zw = self._np(zc), self._np(tab), self._np(idx), self._np(zw)
        s = np.zeros((idx.shape[0], tab.shape[1]), F32)
        for j in range(idx.shape[1]):
            s = s + zw[:, j:j + 1] * tab[idx[:, j]]
        return s + zc

    def _block(self, x, w0, b0, w1, b1, add):
        hh = np.maximum(np.maximum(x, F32(0)) @ w0.T + b0, F32(0))
        y = (x + b1) + hh @ w1.T
        return y if add is None else y + add

    def resblock(self, x, w0p, b0, w1p, b1, out=None, interp=None, addrows=None):
        y = self._block(self._np(x), self._np(w0p), self._np(b0), self._np(w1p), self._np(b1), self._np(addrows))
        if interp is not None:
            y = y + self._term(*interp)
        return self._store(y, out)

    def rowlin(self, x, wp, b, n_out, relu_in=False, residual=None, out=None, interp=None, mask=None, skip=None):
        a = self._np(x)
        y = (np.maximum(a, F32(0)) if relu_in else a) @ self._np(wp).T + self._np(b)
        if residual is not None:
            y = y + self._np(residual)
        if interp is not None:
            y = y + self._term(*interp)
        if mask is not None:
            y = np.where(self._np(mask) > 0, y, F32(0))
        if skip is not None:
            y = y + self._np(skip)
        return self._store(y, out)

    def rowlin_linz(self, x, wp, b, n_out, idx, w, term=None, term2=None, relu_in=False, residual=None, out=None, dense=None):
        d = None if term2 is None else self._store(self._term(term2[0], term2[1], idx, w), dense)
        y = self.rowlin(x, wp, b, n_out, relu_in, residual, out, None if term is None else (term[0], term[1], idx, w))
        return y, d

    def resblock_chain(self, x, blocks, out=None, tail=None):
        cur = self._np(x)
        for w0p, b0, w1p, b1, add in blocks:
            cur = self._block(cur, self._np(w0p), self._np(b0), self._np(w1p), self._np(b1), self._np(add))
        t = None
        if tail is not None:
            wt, bt, n_out, relu_in = tail
            t = torch.from_numpy((np.maximum(cur, F32(0)) if relu_in else cur) @ self._np(wt).T + self._np(bt))
        y = self._store(cur, out)
        return y if tail is None else (y, t)

    def interp_dense(self, x, terms, idx, w, dense=None):
        s = [self._term(zc, tab, idx, w) for zc, tab in terms]
        d1, d2 = self._store(s[1], dense[0]), self._store(s[2], dense[1])
        return self._store(self._np(x) + s[0], x), d1, d2
