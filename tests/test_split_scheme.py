"""The numpy model of the split-precision schemes (tests/split_scheme.py) against the claims of csrc/bf16x6.hpp, on the
CPU: every binade from 2^-30 to 2^16, fp16 tie points, signed zeros and the exact edges of the fp16 windows."""
import numpy as np
import pytest

import split_scheme as ss


def binade_sweep(lo=-30, hi=16, per=257, seed=0):
    """per binade: its edges, random significands, and the fp16 tie points of the leading and of the second piece."""
    rng = np.random.default_rng(seed)
    vals = [np.float32(0.0), np.float32(-0.0)]
    for e in range(lo, hi):
        base = 2.0 ** e
        sig = np.concatenate([[1.0, 2.0 - 2.0 ** -23], 1.0 + rng.random(per)])
        # x = 2^e (1 + (j + 1/2) 2^-10): exactly half-way between two fp16 values of that binade
        ties = 1.0 + (np.arange(0, 1024, 37) + 0.5) * 2.0 ** -10
        # half-way points of the second piece: the residual sits on an fp16 tie of ITS binade
        ties2 = 1.0 + 2.0 ** -10 * np.arange(1, 1024, 113) + 2.0 ** -21 * 1.5
        vals.append((base * np.concatenate([sig, ties, ties2])).astype(np.float32))
    v = np.concatenate([np.atleast_1d(a) for a in vals])
    return np.concatenate([v, -v])


def test_f16_cast_is_round_to_nearest_even_with_subnormals_and_inf():
    """the model's conversion = v_cvt_pk_f16_f32 in the default mode."""
    def f(v):
        with np.errstate(over='ignore'):
            return float(np.float32(v).astype(np.float16))
    assert f(1.0 + 2.0 ** -11) == 1.0                          # tie -> even
    assert f(1.0 + 3 * 2.0 ** -11) == 1.0 + 2.0 ** -9
    assert f(2.0 ** -24) == 2.0 ** -24                         # smallest subnormal kept
    assert f(2.0 ** -25) == 0.0 and f(3 * 2.0 ** -26) == 2.0 ** -24
    assert f(65504.0) == 65504.0 and f(65519.996) == 65504.0
    assert np.isinf(f(65520.0)) and np.isinf(f(-65520.0)) and f(-65520.0) < 0
    assert np.signbit(np.float32(-0.0).astype(np.float16))


@pytest.mark.parametrize('scale', [1.0, ss.F16_HSCALE, ss.F16_WSCALE, ss.F16_HSCALE * ss.F16_WSCALE])
def test_f16_representation_inside_the_stated_bound(scale):
    """|x - (x1 + x2) / s| <= 2^-23 |x| where |x s| >= 0.25, <= 2^-25 / s below: in every binade whose leading piece is
    finite, ties and zeros included; the two pieces reproduce the zeros' sign-insensitive value exactly."""
    x = binade_sweep()
    x = x[np.abs(x.astype(np.float64)) * scale < ss.F16_MAX]
    err = np.abs(ss.represent(x, 'f16x3', scale) - x.astype(np.float64))
    bound = ss.rep_bound(x, 'f16x3', scale)
    ratio = err / np.where(bound > 0, bound, 1.0)
    assert np.isfinite(err).all()
    assert (err <= bound).all(), 'worst %.4g x the bound at x = %r' % (ratio.max(), x[np.argmax(ratio)])
    # the bound is tight: the sweep reaches at least half of it, in both regimes
    big = np.abs(x.astype(np.float64)) * scale >= ss.F16_THRESH
    assert ratio[big].max() > 0.5 and ratio[~big & (x != 0)].max() > 0.5
    assert (ss.represent(np.float32([0.0, -0.0]), 'f16x3', scale) == 0).all()


def test_bf16_pieces_are_exact():
    x = binade_sweep(-60, 60, per=65)
    h, m, l_ = ss.bf16_pieces(x)
    assert ((h + m + l_) == x.astype(np.float64)).all()
    for p in (h, m, l_):      # each piece is a bf16 value
        assert (p.astype(np.float32).view(np.uint32) & 0xffff == 0).all()


@pytest.mark.parametrize('scheme', ss.SCHEMES)
def test_products_inside_the_stated_bound(scheme):
    """every pair of the sweep (weights scaled into the scheme's window): |x w - kept products| <= product_bound --
    the representation errors through the other operand and the dropped partial products, nothing else."""
    x = binade_sweep(-30, 16, per=17, seed=1)
    w = binade_sweep(-20, 8, per=17, seed=2)
    if scheme == 'f16x3':
        x = x[np.abs(x) < ss.F16_MAX]
        w = w[np.abs(w) * ss.F16_WSCALE < ss.F16_MAX]
    else:
        x, w = x * np.float32(2.0 ** 20), w * np.float32(2.0 ** -30)      # bf16: anywhere products stay normal
    err = ss.product_error(x[:, None], w[None, :], scheme)
    bound = ss.product_bound(x[:, None], w[None, :], scheme)
    assert np.isfinite(err).all()
    worst = (err / np.where(bound > 0, bound, 1.0)).max()
    print('\n[%s] worst product error / bound %.3f' % (scheme, worst))
    assert (err <= bound).all(), worst


def test_bf16_dropped_products_worst_case():
    """x = 2^e (1 + 2^-7 - 2^-23) -- significand bits 8 .. 23 all ones -- makes the second piece ~2^-7 |x| and the third
    ~2^-15 |x|: a2 b3 + a3 b2 reaches 2^-21 |a b| (not the 2^-23 an earlier header comment stated), and never more."""
    worst = np.float32(1.0 + 2.0 ** -7 - 2.0 ** -23)
    rng = np.random.default_rng(3)
    cand = np.concatenate([[worst, np.float32(2.0 - 2.0 ** -23), np.float32(1.0 + 2.0 ** -8 + 2.0 ** -16 + 2.0 ** -23)],
                           (1.0 + rng.random(4000)).astype(np.float32)])
    err = ss.product_error(cand[:, None], cand[None, :], 'bf16x6')
    rel = err / np.abs(cand.astype(np.float64)[:, None] * cand.astype(np.float64)[None, :])
    assert rel.max() <= ss.BF16_DROP
    assert rel[0, 0] > 0.95 * ss.BF16_DROP


def test_f16_window_edges():
    """the largest activation with a finite leading piece is just below 65520, the largest packed weight just below
    65520 / 256 = 255.9375; one step further the leading piece is inf."""
    below = np.nextafter(np.float32(ss.F16_MAX), np.float32(0))
    p1, p2 = ss.f16_pieces(below)
    assert np.isfinite(p1) and np.isfinite(p2) and p1 == 65504.0
    p1, _ = ss.f16_pieces(np.float32(ss.F16_MAX))
    assert np.isinf(p1)
    wmax = ss.F16_MAX / ss.F16_WSCALE
    assert wmax == 255.9375
    p1, p2 = ss.f16_pieces(np.nextafter(np.float32(wmax), np.float32(0)), ss.F16_WSCALE)
    assert np.isfinite(p1) and np.isfinite(p2)
    assert np.isinf(ss.f16_pieces(np.float32(wmax), ss.F16_WSCALE)[0])
    assert np.isinf(ss.f16_pieces(np.float32(-wmax), ss.F16_WSCALE)[0])
    # a weight packed at 16 x 256 (the hidden scale on top of the weight scale) has a 16 times narrower window
    assert np.isinf(ss.f16_pieces(np.float32(16.0), ss.F16_HSCALE * ss.F16_WSCALE)[0])
    # out of the window, the two pieces are inf and -inf: their products cancel to NaN
    p1, p2 = ss.f16_pieces(np.float32(7e4))
    assert p1 == np.inf and p2 == -np.inf


@pytest.mark.parametrize('scheme', ss.SCHEMES)
def test_rowlin_model_contract(scheme):
    """the model of a whole row-kernel GEMM (K = 416, rows of very different scales) is inside contract_bound of the
    exact result with the accumulation allowance removed: the contract has room for the kernel's fp32 sums."""
    rng = np.random.default_rng(5)
    rows = 2.0 ** np.arange(-12, 13, 3)
    x = (rng.normal(size=(rows.size, 416)) * rows[:, None]).astype(np.float32)
    w = (rng.normal(size=(208, 416)) / np.sqrt(416)).astype(np.float32)
    w[0, :8] = [0.0, -0.0, 2.0 ** -20, -2.0 ** -12, 128.0, 255.0, 255.93, -200.0]
    model, exact, s, contract = ss.rowlin(x, w, scheme=scheme)
    assert np.isfinite(model).all()
    assert (np.abs(model - exact) <= contract - ss.ACC * s + 1e-300).all()
