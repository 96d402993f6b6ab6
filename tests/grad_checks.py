"""Shared by tests/test_gpu_training.py and tests/test_gpu_decoder_layouts.py: how gradients of the HIP training path are
compared with torch autograd over the CPU oracle (oracle/path.py) -- within 1e-4 relative to the largest entry of each
gradient tensor, with the handful of ReLU units whose input sits within rounding of zero enumerated instead of the
tolerance loosened (strict_with_kinks).  No GPU in here and no test."""
from oracle import path as op

REL = 1e-4


def rel_err(a, b):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / max(1e-12, float(b.abs().max())))


def grad_excess(module, ref_sd, tol=REL, floor=2e-6):
    """Worst (name, max|grad - ref| / (tol * max|ref| + floor)) over the parameters: <= 1 passes.  The absolute floor
    covers parameters whose true gradient is zero (attn_mlp.2.bias: a per-channel constant cancels in the softmax over
    the neighbours), where both sides are rounding noise."""
    worst = ('', 0.0)
    for name, p in module.named_parameters():
        assert p.grad is not None, 'no gradient for ' + name
        ref = ref_sd[name].grad
        assert ref is not None, 'oracle has no gradient for ' + name
        d = p.grad.detach().cpu().double() - ref.double()
        e = float(d.abs().max()) / (tol * float(ref.abs().max()) + floor)
        if e > worst[1]:
            worst = (name, e)
    return worst


def check_grads(module, ref_sd, tol=REL, floor=2e-6):
    """Per parameter: max|grad - ref| <= tol * max|ref| + floor (1e-4 relative)."""
    worst = grad_excess(module, ref_sd, tol, floor)
    assert worst[1] <= 1.0, 'worst gradient mismatch %s: %.3g x tolerance' % worst


KINK_TAU = 5e-6      # |ReLU input| below this: two fp32 implementations may decide differently (their rounding: ~1e-6)


def grad_score(module, ref_sd):
    """Smooth mismatch measure that guides the search below: sum over the parameters of |grad - ref|^2 / |ref|^2."""
    tot = 0.0
    for name, p in module.named_parameters():
        ref = ref_sd[name].grad.double()
        # (absolute floor: a parameter whose true gradient is zero -- attn_mlp.2.bias -- is rounding noise on both sides)
        tot += float((p.grad.detach().cpu().double() - ref).norm() ** 2) / (float(ref.norm() ** 2) + 1e-8 * ref.numel())
    return tot


def strict_with_kinks(oracle_run, compare, max_units=64):
    """Whole-network gradient checks at the STRICT tolerance.  A ReLU input within rounding of zero can land on
    different sides in two correct fp32 implementations; one flipped mask moves gradients by one summand of a sum over
    ~100 rows, far above 1e-4.  Instead of loosening the tolerance: the oracle pass is audited (oracle.path.relu_kinks)
    for units with |input| < KINK_TAU -- a few dozen out of ~10^6 -- and replayed with chosen units deciding the other
    way; a greedy search (one unit at a time, kept when it lowers the smooth mismatch score) has to arrive at an
    assignment for which the product's gradients agree to the strict tolerance.  Units outside the KINK_TAU band
    are never touched.  oracle_run() -> whatever compare needs (fresh leaves, gradients populated);
    compare(ref) -> (worst excess: <= 1 passes, smooth score).
    Returns (number of ambiguous units, number of units that had to decide against the oracle's sign)."""
    with op.relu_kinks(KINK_TAU) as log:
        ref = oracle_run()
    val = {}
    for (c, i, v) in log:
        val[(c, i)] = v
    units = sorted(val, key=lambda u: abs(val[u]))
    assert len(units) <= max_units, '%d ReLU inputs within %.0e of zero: search too large' % (len(units), KINK_TAU)
    excess, score = compare(ref)
    forced = {}
    sweeps = 0
    while excess > 1.0 and sweeps < 3:
        sweeps += 1
        changed = False
        for u in units:
            trial = dict(forced)
            if u in trial:
                del trial[u]                                  # back to the oracle's own sign
            else:
                trial[u] = not (val[u] > 0)                   # decide against it
            with op.relu_kinks(KINK_TAU, forced=trial):
                e, sc = compare(oracle_run())
            if sc < 0.5 * score:                              # (a unit that really decided the other way removes one
                excess, score, forced, changed = e, sc, trial, True   # whole summand: the score drops by far more than noise)
                if excess <= 1.0:
                    break
        if not changed:
            break
    assert excess <= 1.0, ('no assignment of the %d ambiguous ReLU units brings the gradients within the strict '
                           'tolerance: best %.3g x (flipped %d)' % (len(units), excess, len(forced)))
    return len(units), len(forced)


def leaf_sd(sd):
    return {k: v.clone().requires_grad_(True) for k, v in sd.items()}
