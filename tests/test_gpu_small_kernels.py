"""Direct tests of the small kernels that the suite reached only through one or two golden fixtures: BatchNorm training
forward / backward, swish and its backward, the Fourier features, the interpolation weights and the attention-MLP
argument, each against an fp64 statement of the same op at the edges of its tiling and of its value range.

Error measure and bounds are those of tests/test_gpu_kernels_random.py: _rel = max|got - ref| / max|ref|; 3e-6 for
elementwise kernels and plain column sums, 2e-5 for the normalisation kernels (its LayerNorm bound).  The Fourier
features have a bound of their own: 4 x the error of numpy's float32 sin / cos against the same fp64 values, at least
2^-23 (measured on the MI355X: numpy fp32 at most 6.9e-08, bound at least 2.68e-07, kernel at most 6.9e-08 over the six cases)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ELEMENTWISE, NORMALISATION = 3e-6, 2e-5


@pytest.fixture(scope='module')
def pk():
    import occlusions4d_amd
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    occlusions4d_amd._lib.lib()
    return occlusions4d_amd


def C(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rel(got, ref):
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().numpy().astype(np.float64) if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    return np.abs(got - ref).max() / max(1e-6, np.abs(ref).max())


def _strided(a, pad, off=0):
    """`a` on the device as a view of a buffer of noise with `pad` more columns."""
    rng = np.random.default_rng(a.size)
    wide = rng.normal(size=(a.shape[0], a.shape[1] + pad)).astype(np.float32)
    wide[:, off:off + a.shape[1]] = a
    return C(wide)[:, off:off + a.shape[1]]


# ------------------------------------------------------------------------------------------ BatchNorm (training) + ReLU
@pytest.mark.parametrize('n', [2, 511, 512, 513, 14336])       # both sides of the 512-row chunk of the statistics
@pytest.mark.parametrize('d', [1, 63, 64, 65, 144])            # both sides of the 64-column workgroup
def test_batchnorm_training_forward_and_backward(pk, n, d):
    rng = np.random.default_rng(1000 * n + d)
    y = rng.normal(size=(n, d)).astype(np.float32) * rng.uniform(0.5, 2.0, size=(1, d)).astype(np.float32)
    if d >= 63:
        y[:, 5] = np.float32(2.5)                               # constant column: variance exactly 0, eps governs
        if n >= 511:
            # mean = 1e3 x spread.  (Not with 2 rows: the batch mean is returned in fp32, and half an ulp of 1000 is
            # 3e-5 of a spread of 1 -- with hundreds of rows max|out| >= 3 and that stays inside the bound.)
            y[:, 7] = np.float32(1000.0) + rng.normal(size=n).astype(np.float32)
    if n == 2:
        # Two rows: xhat = +-1 / sqrt(1 + eps / var) and dx is what is left of gm - dbeta / 2 - xhat dgamma / 2 after they
        # cancel to O(eps / var): with var >> eps the problem itself loses log10(var / eps) digits in any fp32 evaluation.
        # A spread of 0.03 puts var at eps, where the two-row case is as well conditioned as the others.
        y *= np.float32(0.03)
    gamma = rng.uniform(0.5, 1.5, size=d).astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, size=d).astype(np.float32)
    g = rng.normal(size=(n, d)).astype(np.float32)
    eps = 1e-3
    yt = torch.from_numpy(y).double().requires_grad_(True)
    gt, bt = torch.from_numpy(gamma).double().requires_grad_(True), torch.from_numpy(beta).double().requires_grad_(True)
    pre = torch.nn.functional.batch_norm(yt, None, None, gt, bt, True, 0.1, eps)
    yd, gd = _strided(y, 3, 1), _strided(g, 5, 2)
    out, mean, var = pk.ops.bn_train_fwd(yd, C(gamma), C(beta), eps)
    mref, vref = y.astype(np.float64).mean(axis=0), y.astype(np.float64).var(axis=0)
    assert _rel(mean, mref) <= ELEMENTWISE and _rel(var, vref) <= ELEMENTWISE
    if d >= 63:
        assert float(var[5]) == 0.0
    assert _rel(out, torch.relu(pre).detach()) <= NORMALISATION
    # Backward through the ReLU: where the fp64 pre-activation lies within fp32 rounding of 0 (1e-6; 5e-5 in the column
    # whose fp32 mean carries half an ulp of 1000) either side is a valid fp32 answer, and the reference takes the kernel's.
    thr = torch.full((d,), 1e-6, dtype=torch.float64)
    if d >= 63 and n >= 511:
        thr[7] = 5e-5
    mask = torch.where(pre.detach().abs() < thr, out.cpu() > 0, pre.detach() > 0).double()
    (pre * mask).backward(torch.from_numpy(g).double())
    dx, dgamma, dbeta = pk.ops.bn_train_bwd(yd, gd, out, mean, var, C(gamma), eps)
    assert _rel(dx, yt.grad) <= NORMALISATION
    assert _rel(dgamma, gt.grad) <= NORMALISATION and _rel(dbeta, bt.grad) <= NORMALISATION


def test_batchnorm_training_needs_two_rows(pk):
    y = C(np.ones((1, 8), np.float32))
    with pytest.raises(AssertionError, match='at least 2'):
        pk.ops.bn_train_fwd(y, torch.ones(8, device='cuda'), torch.zeros(8, device='cuda'), 1e-3)
    with pytest.raises(AssertionError):
        pk.ops.bn_train_bwd(y, y, y, torch.zeros(8, device='cuda'), torch.ones(8, device='cuda'), torch.ones(8, device='cuda'), 1e-3)


# ------------------------------------------------------------------------------------------ swish
@pytest.mark.parametrize('span', [8.0, 100.0])
def test_swish_and_its_backward_over_the_sigmoid_range(pk, span):
    """|x| up to 100: the sigmoid saturates (1 above, 0 below: x sigmoid(x) is denormal at -100); +-0; strided rows.  Two
    spans, so that the error of the moderate values is not measured against the largest magnitude."""
    rng = np.random.default_rng(int(span))
    x = rng.uniform(-span, span, size=(37, 130)).astype(np.float32)
    x[0, :4] = [0.0, -0.0, span, -span]
    if span == 100.0:
        x[0, 4:6] = [-87.5, 88.5]                               # either side of where exp(-x) leaves the fp32 range
    g = rng.normal(size=x.shape).astype(np.float32)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    ref = xt * torch.sigmoid(xt)
    ref.backward(torch.from_numpy(g).double())
    xd, gd = _strided(x, 3, 2), _strided(g, 7, 1)
    y = pk.ops.swish(xd)
    dx = pk.ops.swish_bwd(gd, xd)
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    assert _rel(y, ref.detach()) <= ELEMENTWISE and _rel(dx, xt.grad) <= ELEMENTWISE
    assert float(y[0, 0]) == 0.0 and float(y[0, 1]) == 0.0
    if span == 100.0:
        assert abs(float(y[0, 3])) <= 1e-37 and float(y[0, 2]) == 100.0     # -100 sigmoid(-100) = -3.7e-42
    assert float(dx[0, 0]) == 0.5 * float(g[0, 0])


# ------------------------------------------------------------------------------------------ Fourier features
@pytest.mark.parametrize('c', [3, 4])
@pytest.mark.parametrize('reach', [5.0, 16.0, 60.0])            # GREATER cube, CARLA cube, 3 x outside it (far queries)
def test_posenc_against_fp64_sin_cos_of_the_fp32_product(pk, c, reach):
    n_freq, base = 8, 0.1                                       # both published configurations
    rng = np.random.default_rng(int(reach) + c)
    n = 3001
    p = rng.uniform(-reach, reach, size=(n, c)).astype(np.float32)
    p[0] = 0.0
    p[1] = reach
    width = c * (2 * n_freq + 1)
    w = np.array([np.float32(base * 2.0 ** f * np.pi * 2.0) for f in range(n_freq)], np.float32)
    arg = p[:, None, :] * w[None, :, None]                      # the fp32 product the contract fixes: (n, f, c)
    ref = np.concatenate([p.astype(np.float64)] + [fn(arg[:, f].astype(np.float64)) for f in range(n_freq) for fn in (np.sin, np.cos)], axis=1)
    np32 = np.concatenate([p] + [fn(arg[:, f]) for f in range(n_freq) for fn in (np.sin, np.cos)], axis=1)
    e32 = float(np.abs(np32.astype(np.float64) - ref).max())
    bound = max(4.0 * e32, 2.0 ** -23)
    lib, P = pk._lib.lib(), pk.ops._ptr
    ldo = width + 5
    buf = torch.full((n + 2, ldo), -7.0, device='cuda')
    pts = _strided(p, 4 if c == 4 else 5)
    pk._lib.check(lib.occ4d_posenc_f32(P(pts), pts.stride(0), n, c, n_freq, base, P(buf), ldo, pk.ops._stream()))
    got = buf[:n, :width].double().cpu().numpy()
    err = float(np.abs(got - ref).max())
    print('\n[posenc] c %d reach %g: numpy fp32 %.3g  bound %.3g  kernel %.3g' % (c, reach, e32, bound, err))
    assert err <= bound
    assert np.array_equal(got[:, :c], p.astype(np.float64))
    assert bool((buf[:n, width:] == -7.0).all()) and bool((buf[n:] == -7.0).all())      # padding and rows behind: untouched
    assert torch.equal(pk.ops.posenc(pts, n_freq, base), buf[:n, :width])


# ------------------------------------------------------------------------------------------ interpolation weights
@pytest.mark.parametrize('k', range(1, 9))
def test_interp_weights_edges(pk, k):
    rng = np.random.default_rng(k)
    dist = rng.uniform(0.01, 3.0, size=(257, k)).astype(np.float32)
    dist[0, 0] = 0.0                                            # a query ON a point: 1 / 1e-4 dominates
    dist[1] = 0.0                                               # all zero
    dist[2] = np.float32(0.731)                                 # all equal: 1 / k each
    dist[3, -1] = np.float32(1e30)                              # one enormous distance: weight ~ 0, the rest unharmed
    dist[4] = np.float32(1e30)                                  # all enormous
    t = 1.0 / (dist.astype(np.float64) + 1e-4)
    ref = t / np.maximum(np.abs(t).sum(axis=1, keepdims=True), 1e-12)
    got = pk.ops.interp_weights(C(dist))
    assert torch.isfinite(got).all()
    assert _rel(got, ref) <= ELEMENTWISE
    floor_rows = [4] if k > 1 else [3, 4]                       # every distance enormous: the 1e-12 floor of the sum governs
    assert np.abs(np.delete(got.double().cpu().numpy(), floor_rows, axis=0).sum(axis=1) - 1.0).max() <= 1e-6
    assert _rel(got[2], np.full(k, 1.0 / k)) <= ELEMENTWISE


# ------------------------------------------------------------------------------------------ argument of attn_mlp
@pytest.mark.parametrize('n,m,k,d', [(1, 1, 1, 1), (37, 5, 16, 36), (200, 76, 14, 416), (513, 300, 3, 65)])
def test_attn_in_strided_and_repeated_indices(pk, n, m, k, d):
    rng = np.random.default_rng(n + d)
    q = rng.normal(size=(n, d)).astype(np.float32)
    kf = rng.normal(size=(m, d)).astype(np.float32)
    pe = rng.normal(size=(n * k, d)).astype(np.float32)
    idx = rng.integers(0, m, size=(n, k)).astype(np.int32)
    idx[0] = idx[0, 0]                                          # a row of one index
    idx[-1, ::2] = m - 1
    ref = (q.astype(np.float64)[:, None] - kf.astype(np.float64)[idx.astype(np.int64)]).reshape(n * k, d) + pe
    got = pk.ops.pt_attn_in(_strided(q, 3, 1), _strided(kf, 6, 2), C(pe), C(idx))
    assert _rel(got, ref) <= ELEMENTWISE
    assert np.array_equal(got.cpu().numpy(), ((q[:, None] - kf[idx.astype(np.int64)]).reshape(n * k, d) + pe))
