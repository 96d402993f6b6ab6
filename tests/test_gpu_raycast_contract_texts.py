"""The rejected-call table of tests/test_gpu_contract_texts.py for the entry point of include/ext/occ4d_raycast.h: libocc4d.so and the
g++ twin take the argument contract from one source (check_raycast of csrc/raycast_math.hpp over csrc/contract.hpp).  Both are
loaded in one process -- the twin as a second plain handle, never enabled -- and handed the same rejected calls, device tensors for
the one and same-shaped host tensors for the other: the same status and the same occ4d_last_error() bytes."""
import ctypes

import pytest
import torch

import occlusions4d_amd as pk
from contract_texts import float_zeros_on as zeros_on, libraries, p, rejected_test  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = pk._lib.EINVAL
I32 = torch.int32
NAN, INF = float('nan'), float('inf')


def cols(*c):
    return (ctypes.c_int32 * len(c))(*c)


def cast(L, z, **k):
    """A 3 x 2 x 5 grid (30 points), two views of 4 x 6 pixels, two of three attribute columns."""
    a = dict(field=p(z(30)), ld=1, nx=3, ny=2, nz=5, x0=0.0, sx=1.0, y0=0.0, sy=1.0, z0=0.0, sz=1.0, level=0.5, k_inv=p(z(2, 16)),
             rt_inv=p(z(2, 16)), V=2, H=4, W=6, near=0.5, step=0.25, n_steps=8, attrs=p(z(30, 3)), ld_attr=3, d=3, cols_host=cols(0, 2),
             C=2, depth_background=0.0, feat_background=0.0, depth=p(z(2, 4, 6)), cell=p(z(2, 4, 6, dtype=I32)), feat=p(z(2, 4, 6, 2)))
    a.update(k)
    return L.occ4d_raycast_grid_f32(*a.values(), None)


# (message fragment, call(L, z)): z(*shape, dtype) is a zeros tensor where the library L reads
REJECTED = [
    ('occ4d_raycast_grid_f32: nx = 1, ny = 2, nz = 5 must be >= 2', lambda L, z: cast(L, z, nx=1)),
    ('nx = 3, ny = 0, nz = 5 must be >= 2', lambda L, z: cast(L, z, ny=0)),
    ('nx = 3, ny = 2, nz = -5 must be >= 2', lambda L, z: cast(L, z, nz=-5)),
    ('nx * ny * nz = 2048 * 1024 * 1024 exceeds INT32_MAX', lambda L, z: cast(L, z, nx=2048, ny=1024, nz=1024)),
    ('exceeds INT32_MAX', lambda L, z: cast(L, z, nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1)),
    ('ld = 0 must be >= 1', lambda L, z: cast(L, z, ld=0)),
    ('V = -1 must be >= 0, H = 4, W = 6 in 0 .. 32768', lambda L, z: cast(L, z, V=-1)),
    ('H = 32769', lambda L, z: cast(L, z, H=32769)),
    ('V H W = 2147483648 must be < 2^31', lambda L, z: cast(L, z, V=2, H=32768, W=32768)),
    ('step = 0 must be finite and > 0', lambda L, z: cast(L, z, step=0.0)),
    ('step = -0.25 must be finite and > 0', lambda L, z: cast(L, z, step=-0.25)),
    ('step = nan must be finite and > 0', lambda L, z: cast(L, z, step=NAN)),
    ('step = inf must be finite and > 0', lambda L, z: cast(L, z, step=INF)),
    ('near = nan must be finite', lambda L, z: cast(L, z, near=NAN)),
    ('near = -inf must be finite', lambda L, z: cast(L, z, near=-INF)),
    ('n_steps = 0 must be in 1 .. 65536', lambda L, z: cast(L, z, n_steps=0)),
    ('n_steps = 65537 must be in 1 .. 65536', lambda L, z: cast(L, z, n_steps=65537)),
    ('C = 33 must be in 0 .. 32', lambda L, z: cast(L, z, C=33)),
    ('C = -1 must be in 0 .. 32', lambda L, z: cast(L, z, C=-1)),
    ('null cols_host with C = 2', lambda L, z: cast(L, z, cols_host=None)),
    ('column 3 must be in 0 .. d - 1 = 2', lambda L, z: cast(L, z, cols_host=cols(0, 3))),
    ('column -1 must be in 0 .. d - 1 = 2', lambda L, z: cast(L, z, cols_host=cols(-1, 0))),
    ('d = 3, ld_attr = 2: need 1 <= d <= ld_attr', lambda L, z: cast(L, z, ld_attr=2)),
    ('d = 0, ld_attr = 3: need 1 <= d <= ld_attr', lambda L, z: cast(L, z, d=0)),
    ('null attrs with C = 2', lambda L, z: cast(L, z, attrs=None)),
    ('null field with n = 30', lambda L, z: cast(L, z, field=None)),
    ('null k_inv / rt_inv', lambda L, z: cast(L, z, k_inv=None)),
    ('null k_inv / rt_inv', lambda L, z: cast(L, z, rt_inv=None)),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED, zeros_on)


def test_accepted_edges_agree(libraries):
    """No views and an empty image are no-ops in both, with null pointers; no channels take null attrs / cols_host / feat; every
    output may be null; the limits themselves are accepted."""
    for L, dev in zip(libraries, (DEV, 'cpu')):
        z = zeros_on(dev)
        nothing = dict(field=None, k_inv=None, rt_inv=None, attrs=None, depth=None, cell=None, feat=None)
        assert cast(L, z, V=0, **nothing) == pk._lib.OK
        assert cast(L, z, H=0, **nothing) == pk._lib.OK
        assert cast(L, z, W=0, **nothing) == pk._lib.OK
        assert cast(L, z, C=0, attrs=None, cols_host=None, feat=None, ld_attr=0, d=0) == pk._lib.OK
        assert cast(L, z, depth=None, cell=None, feat=None) == pk._lib.OK
        assert cast(L, z, n_steps=65536, step=1e-6) == pk._lib.OK
        assert cast(L, z, C=32, cols_host=cols(*([1] * 32)), feat=p(z(2, 4, 6, 32))) == pk._lib.OK
    torch.cuda.synchronize()
