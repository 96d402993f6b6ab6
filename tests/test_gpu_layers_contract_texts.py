"""The rejected-call table of tests/test_gpu_contract_texts.py for the entry point of include/ext/occ4d_layers.h: libocc4d.so and the
g++ twin take the argument contract from one source (check_layers of csrc/layers_math.hpp over csrc/contract.hpp).  Both are loaded in
one process -- the twin as a second plain handle, never enabled -- and handed the same rejected calls, device tensors for the one
and same-shaped host tensors for the other: the same status and the same occ4d_last_error() bytes."""
import pytest
import torch

import occlusions4d_amd as pk
from contract_texts import libraries, p, rejected_test, zeros_on  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = pk._lib.EINVAL
I32, F32 = torch.int32, torch.float32
INF, NAN = float('inf'), float('nan')


def march(lib, z, **k):
    """A 3 x 2 x 5 grid (30 points), two objects, one view of 4 x 4 pixels, two layers, four samples."""
    a = dict(labels=p(z(30)), nx=3, ny=2, nz=5, K=2, x0=0.0, sx=1.0, y0=0.0, sy=1.0, z0=0.0, sz=1.0, k_inv=p(z(16, dtype=F32)),
             rt_inv=p(z(16, dtype=F32)), V=1, H=4, W=4, near=0.1, step=0.1, n_steps=4, L=2, label=p(z(32)), first=p(z(32)),
             samples=p(z(32)), point=p(z(32)), count=p(z(16)), table=p(z(14)), status=p(z(2)))
    a.update(k)
    return lib.occ4d_layers_march_i32(*a.values(), None)


# (message fragment, call(L, z)): z(*shape) is a zeros tensor where the library L reads
REJECTED = [
    ('occ4d_layers_march_i32: nx = 1, ny = 2, nz = 5 must be >= 2', lambda L, z: march(L, z, nx=1)),
    ('nx = 3, ny = 2, nz = -2147483648 must be >= 2', lambda L, z: march(L, z, nz=-2 ** 31)),
    ('occ4d_layers_march_i32: nx * ny * nz = 65536 * 65536 * 2 exceeds INT32_MAX', lambda L, z: march(L, z, nx=65536, ny=65536, nz=2)),
    ('nx * ny * nz = 2048 * 2048 * 512 exceeds INT32_MAX', lambda L, z: march(L, z, nx=2048, ny=2048, nz=512)),
    ('occ4d_layers_march_i32: V = -1 must be >= 0, H = 4, W = 4 in 0 .. 32768', lambda L, z: march(L, z, V=-1)),
    ('V = 1 must be >= 0, H = 32769, W = 4 in 0 .. 32768', lambda L, z: march(L, z, H=32769)),
    ('V = 1 must be >= 0, H = 4, W = -2 in 0 .. 32768', lambda L, z: march(L, z, W=-2)),
    ('occ4d_layers_march_i32: V H W = 2147483648 must be < 2^31', lambda L, z: march(L, z, V=2, H=32768, W=32768)),
    ('occ4d_layers_march_i32: step = 0 must be finite and > 0', lambda L, z: march(L, z, step=0.0)),
    ('step = -0.5 must be finite and > 0', lambda L, z: march(L, z, step=-0.5)),
    ('step = inf must be finite and > 0', lambda L, z: march(L, z, step=INF)),
    ('step = nan must be finite and > 0', lambda L, z: march(L, z, step=NAN)),
    ('occ4d_layers_march_i32: near = inf must be finite', lambda L, z: march(L, z, near=INF)),
    ('near = -inf must be finite', lambda L, z: march(L, z, near=-INF)),
    ('near = nan must be finite', lambda L, z: march(L, z, near=NAN)),
    ('occ4d_layers_march_i32: n_steps = 0 must be in 1 .. 65536', lambda L, z: march(L, z, n_steps=0)),
    ('n_steps = 65537 must be in 1 .. 65536', lambda L, z: march(L, z, n_steps=65537)),
    ('occ4d_layers_march_i32: K = -1 must be >= 0', lambda L, z: march(L, z, K=-1)),
    ('occ4d_layers_march_i32: V max(K, 1) 7 = 1 * 306783379 * 7 must be < 2^31', lambda L, z: march(L, z, K=306783379)),
    ('V max(K, 1) 7 = 306783379 * 1 * 7 must be < 2^31', lambda L, z: march(L, z, V=306783379, H=1, W=1, K=0)),
    ('occ4d_layers_march_i32: L = 0 must be in 1 .. 8', lambda L, z: march(L, z, L=0)),
    ('L = 9 must be in 1 .. 8', lambda L, z: march(L, z, L=9)),
    ('L = -1 must be in 1 .. 8', lambda L, z: march(L, z, L=-1, V=0)),
    ('occ4d_layers_march_i32: V H W L = 2147483648 must be < 2^31', lambda L, z: march(L, z, H=32768, W=8192, L=8)),
    ('occ4d_layers_march_i32: null labels with n = 30', lambda L, z: march(L, z, labels=None)),
    ('occ4d_layers_march_i32: null k_inv / rt_inv', lambda L, z: march(L, z, k_inv=None)),
    ('null k_inv / rt_inv', lambda L, z: march(L, z, rt_inv=None)),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED)


def test_the_symbol_is_in_the_open_table_only():
    lib = pk._lib
    assert 'occ4d_layers_march_i32' in lib.ADDON_SIGNATURES
    for pinned in (lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
        assert 'occ4d_layers_march_i32' not in pinned


def test_accepted_edges_agree(libraries):
    """V == 0, H W == 0 and all outputs null are no-ops in both, with null inputs; K == 0 takes a null table and writes none; L = 8,
    n_steps = 1 and each output alone are accepted."""
    nothing = dict(label=None, first=None, samples=None, point=None, count=None, table=None, status=None)
    for L, dev in zip(libraries, (DEV, 'cpu')):
        z = zeros_on(dev)
        assert march(L, z, V=0, labels=None, k_inv=None, rt_inv=None, **nothing) == pk._lib.OK
        assert march(L, z, H=0, labels=None, k_inv=None, rt_inv=None) == pk._lib.OK
        assert march(L, z, W=0, labels=None, k_inv=None, rt_inv=None) == pk._lib.OK
        assert march(L, z, labels=None, k_inv=None, rt_inv=None, **nothing) == pk._lib.OK
        assert march(L, z, K=0, labels=None, k_inv=None, rt_inv=None, **dict(nothing, table=p(z(14)))) == pk._lib.OK
        table, status = torch.full((14,), 5, dtype=I32, device=dev), torch.full((2,), 5, dtype=I32, device=dev)
        assert march(L, z, K=0, table=p(table), status=p(status)) == pk._lib.OK
        if dev != 'cpu':
            torch.cuda.synchronize()
        assert table.cpu().tolist() == [5] * 14 and status.cpu().tolist() == [0, 0]
        assert march(L, z, L=8, label=p(z(128)), first=p(z(128)), samples=p(z(128)), point=p(z(128))) == pk._lib.OK
        assert march(L, z, n_steps=1) == pk._lib.OK
        for name in nothing:
            assert march(L, z, **dict(nothing, **{name: p(z(32))})) == pk._lib.OK
    torch.cuda.synchronize()
