"""The rejected-call table of tests/test_gpu_contract_texts.py for the entry point of include/ext/occ4d_distance.h: libocc4d.so and the
g++ twin take the argument contract from one source (check_distance of csrc/distance_math.hpp over csrc/contract.hpp).  Both are
loaded in one process -- the twin as a second plain handle, never enabled -- and handed the same rejected calls, device tensors for
the one and same-shaped host tensors for the other: the same status and the same occ4d_last_error() bytes."""
import pytest
import torch

import occlusions4d_amd as pk
from contract_texts import float_zeros_on as zeros_on, libraries, p, rejected_test  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = pk._lib.EINVAL
I32 = torch.int32
NAN = float('nan')


def grid(L, z, **k):
    """A 3 x 2 x 5 grid (30 points)."""
    a = dict(field=p(z(30)), ld=1, level=0.5, mask=p(z(30)), ld_mask=1, mask_level=0.5, target=0, nx=3, ny=2, nz=5, wx=1, wy=1, wz=1,
             dist2=p(z(30, dtype=I32)), nearest=p(z(30, dtype=I32)))
    a.update(k)
    return L.occ4d_distance_grid_f32(*a.values(), None)


def line(L, z, **k):
    """A 3 x 1 x 1 grid: the largest cost is 4 * wx."""
    return grid(L, z, **dict(dict(field=p(z(3)), mask=None, nx=3, ny=1, nz=1, dist2=p(z(3, dtype=I32)), nearest=p(z(3, dtype=I32))), **k))


# (message fragment, call(L, z)): z(*shape, dtype) is a zeros tensor where the library L reads
REJECTED = [
    ('occ4d_distance_grid_f32: nx = -1, ny = 2, nz = 5 must be >= 0', lambda L, z: grid(L, z, nx=-1)),
    ('nx = 3, ny = -2, nz = -5 must be >= 0', lambda L, z: grid(L, z, ny=-2, nz=-5)),
    ('occ4d_distance_grid_f32: nx * ny * nz = 2048 * 1024 * 1024 exceeds INT32_MAX', lambda L, z: grid(L, z, nx=2048, ny=1024, nz=1024)),
    ('exceeds INT32_MAX', lambda L, z: grid(L, z, nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1)),
    ('nx = 513, ny = 2, nz = 5 must be <= 512', lambda L, z: grid(L, z, nx=513)),
    ('nx = 3, ny = 2, nz = 513 must be <= 512', lambda L, z: grid(L, z, nz=513)),
    ('occ4d_distance_grid_f32: ld = 0 must be >= 1', lambda L, z: grid(L, z, ld=0)),
    ('ld = -3 must be >= 1', lambda L, z: grid(L, z, ld=-3)),
    ('ld_mask = 0 must be >= 1', lambda L, z: grid(L, z, ld_mask=0)),
    ('wx = 0, wy = 1, wz = 1 must be >= 1', lambda L, z: grid(L, z, wx=0)),
    ('wx = 1, wy = 1, wz = 0 must be >= 1', lambda L, z: grid(L, z, wz=0)),
    ('wx = 1, wy = -7, wz = 1 must be >= 1', lambda L, z: grid(L, z, wy=-7)),
    ('the largest cost 2147483648 = 536870912 * 2^2 + 1 * 0^2 + 1 * 0^2 exceeds INT32_MAX - 1', lambda L, z: line(L, z, wx=536870912)),
    ('the largest cost 2147483647 = ', lambda L, z: grid(L, z, wx=2 ** 31 - 1 - 4 * 536870911, wy=3, wz=536870911 // 4)),
    ('target = 2 must be 0 or 1', lambda L, z: grid(L, z, target=2)),
    ('target = -1 must be 0 or 1', lambda L, z: grid(L, z, target=-1)),
    ('null field with n = 30', lambda L, z: grid(L, z, field=None)),
    ('null dist2 with n = 30', lambda L, z: grid(L, z, dist2=None)),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED, zeros_on)


def test_accepted_edges_agree(libraries):
    """An empty grid is a no-op in both, with null pointers; the mask and nearest may be null; axes of length 1, a NaN level, both
    targets and the last legal weight are accepted."""
    for L, dev in zip(libraries, (DEV, 'cpu')):
        z = zeros_on(dev)
        nothing = dict(field=None, mask=None, dist2=None, nearest=None)
        assert grid(L, z, nx=0, **nothing) == pk._lib.OK
        assert grid(L, z, ny=0, nz=0, **nothing) == pk._lib.OK
        assert grid(L, z, mask=None, ld_mask=0) == pk._lib.OK
        assert grid(L, z, nearest=None) == pk._lib.OK
        assert grid(L, z, mask=None, nearest=None, target=1) == pk._lib.OK
        assert grid(L, z, nx=30, ny=1, nz=1) == pk._lib.OK and grid(L, z, nx=1, ny=1, nz=30) == pk._lib.OK
        assert grid(L, z, nx=1, ny=30, nz=1) == pk._lib.OK
        assert grid(L, z, level=NAN, mask_level=NAN) == pk._lib.OK
        assert line(L, z, wx=536870911) == pk._lib.OK
    torch.cuda.synchronize()
