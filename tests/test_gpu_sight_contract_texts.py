"""The rejected-call table of tests/test_gpu_contract_texts.py for the entry points of include/ext/occ4d_sight.h: libocc4d.so and the
g++ twin take the argument contracts from one source (check_bits / check_grid of csrc/sight_math.hpp over csrc/contract.hpp).  Both
are loaded in one process -- the twin as a second plain handle, never enabled -- and handed the same rejected calls, device tensors
for the one and same-shaped host tensors for the other (the origins are host memory for both): the same status and the same
occ4d_last_error() bytes."""
import pytest
import torch

import occlusions4d_amd as pk
from contract_texts import host_int32, libraries, p, rejected_test, zeros_on  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = pk._lib.EINVAL
FAR = 2 ** 20


def origins(*rows):
    return host_int32(*rows, width=3)


def grid(L, z, **k):
    """A 3 x 2 x 5 grid (30 points, one word of bits), two origins."""
    a = dict(bits=p(z(1)), nx=3, ny=2, nz=5, origins_host=origins((0, 0, 0), (-1, 2, 7)), V=2, framed=p(z(30)), seen=p(z(30)),
             blocker=p(z(2, 30)), flags=0)
    a.update(k)
    return L.occ4d_sight_grid_u32(*a.values(), None)


def bits(L, z, **k):
    a = dict(field=p(z(30, dtype=torch.float32)), ld=1, level=0.5, mask=None, ld_mask=0, mask_level=0.0, n=30, bits=p(z(1)))
    a.update(k)
    return L.occ4d_sight_bits_f32(*a.values(), None)


# (message fragment, call(L, z)): z(*shape) is a zeros tensor (int32 unless it says float32) where the library L reads
REJECTED = [
    ('occ4d_sight_grid_u32: nx = -1, ny = 2, nz = 5 must be >= 0', lambda L, z: grid(L, z, nx=-1)),
    ('nx = 3, ny = -2, nz = -5 must be >= 0', lambda L, z: grid(L, z, ny=-2, nz=-5)),
    ('nx = 513, ny = 2, nz = 5 must be <= 512', lambda L, z: grid(L, z, nx=513)),
    ('nx = 3, ny = 2, nz = 65536 must be <= 512', lambda L, z: grid(L, z, nz=65536)),
    ('V = 0 must be in [1, 31]', lambda L, z: grid(L, z, V=0)),
    ('V = 32 must be in [1, 31]', lambda L, z: grid(L, z, V=32)),
    ('V = -1 must be in [1, 31]', lambda L, z: grid(L, z, V=-1)),
    ('origin 1 = (0, 1048577, 0) has a coordinate outside [-1048576, 1048576]', lambda L, z: grid(L, z, origins_host=origins((0, 0, 0), (0, FAR + 1, 0)))),
    ('origin 0 = (-1048577, 0, 0) has a coordinate outside', lambda L, z: grid(L, z, origins_host=origins((-FAR - 1, 0, 0), (0, 0, 0)))),
    ('origin 0 = (0, 0, -2147483648)', lambda L, z: grid(L, z, origins_host=origins((0, 0, -2 ** 31), (0, 0, 0)))),
    ('null bits with n = 30', lambda L, z: grid(L, z, bits=None)),
    ('null seen with n = 30', lambda L, z: grid(L, z, seen=None)),
    ('null origins_host with V = 2', lambda L, z: grid(L, z, origins_host=None)),
    ('flags = 1 must be 0: no flag bit exists', lambda L, z: grid(L, z, flags=1)),
    ('flags = 2 must be 0', lambda L, z: grid(L, z, flags=2)),
    ('flags = -2147483648 must be 0', lambda L, z: grid(L, z, flags=-2 ** 31)),
    ('occ4d_sight_bits_f32: n = -1 must be in [0, INT32_MAX]', lambda L, z: bits(L, z, n=-1)),
    ('n = 2147483648 must be in [0, INT32_MAX]', lambda L, z: bits(L, z, n=2 ** 31)),
    ('ld = 0 must be >= 1', lambda L, z: bits(L, z, ld=0)),
    ('ld_mask = 0 must be >= 1', lambda L, z: bits(L, z, mask=p(z(30, dtype=torch.float32)))),
    ('null field with n = 30', lambda L, z: bits(L, z, field=None)),
    ('null bits with n = 30', lambda L, z: bits(L, z, bits=None)),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED)


def test_accepted_edges_agree(libraries):
    """An empty grid is a no-op in both, with null pointers; axes of length 1 and 512, V = 1 and 31, origins at +-2^20,
    null framed and null blocker are accepted."""
    for L, dev in zip(libraries, (DEV, 'cpu')):
        z = zeros_on(dev)
        nothing = dict(bits=None, origins_host=None, framed=None, seen=None, blocker=None)
        assert grid(L, z, nx=0, **nothing) == pk._lib.OK and grid(L, z, ny=0, nz=0, **nothing) == pk._lib.OK
        assert bits(L, z, n=0, field=None, bits=None) == pk._lib.OK
        assert grid(L, z, nx=30, ny=1, nz=1) == pk._lib.OK and grid(L, z, nx=1, ny=1, nz=30) == pk._lib.OK
        assert grid(L, z, nx=1, ny=512, nz=1, bits=p(z(16)), framed=p(z(512)), seen=p(z(512)), blocker=p(z(2, 512))) == pk._lib.OK
        assert grid(L, z, V=1, framed=None, blocker=None) == pk._lib.OK
        assert grid(L, z, V=31, origins_host=origins(*[(v, -v, 2 * v) for v in range(31)]), blocker=p(z(31, 30))) == pk._lib.OK
        assert grid(L, z, origins_host=origins((FAR, -FAR, FAR), (-FAR, FAR, -FAR))) == pk._lib.OK
        assert bits(L, z) == pk._lib.OK and bits(L, z, mask=p(z(30, dtype=torch.float32)), ld_mask=1) == pk._lib.OK
    torch.cuda.synchronize()
