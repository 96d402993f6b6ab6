"""The rejected-call table of tests/test_gpu_contract_texts.py for the entry points of include/ext/occ4d_boxes.h: libocc4d.so and the
g++ twin take the argument contracts from one source (check_extents / check_choose of csrc/boxes_math.hpp over csrc/contract.hpp).
Both are loaded in one process -- the twin as a second plain handle, never enabled -- and handed the same rejected calls, device
tensors for the one and same-shaped host tensors for the other: the same status and the same occ4d_last_error() bytes."""
import pytest
import torch

import occlusions4d_amd as pk
from contract_texts import libraries, p, rejected_test, zeros_on  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = pk._lib.EINVAL


def extents(L, z, **k):
    """A 3 x 2 x 5 grid (30 points), two objects, three directions."""
    a = dict(labels=p(z(30)), nx=3, ny=2, nz=5, K=2, dirs=p(z(12)), A=3, extent=p(z(24)), zr=p(z(6)))
    a.update(k)
    return L.occ4d_boxes_extents_i32(*a.values(), None)


def choose(L, z, **k):
    """Two objects, three directions."""
    a = dict(extent=p(z(24)), zr=p(z(6)), dirs=p(z(12)), K=2, A=3, box=p(z(16)))
    a.update(k)
    return L.occ4d_boxes_choose_i32(*a.values(), None)


# (message fragment, call(L, z)): z(*shape) is an int32 zeros tensor where the library L reads
REJECTED = [
    ('occ4d_boxes_extents_i32: nx = -1, ny = 2, nz = 5 must be >= 0', lambda L, z: extents(L, z, nx=-1)),
    ('nx = 3, ny = 2, nz = -2147483648 must be >= 0', lambda L, z: extents(L, z, nz=-2 ** 31)),
    ('occ4d_boxes_extents_i32: nx = 2049, ny = 2, nz = 5 must be <= 2048', lambda L, z: extents(L, z, nx=2049)),
    ('nx = 3, ny = 2147483647, nz = 5 must be <= 2048', lambda L, z: extents(L, z, ny=2 ** 31 - 1)),
    ('occ4d_boxes_extents_i32: nx * ny * nz = 2147483648 exceeds INT32_MAX', lambda L, z: extents(L, z, nx=2048, ny=2048, nz=512)),
    ('nx * ny * nz = 8589934592 exceeds INT32_MAX', lambda L, z: extents(L, z, nx=2048, ny=2048, nz=2048)),
    ('occ4d_boxes_extents_i32: K = -1 must be >= 0', lambda L, z: extents(L, z, K=-1)),
    ('occ4d_boxes_extents_i32: A = 0 must be in [1, 256]', lambda L, z: extents(L, z, A=0)),
    ('A = 257 must be in [1, 256]', lambda L, z: extents(L, z, A=257)),
    ('A = -3 must be in [1, 256]', lambda L, z: extents(L, z, A=-3, K=0)),
    ('K * A * 4 = 2097152 * 256 * 4 exceeds INT32_MAX', lambda L, z: extents(L, z, K=2 ** 21, A=256)),
    ('occ4d_boxes_extents_i32: K * A * 4 = 536870912 * 1 * 4 exceeds INT32_MAX', lambda L, z: extents(L, z, K=2 ** 29, A=1)),
    ('occ4d_boxes_extents_i32: null labels with n = 30', lambda L, z: extents(L, z, labels=None)),
    ('occ4d_boxes_extents_i32: null dirs with A = 3', lambda L, z: extents(L, z, dirs=None)),
    ('occ4d_boxes_extents_i32: null extent with K = 2, A = 3', lambda L, z: extents(L, z, extent=None)),
    ('occ4d_boxes_extents_i32: null zr with K = 2', lambda L, z: extents(L, z, zr=None)),
    ('null dirs with A = 3', lambda L, z: extents(L, z, nx=0, labels=None, dirs=None)),
    ('occ4d_boxes_choose_i32: K = -5 must be >= 0', lambda L, z: choose(L, z, K=-5)),
    ('occ4d_boxes_choose_i32: A = 0 must be in [1, 256]', lambda L, z: choose(L, z, A=0)),
    ('occ4d_boxes_choose_i32: A = 257 must be in [1, 256]', lambda L, z: choose(L, z, A=257)),
    ('occ4d_boxes_choose_i32: K * A * 4 = 2097152 * 256 * 4 exceeds INT32_MAX', lambda L, z: choose(L, z, K=2 ** 21, A=256)),
    ('occ4d_boxes_choose_i32: null extent with K = 2, A = 3', lambda L, z: choose(L, z, extent=None)),
    ('occ4d_boxes_choose_i32: null zr with K = 2', lambda L, z: choose(L, z, zr=None)),
    ('occ4d_boxes_choose_i32: null dirs with A = 3', lambda L, z: choose(L, z, dirs=None)),
    ('occ4d_boxes_choose_i32: null box with K = 2', lambda L, z: choose(L, z, box=None)),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED)


def test_the_symbols_are_in_the_open_table_only():
    lib = pk._lib
    for name in ('occ4d_boxes_extents_i32', 'occ4d_boxes_choose_i32'):
        assert name in lib.ADDON_SIGNATURES
        for pinned in (lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
            assert name not in pinned


def test_accepted_edges_agree(libraries):
    """K == 0 is a no-op in both, with null pointers; an empty grid with K > 0 writes the EMPTY rows and takes null labels; A = 256
    and an axis of 2048 are accepted, and so are axes of length 1."""
    for L, dev in zip(libraries, (DEV, 'cpu')):
        z = zeros_on(dev)
        assert extents(L, z, K=0, labels=None, dirs=None, extent=None, zr=None) == pk._lib.OK
        assert choose(L, z, K=0, extent=None, zr=None, dirs=None, box=None) == pk._lib.OK
        extent, zr = z(24), z(6)
        assert extents(L, z, ny=0, labels=None, extent=p(extent), zr=p(zr)) == pk._lib.OK
        if dev != 'cpu':
            torch.cuda.synchronize()
        assert extent.cpu().tolist() == [2 ** 31 - 1, -2 ** 31] * 12 and zr.cpu().tolist() == [2 ** 31 - 1, -2 ** 31, 0] * 2
        assert extents(L, z, A=256, dirs=p(z(1024)), extent=p(z(2048))) == pk._lib.OK
        assert choose(L, z, A=256, dirs=p(z(1024)), extent=p(z(2048))) == pk._lib.OK
        assert extents(L, z, nx=2048, ny=1, nz=1, labels=p(z(2048))) == pk._lib.OK
        assert extents(L, z, nx=1, ny=2048, nz=1, labels=p(z(2048))) == pk._lib.OK
        assert extents(L, z, nx=1, ny=1, nz=2048, labels=p(z(2048))) == pk._lib.OK
        assert extents(L, z, nx=30, ny=1, nz=1) == pk._lib.OK and extents(L, z, nx=1, ny=1, nz=30) == pk._lib.OK
    torch.cuda.synchronize()
