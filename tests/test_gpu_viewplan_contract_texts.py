"""The rejected-call table of tests/test_gpu_contract_texts.py for the entry points of include/ext/occ4d_viewplan.h: libocc4d.so and
the g++ twin take the argument contracts from one source (check_visible / check_greedy of csrc/viewplan_math.hpp over
csrc/contract.hpp).  Both are loaded in one process -- the twin as a second plain handle, never enabled -- and handed the same
rejected calls, device tensors for the one and same-shaped host tensors for the other: the same status and the same
occ4d_last_error() bytes."""
import pytest
import torch

import occlusions4d_amd as pk
from contract_texts import libraries, p, rejected_test, zeros_on  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = pk._lib.EINVAL


def visible(L, z, **k):
    """A 3 x 2 x 5 grid (30 points, one word), four candidates."""
    a = dict(solid=p(z(1)), nx=3, ny=2, nz=5, targets=p(z(1)), candidates=p(z(12)), C=4, wx=1, wy=1, wz=1, max_dist2=-1, vis=p(z(4)))
    a.update(k)
    return L.occ4d_viewplan_visible_u32(*a.values(), None)


def greedy(L, z, **k):
    """Four rows of one word, three picks."""
    a = dict(vis=p(z(4)), C=4, W=1, targets=p(z(1)), k=3, work=p(z(7)), gain=p(z(4)), picks=p(z(3)), pick_gain=p(z(3)), status=p(z(2)))
    a.update(k)
    return L.occ4d_viewplan_greedy_u32(*a.values(), None)


# (message fragment, call(L, z)): z(*shape) is an int32 zeros tensor where the library L reads
REJECTED = [
    ('occ4d_viewplan_visible_u32: nx = -1, ny = 2, nz = 5 must be >= 0', lambda L, z: visible(L, z, nx=-1)),
    ('occ4d_viewplan_visible_u32: nx = 513, ny = 2, nz = 5 must be <= 512', lambda L, z: visible(L, z, nx=513)),
    ('nx = 3, ny = 2, nz = 2147483647 must be <= 512', lambda L, z: visible(L, z, nz=2 ** 31 - 1)),
    ('occ4d_viewplan_visible_u32: C = -1 must be in [0, 4096]', lambda L, z: visible(L, z, C=-1)),
    ('C = 4097 must be in [0, 4096]', lambda L, z: visible(L, z, C=4097)),
    ('wx = 0, wy = 1, wz = 1 must be in [1, 1024]', lambda L, z: visible(L, z, wx=0)),
    ('wx = 1, wy = 1025, wz = 1 must be in [1, 1024]', lambda L, z: visible(L, z, wy=1025)),
    ('wx = 1, wy = 1, wz = -3 must be in [1, 1024]', lambda L, z: visible(L, z, wz=-3)),
    ('C * W = 4096 * 1048576 exceeds INT32_MAX', lambda L, z: visible(L, z, nx=512, ny=512, nz=128, C=4096)),
    ('occ4d_viewplan_visible_u32: null solid with n = 30', lambda L, z: visible(L, z, solid=None)),
    ('occ4d_viewplan_visible_u32: null targets with n = 30', lambda L, z: visible(L, z, targets=None)),
    ('null candidates with C = 4', lambda L, z: visible(L, z, candidates=None)),
    ('null vis with C = 4, n = 30', lambda L, z: visible(L, z, vis=None)),
    ('occ4d_viewplan_greedy_u32: C = -2 must be in [0, 4096]', lambda L, z: greedy(L, z, C=-2)),
    ('occ4d_viewplan_greedy_u32: C = 4097 must be in [0, 4096]', lambda L, z: greedy(L, z, C=4097)),
    ('W = -1 must be >= 0', lambda L, z: greedy(L, z, W=-1)),
    ('occ4d_viewplan_greedy_u32: k = -1 must be in [0, 32]', lambda L, z: greedy(L, z, k=-1)),
    ('k = 33 must be in [0, 32]', lambda L, z: greedy(L, z, k=33)),
    ('C * W = 4 * 536870912 exceeds INT32_MAX', lambda L, z: greedy(L, z, W=2 ** 29)),
    ('occ4d_viewplan_greedy_u32: null vis with C = 4, W = 1', lambda L, z: greedy(L, z, vis=None)),
    ('occ4d_viewplan_greedy_u32: null targets with W = 1', lambda L, z: greedy(L, z, targets=None)),
    ('null work with C = 4, W = 1', lambda L, z: greedy(L, z, work=None)),
    ('null gain / status with C = 4', lambda L, z: greedy(L, z, gain=None)),
    ('null gain / status with C = 4', lambda L, z: greedy(L, z, status=None)),
    ('null picks / pick_gain with k = 3', lambda L, z: greedy(L, z, picks=None)),
    ('null picks / pick_gain with k = 3', lambda L, z: greedy(L, z, pick_gain=None)),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED)


def test_the_symbols_are_in_the_open_table_only():
    lib = pk._lib
    for name in ('occ4d_viewplan_visible_u32', 'occ4d_viewplan_greedy_u32'):
        assert name in lib.ADDON_SIGNATURES
        for pinned in (lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
            assert name not in pinned


def test_accepted_edges_agree(libraries):
    """An empty grid, an empty candidate list and an empty word array are no-ops in both, with null pointers; picks and pick_gain may
    be null with k == 0; axes of length 1, the longest axis, the extreme weights and the extreme values of max_dist2 are accepted."""
    for L, dev in zip(libraries, (DEV, 'cpu')):
        z = zeros_on(dev)
        nothing = dict(solid=None, targets=None, candidates=None, vis=None)
        assert visible(L, z, ny=0, **nothing) == pk._lib.OK
        assert visible(L, z, C=0, **nothing) == pk._lib.OK
        assert visible(L, z, nx=30, ny=1, nz=1) == pk._lib.OK and visible(L, z, nx=1, ny=1, nz=30) == pk._lib.OK
        assert visible(L, z, nx=512, ny=1, nz=1, solid=p(z(16)), targets=p(z(16)), vis=p(z(64))) == pk._lib.OK
        assert visible(L, z, wx=1024, wy=1, wz=1024, max_dist2=2 ** 63 - 1) == pk._lib.OK
        assert visible(L, z, max_dist2=-2 ** 63) == pk._lib.OK and visible(L, z, max_dist2=0) == pk._lib.OK
        empty = dict(vis=None, targets=None, work=None, gain=None, picks=None, pick_gain=None, status=None)
        assert greedy(L, z, C=0, **empty) == pk._lib.OK
        assert greedy(L, z, W=0, **empty) == pk._lib.OK
        assert greedy(L, z, k=0, picks=None, pick_gain=None) == pk._lib.OK
        assert greedy(L, z, k=32, picks=p(z(32)), pick_gain=p(z(32))) == pk._lib.OK
    torch.cuda.synchronize()
