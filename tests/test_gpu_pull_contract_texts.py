"""The rejected-call table of tests/test_gpu_contract_texts.py for the entry points of include/ext/occ4d_pull.h: libocc4d.so and the
g++ twin take the argument contracts from one source (check_bits / check_pairs / check_paths of csrc/pull_math.hpp over
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


def bits(L, z, **k):
    a = dict(clear=p(z(30)), min_clear=1, n=30, blocked=p(z(1)))
    a.update(k)
    return L.occ4d_pull_bits_i32(*a.values(), None)


def pairs(L, z, **k):
    """A 3 x 2 x 5 grid (30 points, one word), four pairs."""
    a = dict(blocked=p(z(1)), nx=3, ny=2, nz=5, a=p(z(4)), b=p(z(4)), n_pairs=4, hit=p(z(4)))
    a.update(k)
    return L.occ4d_pull_pairs_u32(*a.values(), None)


def paths(L, z, **k):
    """The same grid, two goals, cap 4."""
    a = dict(blocked=p(z(1)), nx=3, ny=2, nz=5, paths=p(z(8)), path_len=p(z(2)), n_goals=2, cap=4, waypoints=p(z(8)), waypoint_len=p(z(2)))
    a.update(k)
    return L.occ4d_pull_paths_i32(*a.values(), None)


# (message fragment, call(L, z)): z(*shape) is an int32 zeros tensor where the library L reads
REJECTED = [
    ('occ4d_pull_bits_i32: n = -1 must be in [0, INT32_MAX]', lambda L, z: bits(L, z, n=-1)),
    ('n = 2147483648 must be in [0, INT32_MAX]', lambda L, z: bits(L, z, n=2 ** 31)),
    ('occ4d_pull_bits_i32: null clear with n = 30', lambda L, z: bits(L, z, clear=None)),
    ('occ4d_pull_bits_i32: null blocked with n = 30', lambda L, z: bits(L, z, blocked=None)),
    ('occ4d_pull_pairs_u32: nx = -1, ny = 2, nz = 5 must be >= 0', lambda L, z: pairs(L, z, nx=-1)),
    ('occ4d_pull_pairs_u32: nx = 513, ny = 2, nz = 5 must be <= 512', lambda L, z: pairs(L, z, nx=513)),
    ('nx = 3, ny = 2, nz = 2147483647 must be <= 512', lambda L, z: pairs(L, z, nz=2 ** 31 - 1)),
    ('n_pairs = -1 must be >= 0', lambda L, z: pairs(L, z, n_pairs=-1)),
    ('occ4d_pull_pairs_u32: null blocked with n = 30', lambda L, z: pairs(L, z, blocked=None)),
    ('null a / b with n_pairs = 4', lambda L, z: pairs(L, z, a=None)),
    ('null a / b with n_pairs = 4', lambda L, z: pairs(L, z, b=None)),
    ('null hit with n_pairs = 4', lambda L, z: pairs(L, z, hit=None)),
    ('occ4d_pull_paths_i32: nx = 3, ny = -2, nz = -5 must be >= 0', lambda L, z: paths(L, z, ny=-2, nz=-5)),
    ('occ4d_pull_paths_i32: nx = 3, ny = 513, nz = 5 must be <= 512', lambda L, z: paths(L, z, ny=513)),
    ('n_goals = -2 must be >= 0', lambda L, z: paths(L, z, n_goals=-2)),
    ('cap = -1 must be >= 0', lambda L, z: paths(L, z, cap=-1)),
    ('n_goals * cap = 65536 * 65536 exceeds INT32_MAX', lambda L, z: paths(L, z, n_goals=65536, cap=65536)),
    ('occ4d_pull_paths_i32: null blocked with n = 30', lambda L, z: paths(L, z, blocked=None)),
    ('null path_len / waypoint_len with n_goals = 2', lambda L, z: paths(L, z, path_len=None)),
    ('null path_len / waypoint_len with n_goals = 2', lambda L, z: paths(L, z, waypoint_len=None)),
    ('null paths / waypoints with n_goals = 2, cap = 4', lambda L, z: paths(L, z, paths=None)),
    ('null paths / waypoints with n_goals = 2, cap = 4', lambda L, z: paths(L, z, waypoints=None)),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED)


def test_the_symbols_are_in_the_open_table_only():
    lib = pk._lib
    for name in ('occ4d_pull_bits_i32', 'occ4d_pull_pairs_u32', 'occ4d_pull_paths_i32'):
        assert name in lib.ADDON_SIGNATURES
        for pinned in (lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
            assert name not in pinned


def test_accepted_edges_agree(libraries):
    """An empty array, an empty pair list, an empty goal list and an empty grid are no-ops in both, with null pointers; paths and
    waypoints may be null with cap == 0, blocked with an empty grid and pairs to answer; axes of length 1, the longest axis and the
    extreme values of min_clear are accepted."""
    for L, dev in zip(libraries, (DEV, 'cpu')):
        z = zeros_on(dev)
        assert bits(L, z, n=0, clear=None, blocked=None) == pk._lib.OK
        assert bits(L, z, min_clear=-2 ** 31) == pk._lib.OK and bits(L, z, min_clear=2 ** 31 - 1) == pk._lib.OK
        assert pairs(L, z, n_pairs=0, blocked=None, a=None, b=None, hit=None) == pk._lib.OK
        assert pairs(L, z, nx=0, blocked=None) == pk._lib.OK
        assert pairs(L, z, nx=30, ny=1, nz=1) == pk._lib.OK and pairs(L, z, nx=1, ny=1, nz=30) == pk._lib.OK
        assert pairs(L, z, nx=512, ny=1, nz=1, blocked=p(z(16))) == pk._lib.OK
        nothing = dict(blocked=None, paths=None, path_len=None, waypoints=None, waypoint_len=None)
        assert paths(L, z, n_goals=0, **nothing) == pk._lib.OK
        assert paths(L, z, ny=0, **nothing) == pk._lib.OK
        assert paths(L, z, cap=0, paths=None, waypoints=None) == pk._lib.OK
        assert paths(L, z, nx=1, ny=30, nz=1) == pk._lib.OK
    torch.cuda.synchronize()
