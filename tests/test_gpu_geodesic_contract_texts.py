"""The rejected-call table of tests/test_gpu_contract_texts.py for the entry points of include/ext/occ4d_geodesic.h: libocc4d.so and
the g++ twin take the argument contracts from one source (check_geodesic / check_trace of csrc/geodesic_math.hpp over
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


def grid(L, z, **k):
    """A 3 x 2 x 5 grid (30 points), one seed, four rounds."""
    a = dict(clear=p(z(30)), min_clear=0, nx=3, ny=2, nz=5, seeds=p(z(1)), n_seeds=1, connectivity=26, step_face=3, step_edge=4, step_corner=5,
             rounds=4, resume=0, work=p(z(5)), cost=p(z(30)), parent=p(z(30)), status=p(z(2)))
    a.update(k)
    return L.occ4d_geodesic_grid_i32(*a.values(), None)


def line(L, z, **k):
    """A 3 x 1 x 1 grid: the longest path is 2 * the largest step."""
    return grid(L, z, **dict(dict(clear=p(z(3)), nx=3, ny=1, nz=1, cost=p(z(3)), parent=None), **k))


def trace(L, z, **k):
    a = dict(cost=p(z(30)), parent=p(z(30)), n=30, goals=p(z(2)), n_goals=2, cap=4, paths=p(z(8)), path_len=p(z(2)))
    a.update(k)
    return L.occ4d_geodesic_trace_i32(*a.values(), None)


# (message fragment, call(L, z)): z(*shape) is an int32 zeros tensor where the library L reads
REJECTED = [
    ('occ4d_geodesic_grid_i32: nx = -1, ny = 2, nz = 5 must be >= 0', lambda L, z: grid(L, z, nx=-1)),
    ('nx = 3, ny = -2, nz = -5 must be >= 0', lambda L, z: grid(L, z, ny=-2, nz=-5)),
    ('nx = 513, ny = 2, nz = 5 must be <= 512', lambda L, z: grid(L, z, nx=513)),
    ('nx = 3, ny = 2, nz = 2147483647 must be <= 512', lambda L, z: grid(L, z, nz=2 ** 31 - 1)),
    ('connectivity = 8 must be 6, 18 or 26', lambda L, z: grid(L, z, connectivity=8)),
    ('connectivity = 0 must be 6, 18 or 26', lambda L, z: grid(L, z, connectivity=0)),
    ('step_face = 0, step_edge = 4, step_corner = 5 must be >= 1', lambda L, z: grid(L, z, step_face=0)),
    ('step_face = 3, step_edge = 4, step_corner = -5 must be >= 1', lambda L, z: grid(L, z, step_corner=-5)),
    ('the longest path 2147483648 = (3 - 1) * 1073741824 exceeds INT32_MAX - 1', lambda L, z: line(L, z, step_face=1073741824)),
    ('the longest path 2147483648 = (3 - 1) * 1073741824 exceeds INT32_MAX - 1', lambda L, z: line(L, z, connectivity=6, step_corner=1073741824)),
    ('the longest path 2147483669 = (30 - 1) * 74051161 exceeds', lambda L, z: grid(L, z, step_edge=74051161)),
    ('n_seeds = -1 must be >= 0', lambda L, z: grid(L, z, n_seeds=-1)),
    ('rounds = -1 must be in [0, 65536]', lambda L, z: grid(L, z, rounds=-1)),
    ('rounds = 65537 must be in [0, 65536]', lambda L, z: grid(L, z, rounds=65537)),
    ('resume = 2 must be 0 or 1', lambda L, z: grid(L, z, resume=2)),
    ('null clear with n = 30', lambda L, z: grid(L, z, clear=None)),
    ('null seeds with n_seeds = 1', lambda L, z: grid(L, z, seeds=None)),
    ('null work / cost / status with n = 30', lambda L, z: grid(L, z, work=None)),
    ('null work / cost / status with n = 30', lambda L, z: grid(L, z, cost=None)),
    ('null work / cost / status with n = 30', lambda L, z: grid(L, z, status=None)),
    ('occ4d_geodesic_trace_i32: n = -1 must be >= 0', lambda L, z: trace(L, z, n=-1)),
    ('n_goals = -2 must be >= 0', lambda L, z: trace(L, z, n_goals=-2)),
    ('cap = -1 must be >= 0', lambda L, z: trace(L, z, cap=-1)),
    ('n_goals * cap = 65536 * 65536 exceeds INT32_MAX', lambda L, z: trace(L, z, n_goals=65536, cap=65536)),
    ('null goals with n_goals = 2', lambda L, z: trace(L, z, goals=None)),
    ('null cost / parent with n = 30', lambda L, z: trace(L, z, parent=None)),
    ('null path_len with n_goals = 2', lambda L, z: trace(L, z, path_len=None)),
    ('null paths with n_goals = 2, cap = 4', lambda L, z: trace(L, z, paths=None)),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED)


def test_accepted_edges_agree(libraries):
    """An empty grid and an empty goal list are no-ops in both, with null pointers; seeds, parent and paths may be null where nothing
    is made of them; axes of length 1, no rounds, a negative min_clear and the last legal step are accepted."""
    for L, dev in zip(libraries, (DEV, 'cpu')):
        z = zeros_on(dev)
        nothing = dict(clear=None, seeds=None, work=None, cost=None, parent=None, status=None)
        assert grid(L, z, nx=0, **nothing) == pk._lib.OK
        assert grid(L, z, ny=0, nz=0, **nothing) == pk._lib.OK
        assert grid(L, z, seeds=None, n_seeds=0) == pk._lib.OK
        assert grid(L, z, seeds=None, resume=1) == pk._lib.OK
        assert grid(L, z, parent=None) == pk._lib.OK
        assert grid(L, z, rounds=0, work=p(z(1))) == pk._lib.OK
        assert grid(L, z, min_clear=-2 ** 31, connectivity=6) == pk._lib.OK and grid(L, z, connectivity=18) == pk._lib.OK
        assert grid(L, z, nx=30, ny=1, nz=1) == pk._lib.OK and grid(L, z, nx=1, ny=1, nz=30) == pk._lib.OK
        assert line(L, z, step_face=1073741823, step_edge=1073741823) == pk._lib.OK and grid(L, z, step_corner=74051160) == pk._lib.OK
        assert trace(L, z, n_goals=0, goals=None, paths=None, path_len=None) == pk._lib.OK
        assert trace(L, z, cap=0, paths=None) == pk._lib.OK
        assert trace(L, z, n=0, cost=None, parent=None) == pk._lib.OK
    torch.cuda.synchronize()
