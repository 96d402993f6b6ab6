"""The rejected-call table of tests/test_gpu_contract_texts.py for the entry points of include/occ4d_surface.h: libocc4d.so and the
g++ twin take the two argument contracts from one source (the check_* functions of csrc/surface_math.hpp over csrc/contract.hpp).
Both are loaded in one process -- the twin as a second plain handle, never enabled -- and handed the same rejected calls, device
tensors for the one and same-shaped host tensors for the other: the same status and the same occ4d_last_error() bytes."""
import pytest
import torch

import occlusions4d_amd as pk
from contract_texts import float_zeros_on as zeros_on, libraries, p, rejected_test  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = pk._lib.EINVAL
I32 = torch.int32


def count(L, z, **k):
    """A 4 x 4 x 4 grid: 64 points, one tile."""
    a = dict(density=p(z(64)), ld=1, nx=4, ny=4, nz=4, level=0.5, cell_offsets=p(z(1, dtype=I32)), face_offsets=p(z(1, dtype=I32)),
             totals=p(z(2, dtype=I32)))
    a.update(k)
    return L.occ4d_surface_count_f32(*a.values(), None)


def write(L, z, **k):
    a = dict(density=p(z(64)), ld=1, attrs=p(z(64, 2)), ld_attr=2, n_attr=2, nx=4, ny=4, nz=4, level=0.5, x0=0.0, sx=1.0, y0=0.0,
             sy=1.0, z0=0.0, sz=1.0, cell_offsets=p(z(1, dtype=I32)), face_offsets=p(z(1, dtype=I32)), work=p(z(64, dtype=I32)),
             vertices=p(z(27, 5)), ld_v=5, vertex_cap=27, faces=p(z(36, 4, dtype=I32)), face_cap=36)
    a.update(k)
    return L.occ4d_surface_write_f32(*a.values(), None)


# (message fragment, call(L, z)): z(*shape, dtype) is a zeros tensor where the library L reads
REJECTED = [
    ('occ4d_surface_count_f32: nx = -1, ny = 4, nz = 4 must be >= 0', lambda L, z: count(L, z, nx=-1)),
    ('nx = 4, ny = 4, nz = -4', lambda L, z: count(L, z, nz=-4)),
    ('occ4d_surface_count_f32: 3 * nx * ny * nz = 3 * 1024 * 1024 * 1024 exceeds INT32_MAX', lambda L, z: count(L, z, nx=1024, ny=1024, nz=1024)),
    ('exceeds INT32_MAX', lambda L, z: count(L, z, nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1)),
    ('exceeds INT32_MAX', lambda L, z: count(L, z, nx=895, ny=895, nz=895)),
    ('occ4d_surface_count_f32: ld = 0 must be >= 1', lambda L, z: count(L, z, ld=0)),
    ('null density / cell_offsets / face_offsets / totals', lambda L, z: count(L, z, density=None)),
    ('null density / cell_offsets / face_offsets / totals', lambda L, z: count(L, z, cell_offsets=None)),
    ('null density / cell_offsets / face_offsets / totals', lambda L, z: count(L, z, face_offsets=None)),
    ('null density / cell_offsets / face_offsets / totals', lambda L, z: count(L, z, totals=None)),
    ('occ4d_surface_write_f32: nx = 4, ny = -1, nz = 4', lambda L, z: write(L, z, ny=-1)),
    ('occ4d_surface_write_f32: 3 * nx * ny * nz', lambda L, z: write(L, z, nx=1024, ny=1024, nz=1024)),
    ('occ4d_surface_write_f32: ld = -1 must be >= 1', lambda L, z: write(L, z, ld=-1)),
    ('n_attr = 33: need 0 <= n_attr <= 32', lambda L, z: write(L, z, n_attr=33, ld_attr=33, ld_v=36)),
    ('n_attr = -1: need 0 <= n_attr <= 32', lambda L, z: write(L, z, n_attr=-1)),
    ('ld_attr = 1 must be >= n_attr = 2 and ld_v = 5 >= 3 + n_attr', lambda L, z: write(L, z, ld_attr=1)),
    ('ld_attr = 2 must be >= n_attr = 2 and ld_v = 4 >= 3 + n_attr', lambda L, z: write(L, z, ld_v=4)),
    ('vertex_cap = -1, face_cap = 36 must be >= 0', lambda L, z: write(L, z, vertex_cap=-1)),
    ('vertex_cap = 27, face_cap = -2 must be >= 0', lambda L, z: write(L, z, face_cap=-2)),
    ('null density / cell_offsets / face_offsets / work', lambda L, z: write(L, z, density=None)),
    ('null density / cell_offsets / face_offsets / work', lambda L, z: write(L, z, cell_offsets=None)),
    ('null density / cell_offsets / face_offsets / work', lambda L, z: write(L, z, face_offsets=None)),
    ('null density / cell_offsets / face_offsets / work', lambda L, z: write(L, z, work=None)),
    ('null attrs with n_attr = 2', lambda L, z: write(L, z, attrs=None)),
    ('null vertices / faces with vertex_cap = 27, face_cap = 36', lambda L, z: write(L, z, vertices=None)),
    ('null vertices / faces with vertex_cap = 27, face_cap = 36', lambda L, z: write(L, z, faces=None)),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED, zeros_on)


def test_accepted_edges_agree(libraries):
    """An empty grid is a no-op in both, with null pointers; no attributes take a null attrs; a capacity of 0 a null array; the
    largest accepted grid size is accepted as a size (an axis of 0 beside it: nothing runs)."""
    for L, dev in zip(libraries, (DEV, 'cpu')):
        z = zeros_on(dev)
        assert count(L, z, nx=0, density=None, cell_offsets=None, face_offsets=None, totals=None) == pk._lib.OK
        assert write(L, z, nz=0, density=None, attrs=None, cell_offsets=None, face_offsets=None, work=None, vertices=None,
                     faces=None) == pk._lib.OK
        assert write(L, z, attrs=None, n_attr=0, ld_attr=0, ld_v=3) == pk._lib.OK
        assert write(L, z, vertices=None, vertex_cap=0, faces=None, face_cap=0) == pk._lib.OK
        assert count(L, z, nx=2 ** 31 - 1, ny=0, nz=2 ** 31 - 1, density=None, cell_offsets=None, face_offsets=None, totals=None) == pk._lib.OK
    torch.cuda.synchronize()
