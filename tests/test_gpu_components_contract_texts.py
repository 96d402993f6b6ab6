"""The rejected-call table of tests/test_gpu_contract_texts.py for the entry points of include/ext/occ4d_components.h: libocc4d.so and
the g++ twin take the argument contracts from one source (check_label / check_table of csrc/components_math.hpp over
csrc/contract.hpp).  Both are loaded in one process -- the twin as a second plain handle, never enabled -- and handed the same
rejected calls, device tensors for the one and same-shaped host tensors for the other: the same status and the same
occ4d_last_error() bytes."""
import pytest
import torch

import occlusions4d_amd as pk
from contract_texts import float_zeros_on as zeros_on, libraries, p, rejected_test  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = pk._lib.EINVAL
I32, I64 = torch.int32, torch.int64
NAN = float('nan')


def label(L, z, **k):
    """A 3 x 2 x 5 grid (30 points): 90 + 3 work elements."""
    a = dict(field=p(z(30)), ld=1, level=0.5, mask=p(z(30)), ld_mask=1, mask_level=0.5, klass=p(z(30, dtype=I32)), nx=3, ny=2, nz=5,
             connectivity=6, min_size=1, work=p(z(93, dtype=I32)), labels=p(z(30, dtype=I32)), totals=p(z(3, dtype=I32)))
    a.update(k)
    return L.occ4d_components_label_f32(*a.values(), None)


def table(L, z, **k):
    a = dict(labels=p(z(30, dtype=I32) - 1), klass=p(z(30, dtype=I32)), nx=3, ny=2, nz=5, totals=p(z(3, dtype=I32)),
             table=p(z(4, 12, dtype=I64)), cap=4)
    a.update(k)
    return L.occ4d_components_table_i64(*a.values(), None)


# (message fragment, call(L, z)): z(*shape, dtype) is a zeros tensor where the library L reads
REJECTED = [
    ('occ4d_components_label_f32: nx = -1, ny = 2, nz = 5 must be >= 0', lambda L, z: label(L, z, nx=-1)),
    ('nx = 3, ny = 2, nz = -5 must be >= 0', lambda L, z: label(L, z, nz=-5)),
    ('occ4d_components_label_f32: nx * ny * nz = 2048 * 1024 * 1024 exceeds INT32_MAX', lambda L, z: label(L, z, nx=2048, ny=1024, nz=1024)),
    ('exceeds INT32_MAX', lambda L, z: label(L, z, nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1)),
    ('connectivity = 0 must be 6, 18 or 26', lambda L, z: label(L, z, connectivity=0)),
    ('connectivity = 8 must be 6, 18 or 26', lambda L, z: label(L, z, connectivity=8)),
    ('connectivity = 27 must be 6, 18 or 26', lambda L, z: label(L, z, connectivity=27)),
    ('min_size = 0 must be >= 1', lambda L, z: label(L, z, min_size=0)),
    ('min_size = -3 must be >= 1', lambda L, z: label(L, z, min_size=-3)),
    ('occ4d_components_label_f32: ld = 0 must be >= 1', lambda L, z: label(L, z, ld=0)),
    ('ld_mask = 0 must be >= 1', lambda L, z: label(L, z, ld_mask=0)),
    ('ld_mask = -2 must be >= 1', lambda L, z: label(L, z, ld_mask=-2)),
    ('null field with n = 30', lambda L, z: label(L, z, field=None)),
    ('null work / labels / totals with n = 30', lambda L, z: label(L, z, work=None)),
    ('null work / labels / totals with n = 30', lambda L, z: label(L, z, labels=None)),
    ('null work / labels / totals with n = 30', lambda L, z: label(L, z, totals=None)),
    ('occ4d_components_table_i64: nx = 3, ny = -2, nz = 5 must be >= 0', lambda L, z: table(L, z, ny=-2)),
    ('occ4d_components_table_i64: nx * ny * nz = 2048 * 1024 * 1024 exceeds INT32_MAX', lambda L, z: table(L, z, nx=2048, ny=1024, nz=1024)),
    ('cap = -1 must be >= 0', lambda L, z: table(L, z, cap=-1)),
    ('null labels / totals / table with n = 30, cap = 4', lambda L, z: table(L, z, labels=None)),
    ('null labels / totals / table with n = 30, cap = 4', lambda L, z: table(L, z, totals=None)),
    ('null labels / totals / table with n = 30, cap = 4', lambda L, z: table(L, z, table=None)),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED, zeros_on)


def test_accepted_edges_agree(libraries):
    """An empty grid and an empty table are no-ops in both, with null pointers; the mask and the classes may be null; an axis of
    length 1, a NaN level and every connectivity are accepted."""
    for L, dev in zip(libraries, (DEV, 'cpu')):
        z = zeros_on(dev)
        nothing = dict(field=None, mask=None, klass=None, work=None, labels=None, totals=None)
        assert label(L, z, nx=0, **nothing) == pk._lib.OK
        assert label(L, z, ny=0, nz=0, **nothing) == pk._lib.OK
        assert table(L, z, nz=0, labels=None, klass=None, totals=None, table=None) == pk._lib.OK
        assert table(L, z, cap=0, labels=None, klass=None, totals=None, table=None) == pk._lib.OK
        assert label(L, z, mask=None, ld_mask=0, klass=None) == pk._lib.OK
        assert label(L, z, nx=30, ny=1, nz=1) == pk._lib.OK and label(L, z, nx=1, ny=1, nz=30) == pk._lib.OK
        assert label(L, z, level=NAN, mask_level=NAN) == pk._lib.OK
        for connectivity in (6, 18, 26):
            assert label(L, z, connectivity=connectivity, min_size=2 ** 31 - 1) == pk._lib.OK
        assert table(L, z, klass=None) == pk._lib.OK
    torch.cuda.synchronize()
