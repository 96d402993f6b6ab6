"""The rejected-call table of tests/test_gpu_contract_texts.py for the entry points of include/ext/occ4d_watershed.h: libocc4d.so and
the g++ twin take the argument contracts from one source (check_label / check_peaks of csrc/watershed_math.hpp over
csrc/contract.hpp).  Both are loaded in one process -- the twin as a second plain handle, never enabled -- and handed the same
rejected calls, device tensors for the one and same-shaped host tensors for the other: the same status and the same
occ4d_last_error() bytes."""
import ctypes

import pytest
import torch

import occlusions4d_amd as pk
from contract_texts import libraries, p, rejected_test, zeros_on  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = pk._lib.EINVAL
WORK = 4 * 30 + 4 + 12                 # ops.watershed_work_len(30)


def label(L, z, **k):
    """A 3 x 2 x 5 grid (30 points)."""
    a = dict(height=p(z(30)), nx=3, ny=2, nz=5, connectivity=26, h=0, min_size=1, work=p(z(WORK)), labels=p(z(30)), totals=p(z(4)))
    a.update(k)
    return L.occ4d_watershed_label_i32(*a.values(), None)


def peaks(L, z, **k):
    a = dict(height=p(z(30)), labels=p(z(30)), n=30, totals=p(z(4)), peaks=p(z(4, 2)), cap=4)
    a.update(k)
    return L.occ4d_watershed_peaks_i32(*a.values(), None)


# (message fragment, call(L, z)): z(*shape) is an int32 zeros tensor where the library L reads
REJECTED = [
    ('occ4d_watershed_label_i32: nx = -1, ny = 2, nz = 5 must be >= 0', lambda L, z: label(L, z, nx=-1)),
    ('nx = 3, ny = -2, nz = -5 must be >= 0', lambda L, z: label(L, z, ny=-2, nz=-5)),
    ('nx * ny * nz = 65536 * 65536 * 1 exceeds INT32_MAX', lambda L, z: label(L, z, nx=65536, ny=65536, nz=1)),
    ('nx * ny * nz = 2048 * 1024 * 1024 exceeds INT32_MAX', lambda L, z: label(L, z, nx=2048, ny=1024, nz=1024)),
    ('connectivity = 8 must be 6, 18 or 26', lambda L, z: label(L, z, connectivity=8)),
    ('connectivity = 0 must be 6, 18 or 26', lambda L, z: label(L, z, connectivity=0)),
    ('h = -1 must be >= 0', lambda L, z: label(L, z, h=-1)),
    ('h = -2147483648 must be >= 0', lambda L, z: label(L, z, h=-2 ** 31)),
    ('min_size = 0 must be >= 1', lambda L, z: label(L, z, min_size=0)),
    ('min_size = -3 must be >= 1', lambda L, z: label(L, z, min_size=-3)),
    ('null height with n = 30', lambda L, z: label(L, z, height=None)),
    ('null work / labels / totals with n = 30', lambda L, z: label(L, z, work=None)),
    ('null work / labels / totals with n = 30', lambda L, z: label(L, z, labels=None)),
    ('null work / labels / totals with n = 30', lambda L, z: label(L, z, totals=None)),
    ('occ4d_watershed_peaks_i32: n = -1 must be >= 0', lambda L, z: peaks(L, z, n=-1)),
    ('cap = -1 must be >= 0', lambda L, z: peaks(L, z, cap=-1)),
    ('null height / labels / totals / peaks with n = 30, cap = 4', lambda L, z: peaks(L, z, height=None)),
    ('null height / labels / totals / peaks with n = 30, cap = 4', lambda L, z: peaks(L, z, labels=None)),
    ('null height / labels / totals / peaks with n = 30, cap = 4', lambda L, z: peaks(L, z, totals=None)),
    ('null height / labels / totals / peaks with n = 30, cap = 4', lambda L, z: peaks(L, z, peaks=None)),
    ('peaks must be aligned to 8 bytes', lambda L, z: peaks(L, z, peaks=ctypes.c_void_p(z(5, 2).data_ptr() + 4))),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED)


def test_accepted_edges_agree(libraries):
    """An empty grid and cap = 0 are no-ops in both, with null pointers; axes of length 1, the last legal h and min_size and every
    connectivity are accepted."""
    assert WORK == pk.ops.watershed_work_len(30)
    for L, dev in zip(libraries, (DEV, 'cpu')):
        z = zeros_on(dev)
        nothing = dict(height=None, work=None, labels=None, totals=None)
        assert label(L, z, nx=0, **nothing) == pk._lib.OK
        assert label(L, z, ny=0, nz=0, **nothing) == pk._lib.OK
        assert peaks(L, z, n=0, height=None, labels=None, totals=None, peaks=None) == pk._lib.OK
        assert peaks(L, z, cap=0, height=None, labels=None, totals=None, peaks=None) == pk._lib.OK
        assert label(L, z, nx=30, ny=1, nz=1) == pk._lib.OK and label(L, z, nx=1, ny=1, nz=30) == pk._lib.OK
        assert label(L, z, nx=1, ny=30, nz=1, connectivity=6) == pk._lib.OK and label(L, z, connectivity=18) == pk._lib.OK
        assert label(L, z, h=2 ** 31 - 1) == pk._lib.OK and label(L, z, min_size=2 ** 31 - 1) == pk._lib.OK
        assert peaks(L, z) == pk._lib.OK
    torch.cuda.synchronize()
