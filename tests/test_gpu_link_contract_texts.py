"""The rejected-call table of tests/test_gpu_contract_texts.py for the entry points of include/ext/occ4d_link.h: libocc4d.so and the
g++ twin take the argument contracts from one source (check_overlap / check_match of csrc/link_math.hpp over csrc/contract.hpp).
Both are loaded in one process -- the twin as a second plain handle, never enabled -- and handed the same rejected calls, device
tensors for the one and same-shaped host tensors for the other: the same status and the same occ4d_last_error() bytes."""
import ctypes

import pytest
import torch

import occlusions4d_amd as pk
from contract_texts import float_zeros_on as zeros_on, libraries, p, rejected_test  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EINVAL = pk._lib.EINVAL
I32, I64 = torch.int32, torch.int64


def overlap(L, z, **k):
    """30 points, cap 4: 4 * 64 + 30 + 2 work elements."""
    a = dict(labels_a=p(z(30, dtype=I32)), labels_b=p(z(30, dtype=I32)), k_a=2, k_b=3, n=30, work=p(z(288, dtype=I32)),
             pairs=p(z(4, 4, dtype=I64)), cap=4, totals=p(z(3, dtype=I32)))
    a.update(k)
    return L.occ4d_link_overlap_i32(*a.values(), None)


def match(L, z, **k):
    a = dict(pairs=p(z(4, 4, dtype=I64)), totals=p(z(3, dtype=I32)), cap=4, table_a=p(z(2, 12, dtype=I64)), ld_a=12,
             table_b=p(z(3, 12, dtype=I64)), ld_b=12, k_a=2, k_b=3, track_a=p(z(2, dtype=I32)), iou_num=1, iou_den=2,
             next_in=p(z(1, dtype=I32)), link=p(z(3, 4, dtype=I32)), best_a=p(z(2, 2, dtype=I32)), next_out=p(z(1, dtype=I32)))
    a.update(k)
    return L.occ4d_link_match_i32(*a.values(), None)


def odd_work(L, z):
    return overlap(L, z, work=ctypes.c_void_p(z(290, dtype=I32).data_ptr() + 4))


# (message fragment, call(L, z)): z(*shape, dtype) is a zeros tensor where the library L reads
REJECTED = [
    ('occ4d_link_overlap_i32: n = -1 must be in [0, INT32_MAX]', lambda L, z: overlap(L, z, n=-1)),
    ('occ4d_link_overlap_i32: n = 2147483648 must be in [0, INT32_MAX]', lambda L, z: overlap(L, z, n=2 ** 31)),
    ('n = 1099511627776 must be in [0, INT32_MAX]', lambda L, z: overlap(L, z, n=2 ** 40)),
    ('occ4d_link_overlap_i32: k_a = -1, k_b = 3 must be >= 0', lambda L, z: overlap(L, z, k_a=-1)),
    ('k_a = 2, k_b = -5 must be >= 0', lambda L, z: overlap(L, z, k_b=-5)),
    ('occ4d_link_overlap_i32: cap = -1 must be >= 0', lambda L, z: overlap(L, z, cap=-1)),
    ('null work / totals with n = 30', lambda L, z: overlap(L, z, work=None)),
    ('null work / totals with n = 30', lambda L, z: overlap(L, z, totals=None)),
    ('work must be 8-byte aligned', odd_work),
    ('null labels with n = 30, k_a = 2, k_b = 3', lambda L, z: overlap(L, z, labels_a=None)),
    ('null labels with n = 30, k_a = 2, k_b = 3', lambda L, z: overlap(L, z, labels_b=None)),
    ('null pairs with cap = 4', lambda L, z: overlap(L, z, pairs=None)),
    ('occ4d_link_match_i32: cap = -2 must be >= 0', lambda L, z: match(L, z, cap=-2)),
    ('occ4d_link_match_i32: k_a = -1, k_b = 3 must be >= 0', lambda L, z: match(L, z, k_a=-1)),
    ('k_a = 2, k_b = -1 must be >= 0', lambda L, z: match(L, z, k_b=-1)),
    ('iou_den = 0 must be in [1, 1048576]', lambda L, z: match(L, z, iou_den=0)),
    ('iou_den = -4 must be in [1, 1048576]', lambda L, z: match(L, z, iou_den=-4)),
    ('iou_den = 1048577 must be in [1, 1048576]', lambda L, z: match(L, z, iou_den=2 ** 20 + 1)),
    ('iou_num = -1 must be in [0, iou_den = 2]', lambda L, z: match(L, z, iou_num=-1)),
    ('iou_num = 3 must be in [0, iou_den = 2]', lambda L, z: match(L, z, iou_num=3)),
    ('null pairs / totals with k_a = 2, k_b = 3, cap = 4', lambda L, z: match(L, z, pairs=None)),
    ('null pairs / totals with k_a = 2, k_b = 3, cap = 4', lambda L, z: match(L, z, totals=None)),
    ('null table_a / table_b / track_a with k_a = 2, k_b = 3, cap = 4', lambda L, z: match(L, z, table_a=None)),
    ('null table_a / table_b / track_a with k_a = 2, k_b = 3, cap = 4', lambda L, z: match(L, z, table_b=None)),
    ('null table_a / table_b / track_a with k_a = 2, k_b = 3, cap = 4', lambda L, z: match(L, z, track_a=None)),
    ('ld_a = 0, ld_b = 12 must be >= 1', lambda L, z: match(L, z, ld_a=0)),
    ('ld_a = 12, ld_b = -1 must be >= 1', lambda L, z: match(L, z, ld_b=-1)),
    ('null link with k_b = 3', lambda L, z: match(L, z, link=None)),
    ('null best_a with k_a = 2', lambda L, z: match(L, z, best_a=None)),
    ('null next_in / next_out', lambda L, z: match(L, z, next_in=None)),
    ('null next_in / next_out', lambda L, z: match(L, z, next_out=None, k_a=0, k_b=0)),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED, zeros_on)


def test_accepted_edges_agree(libraries):
    """An empty grid touches no pointer; without components on either side the labels may be null, without rows the pair buffer;
    the match takes null pairs, tables and tracks when there is nothing to read, a threshold of 0, of 1 and of the largest
    denominator, and next_out at next_in's address."""
    for L, dev in zip(libraries, (DEV, 'cpu')):
        z = zeros_on(dev)
        assert overlap(L, z, n=0, labels_a=None, labels_b=None, work=None, pairs=None, totals=None) == pk._lib.OK
        assert overlap(L, z, k_a=0, labels_a=None, labels_b=None) == pk._lib.OK
        assert overlap(L, z, k_b=0, labels_a=None, labels_b=None) == pk._lib.OK
        assert overlap(L, z, cap=0, pairs=None) == pk._lib.OK
        assert overlap(L, z, n=1) == pk._lib.OK and overlap(L, z, k_a=2 ** 31 - 1, k_b=2 ** 31 - 1) == pk._lib.OK
        nothing = dict(pairs=None, totals=None, table_a=None, table_b=None, track_a=None)
        assert match(L, z, k_a=0, best_a=None, **nothing) == pk._lib.OK
        assert match(L, z, k_b=0, link=None, **nothing) == pk._lib.OK
        assert match(L, z, cap=0, **nothing) == pk._lib.OK
        assert match(L, z, k_a=0, k_b=0, link=None, best_a=None, **nothing) == pk._lib.OK
        for num, den in ((0, 1), (1, 1), (0, 2 ** 20), (2 ** 20, 2 ** 20)):
            assert match(L, z, iou_num=num, iou_den=den) == pk._lib.OK
        same = z(1, dtype=I32)
        assert match(L, z, next_in=p(same), next_out=p(same)) == pk._lib.OK
    torch.cuda.synchronize()
