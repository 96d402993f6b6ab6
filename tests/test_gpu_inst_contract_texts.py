"""The rejected-call table of tests/test_gpu_contract_texts.py for the entry points of include/occ4d_inst.h: libocc4d.so and the
g++ twin take the three argument contracts from one source (the check_* functions of csrc/inst_math.hpp over csrc/contract.hpp).
Both are loaded in one process -- the twin as a second plain handle, never enabled -- and handed the same rejected calls, device
tensors for the one and same-shaped host tensors for the other: the same status and the same occ4d_last_error() bytes."""
import pytest
import torch

import occlusions4d_amd as pk
from contract_texts import float_zeros_on as zeros_on, libraries, p, rejected_test  # noqa: F401

pytestmark = pytest.mark.gpu
EINVAL = pk._lib.EINVAL
I32, I64, F64 = torch.int32, torch.int64, torch.float64
FRAME = 1 + 9 + 16                    # occ4d_inst_frame_len(2)


def confusion(L, z, **k):
    a = dict(density=p(z(4)), ld_density=1, pred_id=p(z(4)), ld_pred=1, n=4, nn_idx=p(z(4, dtype=I32)), nn_dist=p(z(4)), target_id=p(z(3)),
             ld_target=1, m=3, n_ids=2, threshold=0.5, radius=0.2, frame=p(z(FRAME, dtype=I64)))
    a.update(k)
    return L.occ4d_inst_confusion_f32(*a.values(), None)


def points(L, z, **k):
    a = dict(rows=p(z(4, 3)), ld=3, n=4, id=p(z(4)), ld_id=1, n_ids=2, side=0, frame=p(z(FRAME, dtype=I64)))
    a.update(k)
    return L.occ4d_inst_points_f32(*a.values(), None)


def fold(L, z, **k):
    a = dict(frame=p(z(FRAME, dtype=I64)), n_ids=2, inst_group=None, n_groups=1, counts=p(z(9, dtype=I64)), sums=p(z(4, dtype=F64)))
    a.update(k)
    return L.occ4d_inst_fold(*a.values(), None)


# (message fragment, call(L, z)): z(*shape, dtype) is a zeros tensor where the library L reads
REJECTED = [
    ('occ4d_inst_confusion_f32: n_ids = 0 must be in 1 .. 64', lambda L, z: confusion(L, z, n_ids=0)),
    ('occ4d_inst_confusion_f32: n_ids = 65 must be in 1 .. 64', lambda L, z: confusion(L, z, n_ids=65)),
    ('occ4d_inst_confusion_f32: n = -1', lambda L, z: confusion(L, z, n=-1)),
    ('ld_density = 0', lambda L, z: confusion(L, z, ld_density=0)),
    ('ld_pred = 0', lambda L, z: confusion(L, z, ld_pred=0)),
    ('ld_target = -1', lambda L, z: confusion(L, z, ld_target=-1)),
    ('occ4d_inst_confusion_f32: null frame', lambda L, z: confusion(L, z, frame=None)),
    ('null density / pred_id / nn_idx / nn_dist / target_id', lambda L, z: confusion(L, z, density=None)),
    ('null density / pred_id / nn_idx / nn_dist / target_id', lambda L, z: confusion(L, z, nn_idx=None)),
    ('null density / pred_id / nn_idx / nn_dist / target_id', lambda L, z: confusion(L, z, target_id=None)),
    ('occ4d_inst_points_f32: n_ids = 0', lambda L, z: points(L, z, n_ids=0)),
    ('occ4d_inst_points_f32: n_ids = 65', lambda L, z: points(L, z, n_ids=65)),
    ('occ4d_inst_points_f32: n = -1', lambda L, z: points(L, z, n=-1)),
    ('ld = 2 must be >= 3', lambda L, z: points(L, z, ld=2)),
    ('ld_id = 0', lambda L, z: points(L, z, ld_id=0)),
    ('side = 2', lambda L, z: points(L, z, side=2)),
    ('occ4d_inst_points_f32: null frame', lambda L, z: points(L, z, frame=None)),
    ('null rows / id', lambda L, z: points(L, z, rows=None)),
    ('null rows / id', lambda L, z: points(L, z, id=None)),
    ('occ4d_inst_fold: n_ids = 0', lambda L, z: fold(L, z, n_ids=0)),
    ('occ4d_inst_fold: n_ids = 65', lambda L, z: fold(L, z, n_ids=65)),
    ('n_groups = 9 must be in 1 .. 8', lambda L, z: fold(L, z, n_groups=9)),
    ('n_groups = 0', lambda L, z: fold(L, z, n_groups=0)),
    ('null frame / counts / sums', lambda L, z: fold(L, z, frame=None)),
    ('null frame / counts / sums', lambda L, z: fold(L, z, counts=None)),
    ('null frame / counts / sums', lambda L, z: fold(L, z, sums=None)),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED, zeros_on)


def test_the_length_helpers_agree(libraries):
    hip, twin = libraries
    for L in (hip, twin):
        assert [L.occ4d_inst_frame_len(k) for k in (0, 1, 2, 64, 65)] == [-1, 13, FRAME, 1 + 65 * 65 + 512, -1]
        assert [L.occ4d_inst_counts_len(k) for k in (0, 1, 8, 9)] == [-1, 9, 65, -1]
        assert [L.occ4d_inst_sums_len(k) for k in (0, 1, 8, 9)] == [-1, 4, 32, -1]
