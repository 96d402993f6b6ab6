"""The rejected-call table of tests/test_gpu_contract_texts.py for the entry points of include/occ4d_refine.h: libocc4d.so and the
g++ twin take the two argument contracts from one source (the check_* functions of csrc/refine_math.hpp over csrc/contract.hpp).
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


def mark(L, z, **k):
    """A 4 x 4 x 4 grid in blocks of 2: 8 blocks, 64 points."""
    a = dict(rep_density=p(z(8)), ld_rep=1, nx=4, ny=4, nz=4, b=2, dilate=1, op=1, low=0.5, active=p(z(8, dtype=I32)), key=p(z(64)))
    a.update(k)
    return L.occ4d_refine_mark_f32(*a.values(), None)


def expand(L, z, **k):
    a = dict(key=p(z(64)), block_offsets=p(z(1, dtype=I32)), rep_out=p(z(8, 5)), ld_rep=5, fine_out=p(z(56, 5)), ld_fine=5, n_fine=56,
             nx=4, ny=4, nz=4, b=2, g=5, out=p(z(64, 5)), ld_out=5)
    a.update(k)
    return L.occ4d_refine_expand_f32(*a.values(), None)


# (message fragment, call(L, z)): z(*shape, dtype) is a zeros tensor where the library L reads
REJECTED = [
    ('occ4d_refine_mark_f32: b = 1 must be in 2 .. 8', lambda L, z: mark(L, z, b=1)),
    ('occ4d_refine_mark_f32: b = 9 must be in 2 .. 8', lambda L, z: mark(L, z, b=9)),
    ('dilate = 3 must be in 0 .. 2', lambda L, z: mark(L, z, dilate=3)),
    ('dilate = -1', lambda L, z: mark(L, z, dilate=-1)),
    ('occ4d_refine_mark_f32: op code 3', lambda L, z: mark(L, z, op=3)),
    ('op code -1', lambda L, z: mark(L, z, op=-1)),
    ('occ4d_refine_mark_f32: nx = -1, ny = 4, nz = 4 must be >= 0', lambda L, z: mark(L, z, nx=-1)),
    ('nx = 4, ny = 4, nz = -4', lambda L, z: mark(L, z, nz=-4)),
    ('exceeds INT32_MAX', lambda L, z: mark(L, z, nx=2048, ny=2048, nz=512)),
    ('exceeds INT32_MAX', lambda L, z: mark(L, z, nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1)),
    ('ld_rep = 0 must be >= 1', lambda L, z: mark(L, z, ld_rep=0)),
    ('null rep_density / active / key', lambda L, z: mark(L, z, rep_density=None)),
    ('null rep_density / active / key', lambda L, z: mark(L, z, active=None)),
    ('null rep_density / active / key', lambda L, z: mark(L, z, key=None)),
    ('occ4d_refine_expand_f32: b = 1', lambda L, z: expand(L, z, b=1)),
    ('occ4d_refine_expand_f32: b = 9', lambda L, z: expand(L, z, b=9)),
    ('occ4d_refine_expand_f32: nx = 4, ny = -1, nz = 4', lambda L, z: expand(L, z, ny=-1)),
    ('g = 0: need 1 <= g <= 32', lambda L, z: expand(L, z, g=0)),
    ('g = 33: need 1 <= g <= 32', lambda L, z: expand(L, z, g=33, ld_rep=33, ld_fine=33, ld_out=33)),
    ('n_fine = -1', lambda L, z: expand(L, z, n_fine=-1)),
    ('ld_rep = 4, ld_fine = 5, ld_out = 5 must be >= g = 5', lambda L, z: expand(L, z, ld_rep=4)),
    ('ld_rep = 5, ld_fine = 4, ld_out = 5 must be >= g = 5', lambda L, z: expand(L, z, ld_fine=4)),
    ('ld_rep = 5, ld_fine = 5, ld_out = 4 must be >= g = 5', lambda L, z: expand(L, z, ld_out=4)),
    ('null key / block_offsets / rep_out / out', lambda L, z: expand(L, z, key=None)),
    ('null key / block_offsets / rep_out / out', lambda L, z: expand(L, z, block_offsets=None)),
    ('null key / block_offsets / rep_out / out', lambda L, z: expand(L, z, rep_out=None)),
    ('null key / block_offsets / rep_out / out', lambda L, z: expand(L, z, out=None)),
    ('null fine_out with n_fine = 56', lambda L, z: expand(L, z, fine_out=None)),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED, zeros_on)


def test_accepted_edges_agree(libraries):
    """An empty grid is a no-op in both, with null pointers; n_fine = 0 takes a null fine_out."""
    for L, dev in zip(libraries, (DEV, 'cpu')):
        z = zeros_on(dev)
        assert mark(L, z, nx=0, rep_density=None, active=None, key=None) == pk._lib.OK
        assert expand(L, z, nz=0, key=None, block_offsets=None, rep_out=None, fine_out=None, out=None) == pk._lib.OK
        assert expand(L, z, n_fine=0, fine_out=None) == pk._lib.OK
    torch.cuda.synchronize()
