"""The rejected-call table of tests/contract_texts.py for the entry point of include/ext/occ4d_sweep.h: libocc4d.so and the g++ twin
take the argument contract from one source (check_sweep of csrc/sweep_math.hpp over csrc/contract.hpp).  Both are loaded in one
process -- the twin as a second plain handle, never enabled -- and handed the same rejected calls, device tensors for the one and
same-shaped host tensors for the other: the same status and the same occ4d_last_error() bytes."""
import ctypes

import pytest
import torch

import occlusions4d_amd as pk
from contract_texts import float_zeros_on as zeros_on, libraries, p, rejected_test  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
I32 = torch.int32
NAN, INF = float('nan'), float('inf')


def cols(*c):
    return (ctypes.c_int32 * len(c))(*c)


def sweep(L, z, **k):
    """A 3 x 2 x 5 grid (30 points), two views of 2 x 6 rays that share one table, two of four attribute columns, two classes."""
    a = dict(field=p(z(30)), ld=1, nx=3, ny=2, nz=5, x0=0.0, sx=1.0, y0=0.0, sy=1.0, z0=0.0, sz=1.0, level=0.5, pose=p(z(2, 12)),
             dirs=p(z(24, 3)), V=2, B=2, A=6, per_view=0, near=0.5, step=0.25, n_steps=8, attrs=p(z(30, 4)), ld_attr=4, d=4,
             cols_host=cols(0, 2), C=2, sem_first=2, n_sem=2, labels=p(z(30, dtype=I32)), K=3, range_background=-1.0, feat_background=0.0,
             range=p(z(2, 12)), point=p(z(2, 12, 3)), cell=p(z(2, 12, dtype=I32)), owner=p(z(2, 12, dtype=I32)), cosine=p(z(2, 12)),
             sem=p(z(2, 12, dtype=I32)), inst=p(z(2, 12, dtype=I32)), feat=p(z(2, 12, 2)))
    a.update(k)
    return L.occ4d_sweep_rays_f32(*a.values(), None)


# (message fragment, call(L, z)): z(*shape, dtype) is a zeros tensor where the library L reads
REJECTED = [
    ('occ4d_sweep_rays_f32: nx = 1, ny = 2, nz = 5 must be >= 2', lambda L, z: sweep(L, z, nx=1)),
    ('nx = 3, ny = 0, nz = 5 must be >= 2', lambda L, z: sweep(L, z, ny=0)),
    ('nx = 3, ny = 2, nz = -5 must be >= 2', lambda L, z: sweep(L, z, nz=-5)),
    ('nx * ny * nz = 2048 * 1024 * 1024 exceeds INT32_MAX', lambda L, z: sweep(L, z, nx=2048, ny=1024, nz=1024)),
    ('exceeds INT32_MAX', lambda L, z: sweep(L, z, nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1)),
    ('ld = 0 must be >= 1', lambda L, z: sweep(L, z, ld=0)),
    ('V = -1, B = 2, A = 6 must be >= 0', lambda L, z: sweep(L, z, V=-1)),
    ('V = 2, B = -2, A = 6 must be >= 0', lambda L, z: sweep(L, z, B=-2)),
    ('V = 2, B = 2, A = -1 must be >= 0', lambda L, z: sweep(L, z, A=-1)),
    ('V R = 2 * 32768 * 32768 must be < 2^31', lambda L, z: sweep(L, z, B=32768, A=32768)),
    ('V R = 1 * 65536 * 32768 must be < 2^31', lambda L, z: sweep(L, z, V=1, B=65536, A=32768)),
    ('V R = 2 * 2147483647 * 2147483647 must be < 2^31', lambda L, z: sweep(L, z, B=2 ** 31 - 1, A=2 ** 31 - 1)),
    ('per_view = 2 must be 0 or 1', lambda L, z: sweep(L, z, per_view=2)),
    ('per_view = -1 must be 0 or 1', lambda L, z: sweep(L, z, per_view=-1)),
    ('step = 0 must be finite and > 0', lambda L, z: sweep(L, z, step=0.0)),
    ('step = -0.25 must be finite and > 0', lambda L, z: sweep(L, z, step=-0.25)),
    ('step = nan must be finite and > 0', lambda L, z: sweep(L, z, step=NAN)),
    ('step = inf must be finite and > 0', lambda L, z: sweep(L, z, step=INF)),
    ('near = nan must be finite', lambda L, z: sweep(L, z, near=NAN)),
    ('near = -inf must be finite', lambda L, z: sweep(L, z, near=-INF)),
    ('n_steps = 0 must be in 1 .. 65536', lambda L, z: sweep(L, z, n_steps=0)),
    ('n_steps = 65537 must be in 1 .. 65536', lambda L, z: sweep(L, z, n_steps=65537)),
    ('C = 33 must be in 0 .. 32', lambda L, z: sweep(L, z, C=33)),
    ('C = -1 must be in 0 .. 32', lambda L, z: sweep(L, z, C=-1)),
    ('n_sem = -1 must be >= 0', lambda L, z: sweep(L, z, n_sem=-1)),
    ('K = -1 must be >= 0', lambda L, z: sweep(L, z, K=-1)),
    ('null cols_host with C = 2', lambda L, z: sweep(L, z, cols_host=None)),
    ('column 4 must be in 0 .. d - 1 = 3', lambda L, z: sweep(L, z, cols_host=cols(0, 4))),
    ('column -1 must be in 0 .. d - 1 = 3', lambda L, z: sweep(L, z, cols_host=cols(-1, 0))),
    ('d = 4, ld_attr = 3: need 1 <= d <= ld_attr', lambda L, z: sweep(L, z, ld_attr=3)),
    ('d = 0, ld_attr = 4: need 1 <= d <= ld_attr', lambda L, z: sweep(L, z, d=0)),
    ('d = 0, ld_attr = 4: need 1 <= d <= ld_attr', lambda L, z: sweep(L, z, d=0, C=0)),            # (the classes alone need attrs)
    ('sem_first = 3, n_sem = 2: need 0 <= sem_first and sem_first + n_sem <= d = 4', lambda L, z: sweep(L, z, sem_first=3)),
    ('sem_first = -1, n_sem = 2: need 0 <= sem_first', lambda L, z: sweep(L, z, sem_first=-1)),
    ('sem_first = 0, n_sem = 5: need 0 <= sem_first and sem_first + n_sem <= d = 4', lambda L, z: sweep(L, z, sem_first=0, n_sem=5)),
    ('sem_first = 2147483647, n_sem = 2', lambda L, z: sweep(L, z, sem_first=2 ** 31 - 1)),
    ('null attrs with C = 2, n_sem = 2', lambda L, z: sweep(L, z, attrs=None)),
    ('null attrs with C = 0, n_sem = 2', lambda L, z: sweep(L, z, attrs=None, C=0)),
    ('null field with n = 30', lambda L, z: sweep(L, z, field=None)),
    ('null pose / dirs', lambda L, z: sweep(L, z, pose=None)),
    ('null pose / dirs', lambda L, z: sweep(L, z, dirs=None)),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED, zeros_on)


def test_the_symbol_is_in_the_open_table_only():
    lib = pk._lib
    assert 'occ4d_sweep_rays_f32' in lib.ADDON_SIGNATURES
    for pinned in (lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
        assert 'occ4d_sweep_rays_f32' not in pinned


def test_accepted_edges_agree(libraries):
    """No views and an empty ray image are no-ops in both, with null pointers; no channels and no classes take null attrs /
    cols_host; null labels are accepted with any inst pointer; every output may be null, and each alone is accepted; per_view with
    its own table; the limits themselves are accepted."""
    names = ('range', 'point', 'cell', 'owner', 'cosine', 'sem', 'inst', 'feat')
    for L, dev in zip(libraries, (DEV, 'cpu')):
        z = zeros_on(dev)
        nothing = dict(field=None, pose=None, dirs=None, attrs=None, labels=None, **{name: None for name in names})
        assert sweep(L, z, V=0, **nothing) == pk._lib.OK
        assert sweep(L, z, B=0, **nothing) == pk._lib.OK
        assert sweep(L, z, A=0, **nothing) == pk._lib.OK
        assert sweep(L, z, C=0, n_sem=0, attrs=None, cols_host=None, feat=None, sem=None, ld_attr=0, d=0) == pk._lib.OK
        assert sweep(L, z, labels=None, K=0) == pk._lib.OK
        assert sweep(L, z, attrs=None, feat=None, sem=None) == pk._lib.OK          # (attrs is looked at for feat and sem only)
        assert sweep(L, z, **{name: None for name in names}) == pk._lib.OK
        for name in names:
            assert sweep(L, z, **{other: None for other in names if other != name}) == pk._lib.OK
        assert sweep(L, z, per_view=1, dirs=p(z(48, 3))) == pk._lib.OK
        assert sweep(L, z, n_steps=65536, step=1e-6) == pk._lib.OK
        assert sweep(L, z, C=32, cols_host=cols(*([1] * 32)), feat=p(z(2, 12, 32))) == pk._lib.OK
        assert sweep(L, z, sem_first=0, n_sem=4) == pk._lib.OK
        assert sweep(L, z, V=1, B=1, A=1) == pk._lib.OK
    torch.cuda.synchronize()
