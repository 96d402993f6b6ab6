"""The rejected-call table of tests/contract_texts.py for the entry points of include/ext/occ4d_evidence.h: libocc4d.so and the g++
twin take the argument contracts from one source (check_carve / check_classify of csrc/evidence_math.hpp over csrc/contract.hpp).
Both are loaded in one process -- the twin as a second plain handle, never enabled -- and handed the same rejected calls, device
tensors for the one and same-shaped host tensors for the other: the same status and the same occ4d_last_error() bytes."""
import numpy as np
import pytest
import torch

import occlusions4d_amd as pk
from contract_texts import libraries, p, rejected_test, zeros_on  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
F32, I64 = torch.float32, torch.int64
NAN, INF = float('nan'), float('inf')


def carve(L, z, **k):
    """Seven returns of two sensors into a 3 x 2 x 5 grid (30 cells, one word)."""
    a = dict(returns=p(z(7, 4, dtype=F32)), ld=4, R=7, sensor=p(z(7)), origins=p(z(2, 3)), V=2, nx=3, ny=2, nz=5, x0=0.0, sx=1.0, y0=0.0,
             sy=1.0, z0=0.0, sz=1.0, passed=p(z(1)), hits=p(z(30)), passes=p(z(30)), status=p(z(4)))
    a.update(k)
    return L.occ4d_evidence_carve_f32(*a.values(), None)


def classify(L, z, **k):
    a = dict(field=p(z(30, dtype=F32)), ld=1, level=0.5, mask=p(z(30, dtype=F32)), ld_mask=1, mask_level=0.5, n=30, passed=p(z(1)),
             passes=p(z(30)), min_pass=1, hits=p(z(30)), code=p(z(30)), totals=p(z(6, dtype=I64)))
    a.update(k)
    return L.occ4d_evidence_classify_f32(*a.values(), None)


# (message fragment, call(L, z)): z(*shape, dtype) is a zeros tensor where the library L reads
REJECTED = [
    ('occ4d_evidence_carve_f32: R = -1 must be in [0, INT32_MAX]', lambda L, z: carve(L, z, R=-1)),
    ('R = 2147483648 must be in [0, INT32_MAX]', lambda L, z: carve(L, z, R=2 ** 31)),
    ('ld_returns = 2 must be >= 3', lambda L, z: carve(L, z, ld=2)),
    ('V = 0 must be in [1, 4096]', lambda L, z: carve(L, z, V=0)),
    ('V = 4097 must be in [1, 4096]', lambda L, z: carve(L, z, V=4097)),
    ('V = -3 must be in [1, 4096]', lambda L, z: carve(L, z, V=-3)),
    ('nx = -1, ny = 2, nz = 5 must be >= 0', lambda L, z: carve(L, z, nx=-1)),
    ('nx = 3, ny = 513, nz = 5 must be <= 512', lambda L, z: carve(L, z, ny=513)),
    ('nx = 3, ny = 2, nz = 2147483647 must be <= 512', lambda L, z: carve(L, z, nz=2 ** 31 - 1)),
    ('min = (nan, 0, 0) must be finite', lambda L, z: carve(L, z, x0=NAN)),
    ('min = (0, 0, -inf) must be finite', lambda L, z: carve(L, z, z0=-INF)),
    ('spacing = (0, 1, 1) must be finite and > 0', lambda L, z: carve(L, z, sx=0.0)),
    ('spacing = (1, -1, 1) must be finite and > 0', lambda L, z: carve(L, z, sy=-1.0)),
    ('spacing = (1, 1, inf) must be finite and > 0', lambda L, z: carve(L, z, sz=INF)),
    ('spacing = (1, nan, 1) must be finite and > 0', lambda L, z: carve(L, z, sy=NAN)),
    ('null status', lambda L, z: carve(L, z, status=None)),
    ('null passed / hits with n = 30', lambda L, z: carve(L, z, passed=None)),
    ('null passed / hits with n = 30', lambda L, z: carve(L, z, hits=None)),
    ('null returns with R = 7', lambda L, z: carve(L, z, returns=None)),
    ('null origins with V = 2', lambda L, z: carve(L, z, origins=None)),
    ('occ4d_evidence_classify_f32: n = -1 must be in [0, INT32_MAX]', lambda L, z: classify(L, z, n=-1)),
    ('n = 2147483648 must be in [0, INT32_MAX]', lambda L, z: classify(L, z, n=2 ** 31)),
    ('ld = 0 must be >= 1', lambda L, z: classify(L, z, ld=0)),
    ('ld_mask = 0 must be >= 1', lambda L, z: classify(L, z, ld_mask=0)),
    ('min_pass = 0 must be >= 1', lambda L, z: classify(L, z, min_pass=0)),
    ('min_pass = 2 needs passes', lambda L, z: classify(L, z, passes=None, min_pass=2)),
    ('null totals', lambda L, z: classify(L, z, totals=None)),
    ('null field with n = 30', lambda L, z: classify(L, z, field=None)),
    ('null passed and null passes with n = 30', lambda L, z: classify(L, z, passed=None, passes=None)),
    ('null hits / code with n = 30', lambda L, z: classify(L, z, hits=None)),
    ('null hits / code with n = 30', lambda L, z: classify(L, z, code=None)),
]


test_both_libraries_reject_with_the_same_text = rejected_test(REJECTED, zeros_on)


def test_the_symbols_are_in_the_open_table_only():
    lib = pk._lib
    for name in ('occ4d_evidence_carve_f32', 'occ4d_evidence_classify_f32'):
        assert name in lib.ADDON_SIGNATURES
        for pinned in (lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
            assert name not in pinned


def test_accepted_edges_agree(libraries):
    """R = 0 clears and needs neither returns nor origins; N = 0 (an axis of length 0) needs no cell array and drops every return
    as outside; a null sensor table; null passes; V = 4096; the longest axes; classify of no cell; classify from the bits alone
    and from the counts alone.  Both libraries leave the same outputs."""
    results = []
    for L, dev in zip(libraries, (DEV, 'cpu')):
        z = zeros_on(dev)
        out = []

        def ok(rc, *tensors):
            assert rc == pk._lib.OK
            if dev != 'cpu':
                torch.cuda.synchronize()
            out.extend(t.cpu().numpy().copy() for t in tensors)

        status, hits = z(4) + 9, z(30) + 9
        ok(carve(L, z, R=0, returns=None, sensor=None, origins=None, status=p(status), hits=p(hits)), status, hits)
        status = z(4) + 9
        ok(carve(L, z, ny=0, passed=None, hits=None, passes=None, status=p(status)), status)
        assert out[-1].tolist() == [0, 0, 0, 7]
        status, hits = z(4), z(30)
        ok(carve(L, z, sensor=None, passes=None, status=p(status), hits=p(hits)), status, hits)
        assert out[-2].tolist() == [7, 0, 0, 0] and out[-1][0] == 7
        status = z(4)
        ok(carve(L, z, V=4096, origins=p(z(4096, 3)), status=p(status)), status)
        ok(carve(L, z, nx=512, ny=512, nz=1, passed=p(z(8192)), hits=p(z(512 * 512)), passes=p(z(512 * 512))))
        ok(carve(L, z, R=1), )
        totals = z(6, dtype=I64) + 9
        ok(classify(L, z, n=0, field=None, mask=None, passed=None, passes=None, hits=None, code=None, totals=p(totals)), totals)
        assert out[-1].tolist() == [0] * 6
        totals, code = z(6, dtype=I64), z(30)
        ok(classify(L, z, level=-1.0, passes=None, mask=None, totals=p(totals), code=p(code)), totals, code)
        assert out[-2].tolist() == [0, 0, 0, 30, 0, 0]
        totals = z(6, dtype=I64)
        ok(classify(L, z, passed=None, min_pass=2 ** 31 - 1, totals=p(totals)), totals)
        results.append(out)
    assert len(results[0]) == len(results[1])
    for a, b in zip(*results):
        assert np.array_equal(a, b)
