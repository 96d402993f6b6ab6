"""Measured returns carved into the query grid (include/ext/occ4d_evidence.h, ops.grid_carve / ops.grid_evidence, evidence.carve /
classify / observe / by_label / rates / Evidence, perform_inference(evidence=...)) through the g++ twin, without a GPU: the header and
its binding, the case matrix of tests/evidence_cases.py against the numpy restatement of the header, the walks worked by hand, the
contention and drop cases, the pins to sight.look's walk, the option object, and perform_inference / evaluate_clip on the refine
fixture -- everything EQUAL.  The twin and the HIP kernels share the body of a return, the code of a cell and the argument contracts
(csrc/evidence_math.hpp), but not where the marks land.  tests/test_gpu_evidence.py runs the same comparisons on the device."""
import ctypes

import pytest
import torch

import evidence_cases as ec
import refine_cases as rc
import occlusions4d_amd as pk

CPU = torch.device('cpu')


@pytest.fixture
def twin():
    pk.cpu_twin.enable()
    try:
        yield pk
    finally:
        pk.cpu_twin.disable()


@pytest.fixture(scope='module')
def shared():
    pk.cpu_twin.enable()
    try:
        return rc.Shared(CPU)
    finally:
        pk.cpu_twin.disable()


def test_symbols_are_in_the_open_table_and_in_no_other():
    lib = pk._lib
    assert lib.ADDON_HEADERS['EVIDENCE'] == 'ext/occ4d_evidence.h' and ('EVIDENCE', 'ext/occ4d_evidence.h', 'addon', True) in lib.HEADERS
    for table in (lib.FEATURE_HEADERS, lib.EXTENSION_HEADERS, lib.STRUCT_EXTENSION_HEADERS):
        assert 'EVIDENCE' not in table
    with open(lib.EVIDENCE_HEADER_PATH) as f:
        text = f.read()
    assert lib.EVIDENCE_SIGNATURES == lib.parse_prototypes(text, lib._STRUCTS) and sorted(lib.EVIDENCE_SIGNATURES) == sorted(ec.SYMBOLS)
    for name in ec.SYMBOLS:
        assert lib.ADDON_SIGNATURES[name] == lib.EVIDENCE_SIGNATURES[name]
        for other in (lib.SIGNATURES, lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
            assert name not in other
    for name, value in ec.CONSTANTS.items():
        assert lib.EVIDENCE_CONSTANTS[name] == value, name
    assert lib.EVIDENCE_CONSTANTS['MAX_COORD'] == lib.SIGHT_CONSTANTS['MAX_COORD'] and lib.ABI_VERSION == 5
    I, L, P, F = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float
    assert lib.EVIDENCE_SIGNATURES['occ4d_evidence_carve_f32'] == (I, [P, L, L, P, P, I, I, I, I, F, F, F, F, F, F, P, P, P, P, P])
    assert lib.EVIDENCE_SIGNATURES['occ4d_evidence_classify_f32'] == (I, [P, L, F, P, L, F, L, P, P, I, P, P, P, P])
    for phrase in ('THE RULES', 'SNAP', 'DROPPED', 'WALK', 'STATE', 'CODE = STATE + 3 * SOLID', 'OUT OF SCOPE', 'ACCESS SAFETY',
                   'floorf((p_a - min_a) / spacing_a)', 'ADVANCE', 'THE SIDE THE RULE ERRS ON IS "UNKNOWN"', 'e == o is a hit and nothing else',
                   'no SQUEEZE and no solid test', 'nx + ny + nz'):
        assert phrase in text, phrase


def test_twin_exports_and_binds_the_prototypes(twin):
    lib = pk._lib.lib()
    handle = ctypes.CDLL(pk.cpu_twin.LIB)
    for name, (res, args) in pk._lib.EVIDENCE_SIGNATURES.items():
        assert hasattr(handle, name), name
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_package_exports():
    for name in ('Evidence', 'carve', 'classify', 'observe', 'by_label', 'rates', 'CODES'):
        assert hasattr(pk.evidence, name), name
    assert hasattr(pk.ops, 'grid_carve') and hasattr(pk.ops, 'grid_evidence') and 'evidence' in pk.__all__


def test_the_math_header_calls_sights_member_test():
    """csrc/evidence_math.hpp includes csrc/sight_math.hpp and calls its member(); it restates no comparison with the level."""
    with open(pk._lib.LIB_PATH.replace('libocc4d.so', 'csrc/evidence_math.hpp')) as f:
        text = f.read()
    assert '#include "sight_math.hpp"' in text and 'sm::member(a.solid, p)' in text
    assert '>= a.level' not in text and 'level >' not in text and 'while (' not in text


@pytest.mark.parametrize('counts', ec.GRIDS, ids=lambda c: '%dx%dx%d' % c)
def test_matrix_equals_the_restatement(twin, counts):
    assert ec.check_matrix(counts, CPU) == len(ec.matrix_cells(counts))


def test_walks_worked_by_hand(twin):
    ec.check_hand_worked(CPU)


def test_contention(twin):
    ec.check_contention(CPU)


def test_drops_are_counted_in_their_priority(twin):
    ec.check_drops(CPU)


def test_pinned_to_the_walk_of_sight(twin):
    ec.check_pinned_to_the_walk_of_sight(CPU)


@pytest.mark.parametrize('share,seed', [(0.15, 11), (0.30, 12)])
def test_seen_solids_contradict_nothing(twin, share, seed):
    ec.check_seen_solids_contradict_nothing(CPU, share, seed)


def test_consequences(twin):
    ec.check_consequences(CPU)


def test_rates():
    ec.check_rates()


def test_argument_errors(twin):
    ec.check_argument_errors(CPU)


def test_option():
    ec.check_option()


def test_signature_positions():
    ec.check_signatures()


def test_perform_inference_with_evidence(shared, twin, monkeypatch):
    ec.check_end_to_end(shared, monkeypatch)


def test_evaluate_clip_appends_the_evidences(shared, twin):
    ec.check_clip(shared)


def test_none_is_untouched(shared, twin, monkeypatch):
    ec.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared, twin):
    ec.check_value_errors(shared)
