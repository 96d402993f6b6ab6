"""The next best view over the query grid (include/ext/occ4d_viewplan.h, ops.grid_visible / viewplan_greedy, sight.plan / NextView /
cells_to_world, perform_inference(next_view=...)) through the g++ twin, without a GPU: the header and its binding, the case matrix of
tests/viewplan_cases.py against the restatement of the header, GREEDY and a wall worked by hand, the consequences of the rules on what
the library returns, the raw entry points with canaries, the option object, and perform_inference / evaluate_clip on the refine
fixture -- everything EQUAL, no tolerance.  The twin and the HIP kernels share DEAD, RANGE, the pair test, the keys and the argument
contracts (csrc/viewplan_math.hpp over csrc/sight_math.hpp), but neither the order of the work nor the reductions.
tests/test_gpu_viewplan.py runs the same comparisons on the device."""
import ctypes

import pytest
import torch

import viewplan_cases as vc
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
    """ADDON_HEADERS is open by design: this header's symbols are IN it -- the table is never compared with them."""
    lib = pk._lib
    assert lib.ADDON_HEADERS['VIEWPLAN'] == 'ext/occ4d_viewplan.h'
    for table in (lib.FEATURE_HEADERS, lib.EXTENSION_HEADERS, lib.STRUCT_EXTENSION_HEADERS):
        assert 'VIEWPLAN' not in table
    with open(lib.VIEWPLAN_HEADER_PATH) as f:
        text = f.read()
    assert lib.VIEWPLAN_SIGNATURES == lib.parse_prototypes(text, lib._STRUCTS) and sorted(lib.VIEWPLAN_SIGNATURES) == sorted(vc.SYMBOLS)
    for name in vc.SYMBOLS:
        assert lib.ADDON_SIGNATURES[name] == lib.VIEWPLAN_SIGNATURES[name]
        for other in (lib.SIGNATURES, lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
            assert name not in other
    assert lib.VIEWPLAN_CONSTANTS == dict(MAX_CANDIDATES=4096, MAX_PICKS=32, MAX_WEIGHT=1024, CHUNK=8, SLICE=4096) and lib.ABI_VERSION == 5
    I, P, L = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert lib.VIEWPLAN_SIGNATURES['occ4d_viewplan_visible_u32'] == (I, [P, I, I, I, P, P, I, I, I, I, L, P, P])
    assert lib.VIEWPLAN_SIGNATURES['occ4d_viewplan_greedy_u32'] == (I, [P, I, L, P, I, P, P, P, P, P, P])
    for phrase in ('THE RULES', 'LAUNCHES', 'ACCESS SAFETY', 'CANDIDATES', 'DEAD', 'RANGE', 'VIS', 'GREEDY', 'A DEAD CANDIDATE SEES NOTHING',
                   'THE LOWEST c', 'before any coordinate is used', 'ONE GREEDY PASS', '1 + 2 * max(k, 1)', 'is tested against [0, C)'):
        assert phrase in text, phrase


def test_twin_exports_and_binds_the_prototypes(twin):
    lib = pk._lib.lib()
    handle = ctypes.CDLL(pk.cpu_twin.LIB)
    for name, (res, args) in pk._lib.VIEWPLAN_SIGNATURES.items():
        assert hasattr(handle, name), name
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_package_exports():
    for name in ('plan', 'NextView', 'cells_to_world', 'Sight', 'look', 'grid_origin'):
        assert hasattr(pk.sight, name), name
    for name in vc.OPS:
        assert hasattr(pk.ops, name), name


@pytest.mark.parametrize('counts', vc.GRIDS, ids=vc.GRID_IDS)
def test_matrix_equals_the_restatement_twice(twin, counts):
    calls, live_inside, dead_solid = vc.check_grid(counts, CPU)
    assert calls == len(vc.FIELDS) * 12 * 2
    if counts == (3, 2, 5):
        assert live_inside >= 6 and dead_solid >= 6                                     # both kinds of candidate inside the grid occur


def test_greedy_by_hand(twin):
    vc.check_greedy_by_hand(CPU, pk._lib.lib())


def test_wall_by_hand(twin):
    vc.check_wall_by_hand(CPU)


def test_consequences_of_the_rules(twin):
    vc.check_consequences(CPU)


def test_raw_calls_write_nothing_else(twin):
    vc.check_raw_canaries(CPU, pk._lib.lib())


def test_argument_errors(twin):
    vc.check_argument_errors(CPU)


def test_plan_equals_the_restatement(twin):
    vc.check_plan(CPU)


def test_cells_to_world():
    vc.check_cells_to_world()


def test_option():
    vc.check_option()


def test_signature_positions():
    vc.check_signatures()


def test_perform_inference_with_next_view(shared, twin, monkeypatch):
    vc.check_end_to_end(shared, monkeypatch)


def test_evaluate_clip_appends_the_plans(shared, twin):
    vc.check_clip(shared)


def test_none_is_untouched(shared, twin, monkeypatch):
    vc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(shared, twin):
    vc.check_value_errors(shared)
