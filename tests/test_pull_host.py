"""Straight free legs over the query grid (include/ext/occ4d_pull.h, geodesic.straight / pull / polyline_length, Route(pull=True))
through the g++ twin, without a GPU: the header and its binding, the bits, pairwise line of sight over the case matrix of
tests/pull_cases.py against the restatement of the header, the consequences of the rules (symmetry, walls that separate), the pulled
paths of the library's own solve() with their pinned counts, hand-made chains through the raw entry point, the option object, and
perform_inference / evaluate_clip with Route(pull=True) on the refine fixture -- everything EQUAL; the one tolerance is derived in
pull_cases.LENGTH_MARGIN.  The twin and the HIP kernels share the blocked test, HIT and the candidate test (csrc/pull_math.hpp over
csrc/sight_math.hpp), but not the order of the candidates.  tests/test_gpu_pull.py runs the same comparisons on the device."""
import ctypes

import pytest
import torch

import pull_cases as pc
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
    assert lib.ADDON_HEADERS['PULL'] == 'ext/occ4d_pull.h'
    for table in (lib.FEATURE_HEADERS, lib.EXTENSION_HEADERS, lib.STRUCT_EXTENSION_HEADERS):
        assert 'PULL' not in table
    with open(lib.PULL_HEADER_PATH) as f:
        text = f.read()
    assert lib.PULL_SIGNATURES == lib.parse_prototypes(text, lib._STRUCTS) and sorted(lib.PULL_SIGNATURES) == sorted(pc.SYMBOLS)
    for name in pc.SYMBOLS:
        assert lib.ADDON_SIGNATURES[name] == lib.PULL_SIGNATURES[name]
        for other in (lib.SIGNATURES, lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
            assert name not in other
    assert lib.PULL_CONSTANTS == dict(ROUND=256, LDS_WORDS=32768) and lib.ABI_VERSION == 5
    I, P, L = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert lib.PULL_SIGNATURES['occ4d_pull_bits_i32'] == (I, [P, I, L, P, P])
    assert lib.PULL_SIGNATURES['occ4d_pull_pairs_u32'] == (I, [P, I, I, I, P, P, I, P, P])
    assert lib.PULL_SIGNATURES['occ4d_pull_paths_i32'] == (I, [P, I, I, I, P, P, I, I, P, P, P])
    for phrase in ('THE RULES', 'LAUNCHES', 'ACCESS SAFETY', 'BLOCKED', 'FREE(a, b)', 'HIT(a, b)', 'PULL', 'NEVER FIRES', 'DEPENDS ON THE DIRECTION',
                   'symmetric', 'KEPT UNTESTED', 'NOT THE EUCLIDEAN SHORTEST PATH'):
        assert phrase in text, phrase


def test_twin_exports_and_binds_the_prototypes(twin):
    lib = pk._lib.lib()
    handle = ctypes.CDLL(pk.cpu_twin.LIB)
    for name, (res, args) in pk._lib.PULL_SIGNATURES.items():
        assert hasattr(handle, name), name
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_package_exports():
    for name in ('straight', 'pull', 'polyline_length', 'Route', 'solve', 'paths_to_world'):
        assert hasattr(pk.geodesic, name), name
    for name in pc.OPS:
        assert hasattr(pk.ops, name), name


def test_bits_equal_the_restatement(twin):
    assert pc.check_bits(CPU) == len(pc.BIT_LENGTHS) * len(pc.MIN_CLEARS) * 2


@pytest.mark.parametrize('counts', pc.PAIR_GRIDS, ids=pc.PAIR_GRID_IDS)
def test_pairs_equal_the_restatement_twice(twin, counts):
    assert pc.check_pairs(counts, CPU) == len(pc.FIELDS) * 2


def test_pair_counts_round_the_wave(twin):
    pc.check_pair_counts(CPU)


def test_consequences_of_the_rules(twin):
    pc.check_consequences(CPU)


@pytest.mark.parametrize('name', [n for n in pc.PULL_NAMES if n not in pc.RANDOM30])
def test_pulled_paths_equal_the_restatement_twice(twin, name):
    pc.check_pull_case(name, CPU)


def test_random_fields_take_the_fallback_leg(twin):
    """On 30 %-solid fields a legal edge or corner move between two blocked side cells occurs in practice: the rule is exercised."""
    assert sum(pc.check_pull_case(name, CPU) for name in pc.RANDOM30) >= 1


def test_pinned_shapes(twin):
    pc.check_pinned_shapes(CPU)


def test_hand_made_chains_through_the_raw_entry_point(twin):
    pc.check_hand_chains(CPU, pk._lib.lib())


@pytest.mark.parametrize('counts', pc.THRESHOLD_GRIDS, ids=['largest-staged', 'first-beyond'])
def test_either_side_of_the_staging_limit(twin, counts):
    pc.check_threshold(counts, CPU, pk._lib.lib())


def test_argument_errors(twin):
    pc.check_argument_errors(CPU)


def test_polyline_length():
    pc.check_polyline_length()


def test_paths_to_world_takes_waypoints(twin):
    pc.check_paths_to_world_takes_waypoints(CPU)


def test_route_option():
    pc.check_route_option()


def test_perform_inference_with_pull(shared, twin, monkeypatch):
    pc.check_end_to_end(shared, monkeypatch)


def test_evaluate_clip_passes_the_waypoints_through(shared, twin):
    pc.check_clip(shared)


def test_pull_false_is_untouched(shared, twin, monkeypatch):
    pc.check_pull_false_is_untouched(shared, monkeypatch)
