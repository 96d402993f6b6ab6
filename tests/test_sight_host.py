"""Line of sight through the decoded occupancy (include/ext/occ4d_sight.h, sight.py, inference.perform_inference(sight=...)) through
the g++ twin, without a GPU: the header and its binding, the two restatements against each other and on cases worked by hand, the
entry points against them over the case matrix of tests/sight_cases.py, the consequences of the rules (symmetry, walls that hide, the
free components), the option object, and perform_inference / evaluate_clip with Sight on the refine fixture -- everything EQUAL, no
tolerance.  The twin and the HIP kernels share the bit test, the choice of T, the SQUEEZE and the walk (csrc/sight_math.hpp), but not
the order of the queries.  tests/test_gpu_sight.py runs the same comparisons on the device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import refine_cases as rc
import sight_cases as sc
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
    assert lib.ADDON_HEADERS['SIGHT'] == 'ext/occ4d_sight.h'
    for table in (lib.FEATURE_HEADERS, lib.EXTENSION_HEADERS, lib.STRUCT_EXTENSION_HEADERS):
        assert 'SIGHT' not in table
    with open(lib.SIGHT_HEADER_PATH) as f:
        text = f.read()
    assert lib.SIGHT_SIGNATURES == lib.parse_prototypes(text, lib._STRUCTS) and sorted(lib.SIGHT_SIGNATURES) == sc.SYMBOLS
    for name in sc.SYMBOLS:
        assert lib.ADDON_SIGNATURES[name] == lib.SIGHT_SIGNATURES[name]
        for other in (lib.SIGNATURES, lib.ALL_SIGNATURES, lib.EXTENSION_SIGNATURES, lib.STRUCT_EXTENSION_SIGNATURES):
            assert name not in other
    k = lib.SIGHT_CONSTANTS
    assert k == dict(MAX_AXIS=512, MAX_ORIGINS=31, MAX_COORD=2 ** 20, BLOCK_X=4, BLOCK_Y=4, BLOCK_Z=4)
    assert k['BLOCK_X'] * k['BLOCK_Y'] * k['BLOCK_Z'] == 64 and k['MAX_AXIS'] == lib.DISTANCE_CONSTANTS['MAX_AXIS'] and sc.FAR == k['MAX_COORD']
    assert sc.FLAGS == (0,)                                                             # one variant of the walk stayed
    assert lib.ABI_VERSION == 5
    I, P, L, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert lib.SIGHT_SIGNATURES['occ4d_sight_bits_f32'] == (I, [P, L, F, P, L, F, L, P, P])
    assert lib.SIGHT_SIGNATURES['occ4d_sight_grid_u32'] == (I, [P, I, I, I, P, I, P, P, P, I, P])
    for phrase in ('THE RULES', 'LAUNCHES', 'ACCESS SAFETY', 'SQUEEZE', 'THE ONLY APPROXIMATION'):
        assert phrase in text, phrase


def test_twin_exports_and_binds_the_prototypes(twin):
    lib = pk._lib.lib()
    handle = ctypes.CDLL(pk.cpu_twin.LIB)
    for name, (res, args) in pk._lib.SIGHT_SIGNATURES.items():
        assert hasattr(handle, name), name
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_restatements_agree_on_every_small_grid():
    sc.check_restatements_agree()


def test_cases_worked_by_hand(twin):
    sc.check_by_hand(CPU)


@pytest.mark.parametrize('counts', sc.GRIDS, ids=sc.GRID_IDS)
def test_matrix_equals_the_restatement_twice(twin, counts):
    assert sc.check_grid(counts, CPU) == len(sc.FIELDS) * len(sc.origin_counts(counts)) * 3 * 2 * len(sc.FLAGS) * 2


def test_raw_entry_points_write_nothing_else(twin):
    sc.check_raw_canaries(CPU, pk._lib.lib())


def test_consequences_of_the_rules(twin):
    sc.check_consequences(CPU)


def test_argument_errors(twin):
    sc.check_argument_errors(CPU)


def test_option_object_and_signatures():
    pts = [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]
    s = pk.sight.Sight(origins=pts)
    assert (s.level, s.select, s.blocker, s.cameras) == (None, None, False, None) and s.origins.tolist() == pts and s.origins.dtype == np.float64
    assert (s.keyword, s.clip_list, s.needs, s.into) == ('sight', ('sights', 'one dict of seen[, framed][, blocker]'), None, None)
    assert isinstance(s, pk.products.LevelProduct) and s.resolve(0.5) == 0.5
    assert repr(s) == 'Sight(V=2, origins, level=None, select=None, blocker=False)'
    s = pk.sight.Sight(origins=np.zeros((31, 3)), level=0.25, select=(3, 0.5), blocker=True)
    assert (s.level, s.select, s.blocker) == (0.25, (3, 0.5), True) and s.resolve(0.5) == 0.25
    RT = np.concatenate([np.eye(3), [[1.0], [2.0], [3.0]]], axis=1)[None]
    s = pk.sight.Sight(cameras=(RT, np.eye(3), 4, 6))
    assert s.origins.tolist() == [[-1.0, -2.0, -3.0]] and s.cameras[2:] == (4, 6)     # the centre of [I | t] is -t
    assert repr(s) == 'Sight(V=1, cameras 4 x 6, level=None, select=None, blocker=False)'
    grid = pk.products.Grid(((4, 4, 4), (0.0, 0.0, 0.0), (0.5, 0.5, 0.5)), 0.5, False, 13, CPU)
    assert grid.points is None and grid.output is None
    level, ijk = s.prepare(grid)
    assert level == 0.5 and ijk.dtype == np.int32 and ijk.tolist() == [[-2, -4, -6]]
    for kw, text in ((dict(), 'exactly one of origins and cameras'), (dict(origins=pts, cameras=(RT, np.eye(3), 4, 6)), 'exactly one of'),
                     (dict(origins=np.zeros((0, 3))), r'V = 0 origins, must be in \[1, 31\]'), (dict(origins=np.zeros((32, 3))), 'V = 32 origins'),
                     (dict(cameras=(np.zeros((32, 3, 4)) + RT, np.eye(3), 4, 6)), 'V = 32 origins'),
                     (dict(origins=pts, level=float('nan')), 'level is NaN'), (dict(origins=pts, select=5), 'select = 5 must be'),
                     (dict(origins=[0.0, 1.0, 2.0]), r'origins must be \(V, 3\)'), (dict(cameras=(RT, np.eye(3))), 'cameras must be'),
                     (dict(cameras=(RT, np.eye(3), -1, 6)), 'height = -1')):
        with pytest.raises(ValueError, match=text):
            pk.sight.Sight(**kw)
    far = pk.sight.Sight(origins=[[0.0, 0.0, 0.5 * (2 ** 20 + 1)]])                     # an origin beyond 2^20 cells: in prepare()
    with pytest.raises(ValueError, match='beyond 2\\^20 cells'):
        far.prepare(grid)
    assert pk.sight.Sight(origins=[[0.0, 0.0, 0.5 * 2 ** 20]]).prepare(grid)[1].tolist() == [[0, 0, 2 ** 20]]
    sig = inspect.signature(pk.inference.perform_inference).parameters
    names = list(sig)
    assert sig['sight'].default is None and names[-4:] == ['sight', 'segments', 'tracker', 'clearance']
    sig = inspect.signature(pk.evaluation.evaluate_clip).parameters
    assert sig['sight'].default is None and sig['sights'].default is None
    assert list(sig)[-6:] == ['sight', 'sights', 'segments', 'parts', 'route', 'routes']
    assert list(inspect.signature(pk.sight.look).parameters) == ['implicit_output', 'counts', 'origins_ijk', 'level', 'select', 'framed', 'blocker',
                                                                 'channel']
    assert list(inspect.signature(pk.ops.grid_sight).parameters) == ['bits', 'counts', 'origins', 'framed', 'blocker', 'flags']
    assert list(inspect.signature(pk.ops.grid_solid_bits).parameters) == ['values', 'level', 'mask', 'mask_level']
    assert 'sight' in pk.__all__
    doc = ' '.join(pk.sight.__doc__.split())
    assert 'at most one cell' in doc and 'There is no checkpoint' in doc
    for text in (pk.inference.perform_inference.__doc__, pk.evaluation.evaluate_clip.__doc__):
        assert 'sight.Sight' in text


def test_grid_origin():
    sc.check_grid_origin()


def test_look_against_the_restatement(twin):
    sc.check_look(CPU)


def test_codes_and_by_label_against_numpy(twin):
    sc.check_codes_and_by_label(CPU)


def test_perform_inference_with_sight(twin, shared, monkeypatch):
    sc.check_end_to_end(shared, monkeypatch)


def test_evaluate_clip_passes_sight_through(twin, shared):
    sc.check_clip(shared)


def test_sight_none_is_untouched(twin, shared, monkeypatch):
    sc.check_none_is_untouched(shared, monkeypatch)


def test_value_errors(twin, shared):
    sc.check_value_errors(shared)
