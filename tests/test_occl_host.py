"""Per-instance visibility (occlusions4d_amd.occlusion, include/occ4d_occl.h) through the g++ twin, without a GPU: the segmented
id histogram against a numpy restatement over the case matrix of tests/occl_cases.py, valo_ids / choose_track_id and the clip
functions against the reference's own results (tests/golden/occl_*.npz, written by tests/gen_occl_fixture.py) -- everything
EQUAL, no tolerance.  The twin and the HIP kernel share the per-row source (csrc/occl_math.hpp); tests/test_gpu_occl.py runs the
same comparisons on the device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gen_occl_fixture as gen
import occl_cases as oc
import occlusions4d_amd as pk

CPU = torch.device('cpu')


@pytest.fixture
def twin():
    pk.cpu_twin.enable()
    try:
        yield pk
    finally:
        pk.cpu_twin.disable()


def test_signature_table_matches_the_header():
    lib = pk._lib
    with open(lib.OCCL_HEADER_PATH) as f:
        text = f.read()
    assert lib.OCCL_SIGNATURES == lib.parse_prototypes(text, {})
    assert sorted(lib.OCCL_SIGNATURES) == ['occ4d_id_histogram_f32']
    for table in (lib.SIGNATURES, lib.FRONTEND_SIGNATURES, lib.EVAL_SIGNATURES):
        assert not any(n in table for n in lib.OCCL_SIGNATURES)
    assert lib.parse_constants(text) == {'OCCL_' + k: v for k, v in lib.OCCL_CONSTANTS.items()}
    assert lib.OCCL_CONSTANTS == dict(MAX_IDS=4096, EXTRA_BINS=2, NEGATIVE=0, OTHER=1)
    res, args = lib.OCCL_SIGNATURES['occ4d_id_histogram_f32']
    assert res is ctypes.c_int and len(args) == 13 and args[1] is ctypes.c_int64 and args[9] is ctypes.c_float
    assert pk.occlusion.MAX_IDS == 4096


def test_hip_library_exports_the_symbol():
    if not os.path.exists(pk._lib.LIB_PATH):
        pytest.skip('libocc4d.so not built')
    handle = ctypes.CDLL(pk._lib.LIB_PATH)
    for name in pk._lib.OCCL_SIGNATURES:
        assert hasattr(handle, name), name


def test_twin_binds_the_prototype(twin):
    lib = pk._lib.lib()
    for name, (res, args) in pk._lib.OCCL_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


@pytest.mark.parametrize('n', oc.ROW_COUNTS)
def test_histogram_case_matrix(twin, n):
    assert oc.check_matrix(n, CPU) == 3 * 3 * (2 * 3 + 1)


def test_histogram_argument_errors(twin):
    oc.check_argument_errors(CPU)
    rows = torch.zeros(10, 4)
    with pytest.raises(AssertionError, match='ascend'):             # offsets the library can see (the twin: host memory)
        pk.ops.id_histogram(rows, 0, torch.tensor([0, 7, 3, 10]), 4)
    with pytest.raises(AssertionError, match='from 0 to n'):
        pk.ops.id_histogram(rows, 0, torch.tensor([1, 10]), 4)


@pytest.mark.parametrize('name', oc.GOLDEN_NAMES)
def test_valo_ids_equal_the_reference(twin, name):
    oc.check_valo_golden(name, CPU)


@pytest.mark.parametrize('name', oc.GOLDEN_NAMES)
def test_step_by_step_path_equals_the_reference(twin, name):
    """n_ids = 1 leaves the histogram no bin for the ids 1 ..: the call takes the step-by-step path, same results."""
    oc.check_valo_golden(name, CPU, n_ids=1)


@pytest.mark.parametrize('name', [c[0] for c in gen.GREATER_CASES])
def test_choose_track_id_equals_the_reference(twin, name):
    oc.check_track_golden(name, CPU)
    oc.check_track_golden(name, CPU, n_ids=1)                       # (the step-by-step path)


def test_track_modes(twin):
    sem = torch.tensor([[3.0]] * 20 + [[5.0]] * 15 + [[8.0]] * 16 + [[-1.0]] * 40)
    pcl = torch.zeros(91, 7)
    assert pk.occlusion.choose_track_id(pcl, sem, 'none') == -1
    assert pk.occlusion.choose_track_id(pcl, sem, 'snitch') == 0
    state = np.random.get_state()
    assert pk.occlusion.choose_track_id(pcl, sem, 'random') in (3, 8)    # (5 has 15 points, -1 is no id)
    after = np.random.get_state()
    assert after[2] != state[2] or not np.array_equal(after[1], state[1])
    pcl[:, 6] = 1.0                                                  # nothing in the first frame: no draw
    state = np.random.get_state()
    assert pk.occlusion.choose_track_id(pcl, sem, 'random') == -1 and pk.occlusion.choose_track_id(pcl, sem, 'snitch') == -1
    assert np.random.get_state()[2] == state[2]
    with pytest.raises(ValueError):
        pk.occlusion.choose_track_id(pcl, sem, 'nearest')


def _by_the_rule(all_pcl, input_ids, min_points, src_view, frames, max_ids):
    """get_valo_ids' rule on numpy columns, one `==` scan per id (GREATER's arguments)."""
    ids = sorted({int(i) for i in input_ids if i >= 0 and i == np.floor(i) and (input_ids == i).sum() >= min_points})
    live = np.zeros((frames, max_ids))
    for k, i in enumerate(ids):
        c_max = max(sum(int((view[t][:, 3] == i).sum()) for view in all_pcl) for t in range(len(all_pcl[0])))
        for t in range(frames):
            live[t, k] = max(1.0 - int((all_pcl[src_view][t][:, 3] == i).sum()) * len(all_pcl) / (c_max + 1e-6), 0.0)
    pad = -np.ones(max_ids, dtype=np.int32)
    pad[:len(ids)] = ids
    return live, pad, len(ids)


@pytest.mark.parametrize('mode', ['unfilt', 'normal'])
def test_ids_outside_the_bins_and_non_integral_ids(twin, mode):
    rng = np.random.default_rng(5)
    pool = np.array([70000.0, 2.5, 2.0, 7.0, -1.0, 4095.0, 4096.0], dtype=np.float32)
    all_pcl = []
    for v in range(2):
        view = []
        for t in range(3):
            f = np.zeros((300 + 10 * t, 7), dtype=np.float32)
            f[:, 3] = pool[rng.integers(0, len(pool), size=f.shape[0])]
            view.append(f)
        all_pcl.append(view)
    sem = np.concatenate(all_pcl[1])[rng.permutation(930)[:400], 3:4]
    want = _by_the_rule(all_pcl, np.concatenate(all_pcl[1])[:, 3] if mode == 'unfilt' else sem[:, 0], 16 if mode == 'unfilt' else 8,
                        1, 3, 32)
    assert want[2] == 5 and 70000 in want[1] and 4096 in want[1]
    got = pk.occlusion.valo_ids(mode, False, 0, None, 3, 3, 3, 1, 2, 32, [[torch.from_numpy(f) for f in view] for view in all_pcl],
                                torch.from_numpy(sem), None)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] and got[3] is None


def test_modes_and_limits(twin):
    args, _ = oc.golden_arguments('greater_normal', CPU)
    with pytest.raises(ValueError):
        pk.occlusion.valo_ids(**dict(args, live_occl_mode='exact'))
    with pytest.raises(IndexError, match='max_valo_ids'):
        pk.occlusion.valo_ids(**dict(args, max_valo_ids=11))
    with pytest.raises(IndexError, match='max_valo_ids'):
        pk.occlusion.valo_ids(**dict(args, max_valo_ids=11, n_ids=1))
    with pytest.raises(AssertionError):                             # 'unfilt' needs pcl_input_frames == video_length
        pk.occlusion.valo_ids(**dict(args, live_occl_mode='unfilt'))
    inp = oc.fc.greater_inputs()
    with pytest.raises(ValueError):
        pk.frontend.greater_clip(**inp, **gen.GREATER_BY_NAME['greater_normal'][1], live_occl_mode='exact')
    with pytest.raises(ValueError):
        pk.frontend.greater_clip(**inp, **gen.GREATER_BY_NAME['greater_normal'][1], track_mode='nearest')


@pytest.mark.parametrize('name', [c[0] for c in gen.GREATER_CASES])
def test_greater_clip_with_and_without_the_new_arguments(twin, name):
    oc.check_greater_clip(name, CPU)


@pytest.mark.parametrize('name', [c[0] for c in gen.CARLA_CASES])
def test_carla_clip_with_and_without_the_new_arguments(twin, name):
    oc.check_carla_clip(name, CPU)
