"""The running merge of the per-instance reruns (include/occ4d_track.h, inference.perform_inference(track_merge='device'))
through the g++ twin, without a GPU: the two entry points against the reference's own multi_track_merge (tests/golden/
track_merge_*.npz, written by tests/gen_track_fixture.py) and against its numpy restatement over the case matrix of
tests/track_cases.py, and perform_inference / evaluate_clip in track_mode 'all' with the merge on the device against the merge
on the host -- everything EQUAL, no tolerance.  The twin and the HIP kernels share the per-element source
(csrc/track_math.hpp); tests/test_gpu_track.py runs the same comparisons on the device."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import gen_track_fixture as gen
import track_cases as tc
import occlusions4d_amd as pk

CPU = torch.device('cpu')
NAMES = ['occ4d_track_merge_add_f32', 'occ4d_track_merge_finish_f32']


@pytest.fixture
def twin():
    pk.cpu_twin.enable()
    try:
        yield pk
    finally:
        pk.cpu_twin.disable()


def test_signature_table_matches_the_header():
    lib = pk._lib
    with open(lib.TRACK_HEADER_PATH) as f:
        text = f.read()
    assert lib.TRACK_SIGNATURES == lib.parse_prototypes(text, {})
    assert sorted(lib.TRACK_SIGNATURES) == NAMES
    for table in (lib.SIGNATURES, lib.FRONTEND_SIGNATURES, lib.EVAL_SIGNATURES, lib.OCCL_SIGNATURES):
        assert not any(n in table for n in lib.TRACK_SIGNATURES)
    assert lib.parse_constants(text) == {}
    res, args = lib.TRACK_SIGNATURES[NAMES[0]]
    assert res is ctypes.c_int and len(args) == 13 and args[1] is ctypes.c_int64 and args[6] is ctypes.c_float
    res, args = lib.TRACK_SIGNATURES[NAMES[1]]
    assert res is ctypes.c_int and len(args) == 8 and args[1] is ctypes.c_int64 and args[4] is ctypes.c_int


def test_hip_library_exports_the_symbols():
    if not os.path.exists(pk._lib.LIB_PATH):
        pytest.skip('libocc4d.so not built')
    handle = ctypes.CDLL(pk._lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(handle, name), name


def test_twin_binds_the_prototypes(twin):
    lib = pk._lib.lib()
    for name, (res, args) in pk._lib.TRACK_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


def test_fixture_generator_lists_the_committed_files():
    assert [c[:4] for c in gen.CASES] == [(1, 64, 5, 4), (2, 257, 6, 4), (3, 257, 6, 4), (5, 1025, 5, 4), (6, 300, 16, 15),
                                          (7, 300, 29, 15)]
    for name, (K, N, G, track_col, ids) in zip(gen.NAMES, gen.CASES):
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', name + '.npz')
        assert os.path.getsize(path) < 480 * 1024
        z = tc.load_golden(name)
        assert z['outputs'].shape == (K, N, G) and z['ids'].tolist() == ids and max(ids) <= 4095
        s = z['outputs'][:, :, track_col]
        assert s[K - 1, 0] == 0.5 and (s[:, 1] == 0.75).all() and (s[:, 2] < 0.5).all() and np.isnan(s[0, 3])
        assert K == 1 or s[1, 3] > 0.5
        assert z['merged_output'][0, track_col] == ids[-1] and z['merged_output'][1, track_col] == ids[-1]
        assert z['merged_output'][2, track_col] == -1 and z['merged_output'][3, track_col] == -1     # (nothing wins after a NaN)
        rest = np.delete(z['outputs'], track_col, axis=2)
        assert ((rest != 0) & (np.abs(rest) < 1e-38)).any() and np.signbit(rest[rest == 0]).any()


@pytest.mark.parametrize('name', gen.NAMES)
def test_merge_equals_the_reference(twin, name):
    tc.check_golden(name, CPU)


@pytest.mark.parametrize('n', tc.ROW_COUNTS)
def test_merge_case_matrix(twin, n):
    assert tc.check_matrix(n, CPU) == tc.cells_of(n)
    assert tc.cells_of(1025) == 16 * 6 * 8 and tc.cells_of(262401) == 4 * 2 * 8


def test_division_is_not_a_reciprocal_multiply():
    """The restatement the matrix compares with separates the two: at K = 7 every second element differs."""
    x = np.random.default_rng(5).uniform(0, 7, size=4096).astype(np.float32)
    for K in (3, 5, 6, 7):
        assert (x / np.float32(K) != x * np.float32(1.0 / K)).mean() > 0.1


def test_argument_errors(twin):
    tc.check_argument_errors(CPU)


def test_device_merge_equals_host_merge_end_to_end(twin, monkeypatch):
    """... and waits once, and never merges on the host."""
    tc.check_modes_agree(CPU, monkeypatch)
    assert inspect.signature(pk.inference.perform_inference).parameters['track_merge'].default in ('device', 'host')


def test_clip_in_all_mode_reuses_one_encode_per_instance(twin, monkeypatch):
    tc.check_clip_reuses_the_encodes(CPU, monkeypatch)


def test_track_modes_none_and_one_keep_their_encoded_tuple(twin):
    """'none' / 'one' behave as before: `_encoded` is the tuple of the single run, and feeding it back gives the same arrays;
    an unknown track_merge is rejected."""
    pcl, sem, target, inf, enc, dec = inputs = tc.nets(CPU)
    kw = dict(sample_implicit=True, num_sample=tc.CASE['num_sample'], point_sample_mode='grid', batch_size=tc.CASE['batch_size'],
              track_mode='one', data_kind='greater', compress_air=True)
    call = lambda **more: pk.inference.perform_inference(pcl.clone(), sem.copy(), None, [enc, dec], CPU, 'if', inf['min_z'],
                                                         inf['cube_bounds'], inf['color_mode'], 1, None, **kw, **more)
    first = call(return_encoded=True)
    enc_t = first.pop('_encoded')
    assert isinstance(enc_t, tuple) and len(enc_t) == 2 and torch.is_tensor(enc_t[1])
    again = call(encoded=enc_t, track_merge='host')
    tc.same_result(first, again)
    with pytest.raises(AssertionError):
        call(track_merge='numpy')
    all_mode = tc.infer(CPU, inputs, return_encoded=True)['_encoded']
    assert isinstance(all_mode, dict) and sorted(all_mode) == [0, 1, 2] and all(len(v) == 2 for v in all_mode.values())
