"""The decoder's query prelude (include/ext/occ4d_prelude.h) through the g++ twin: the binding's table, the shared argument
contract (csrc/decoder_math.hpp), and the forward entry that takes the prelude's rows = the forward entry that searches itself,
bit for bit (the twin runs the same expressions per row in both).  No GPU."""
import ctypes

import pytest
import torch

import occlusions4d_amd as pk
from query_prelude_cases import ROWS, forward_both_ways, prelude_buffers, scene_of

NAMES = ['occ4d_decoder_query_fwd_prelude_f32', 'occ4d_decoder_query_prelude_f32', 'occ4d_decoder_query_prelude_workspace_floats']


@pytest.fixture(scope='module')
def twin():
    pk.cpu_twin.enable()
    try:
        yield pk
    finally:
        pk.cpu_twin.disable()


def test_signature_table_matches_the_header():
    lib = pk._lib
    assert lib.STRUCT_EXTENSION_HEADERS['PRELUDE'] == 'ext/occ4d_prelude.h'
    with open(lib.PRELUDE_HEADER_PATH) as f:
        text = f.read()
    assert lib.PRELUDE_SIGNATURES == lib.parse_prototypes(text, lib._STRUCTS) == lib.STRUCT_EXTENSION_SIGNATURES
    assert sorted(lib.PRELUDE_SIGNATURES) == NAMES and lib.parse_constants(text) == {}
    assert not set(NAMES) & (set(lib.ALL_SIGNATURES) | set(lib.EXTENSION_SIGNATURES))
    res, args = lib.PRELUDE_SIGNATURES['occ4d_decoder_query_fwd_prelude_f32']
    old = lib.SIGNATURES['occ4d_decoder_query_fwd_f32'][1]
    assert len(args) == len(old) + 3 and args[0] == old[0] and args[-4:] == old[-4:]


def test_twin_exports_and_binds_the_prototypes(twin):
    lib = pk._lib.lib()
    for name, (res, args) in pk._lib.PRELUDE_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype == res and fn.argtypes == args, name


@pytest.mark.parametrize('with_x0', [True, False], ids=['x0', 'lists_only'])
@pytest.mark.parametrize('kind', ['greater', 'carla'])
def test_forward_on_the_prelude_rows_equals_the_forward_that_searches(twin, kind, with_x0):
    dec, xyz, feats, fglobal, q = scene_of(kind, 'cpu')
    (o_ref, p_ref), (o, p), buf = forward_both_ways(dec, xyz, feats, fglobal, q, with_x0)
    assert torch.equal(o, o_ref) and torch.equal(p, p_ref)
    # the rows are what the stand-alone searches give: Euclidean norm with distances, squared distance
    idx8, dist = pk.ops.knn(q, xyz, 8, metric=1, return_dist=True)
    assert torch.equal(buf['idx_local'], idx8) and torch.equal(buf['w_local'], pk.ops.interp_weights(dist))
    assert torch.equal(buf['idx_cross'], pk.ops.knn(q, xyz, 14, metric=0))


def test_argument_contract(twin):
    dec, xyz, feats, fglobal, q = scene_of('greater', 'cpu')
    w, prepared, flags = dec.path_weights()
    buf = prelude_buffers(w, ROWS, 'cpu', True)
    args = (buf['idx_local'], buf['w_local'], buf['idx_cross'], buf['x0'], buf['workspace'])
    with pytest.raises(AssertionError, match='m = 7 abstract points cannot serve the 8 / 14 neighbours'):
        pk.ops.decoder_query_prelude(w, xyz[:7].contiguous(), q, *args)
    sc = dec.prepare_scene(xyz, fglobal, feats)
    with pytest.raises(AssertionError, match="occ4d_decoder_query_fwd_prelude_f32: the prelude's idx_local, w_local, idx_cross rows"):
        pk._lib.check(pk._lib.lib().occ4d_decoder_query_fwd_prelude_f32(
            ctypes.byref(w), pk.ops._ptr(prepared), pk.ops._ptr(sc['scene']), sc['m'], pk.ops._ptr(q), 4, ROWS, None, None, None, None, 0,
            pk.ops._ptr(torch.empty((ROWS, w.d_out))), w.d_out, None, 0, pk.ops._ptr(torch.empty(64)), flags, None, None))
    # n == 0: nothing to do, nothing touched
    empty = prelude_buffers(w, 0, 'cpu', False)
    pk.ops.decoder_query_prelude(w, xyz, q[:0], empty['idx_local'], empty['w_local'], empty['idx_cross'])
