"""CPU: the C-ABI library loads without a GPU and exports exactly what include/occ4d.h declares;
the ctypes table (occlusions-4d_amd/_lib.py) names the same symbols.  No compute calls here."""
import ctypes
import os
import re

import pytest

import occlusions4d_amd as pk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(ROOT, 'include', 'occ4d.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(occ4d_[a-z0-9_]+)\s*\(', text)))


def test_header_declares_entry_points():
    syms = header_symbols()
    assert 'occ4d_knn_f32' in syms and 'occ4d_linear_f32' in syms and 'occ4d_fps_f32' in syms
    assert len(syms) >= 15


def test_ctypes_table_matches_header():
    assert sorted(pk._lib.SIGNATURES) == header_symbols()


def test_library_loads_and_exports_every_symbol():
    lib = pk._lib.lib()           # raises NativeLibraryError if absent/stale
    raw = ctypes.CDLL(pk._lib.LIB_PATH)
    for name in header_symbols():
        assert hasattr(raw, name), name
    assert lib.occ4d_abi_version() == pk._lib.ABI_VERSION


def test_linear_args_struct_layout():
    a = pk._lib.LinearArgs
    assert ctypes.sizeof(a) == 144
    assert a.M.offset == 72 and a.add_rows.offset == 96 and a.sub_idx.offset == 136


def test_cpu_tensors_are_rejected_loudly():
    import torch
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pk.ops.linear(torch.zeros(4, 8), torch.zeros(4, 8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pk.point_transformer_layer.kNN_torch(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), 2)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(pk._lib, '_lib', None)
    monkeypatch.setattr(pk._lib, 'LIB_PATH', str(tmp_path / 'libocc4d.so'))
    with pytest.raises(pk._lib.NativeLibraryError, match='no CPU/PyTorch fallback'):
        pk._lib.lib()


# ---- the binding is derived from the header (occlusions-4d_amd/_lib.py: parse_prototypes / parse_constants) ----------

class _S(ctypes.Structure):
    _fields_ = [('x', ctypes.c_int)]


def _parse(text):
    return pk._lib.parse_prototypes(text, {'occ4d_thing': _S})


def test_parser_maps_every_argument_kind():
    C = ctypes
    sig = _parse('''
        /* a comment with occ4d_not_a_function(int) inside */
        #define OCC4D_X 1
        typedef struct occ4d_thing { int32_t a, b; const float* p; } occ4d_thing;
        int occ4d_scalars(int a, int32_t b, int64_t c, unsigned d, float e, double f);   // trailing comment
        int64_t occ4d_pointers(const float* a, float* b, double* c, const int32_t* d, int* e, int64_t* f,
                               const void* g, void* stream, unsigned long long* h);
        const char* occ4d_text(void);
        float occ4d_structs(const occ4d_thing* w, occ4d_thing* ev);
        int occ4d_spacing( const float *a , int64_t  lda );
    ''')
    assert sig == {
        'occ4d_scalars': (C.c_int, [C.c_int, C.c_int32, C.c_int64, C.c_uint, C.c_float, C.c_double]),
        'occ4d_pointers': (C.c_int64, [C.c_void_p] * 9),
        'occ4d_text': (C.c_char_p, []),
        'occ4d_structs': (C.c_float, [C.POINTER(_S), C.POINTER(_S)]),
        'occ4d_spacing': (C.c_int, [C.c_void_p, C.c_int64]),
    }


@pytest.mark.parametrize('text, match', [
    ('int occ4d_f(size_t n);', 'size_t'),                                       # a type the mapping does not know
    ('int occ4d_f(const char* name);', 'char'),                                 # char* is a return type only
    ('int occ4d_f(float** rows);', 'occ4d_f'),                                  # pointer to pointer
    ('int occ4d_f(unsigned long n);', 'occ4d_f'),                               # (would otherwise read as `unsigned` named long)
    ('void occ4d_f(int n);', 'void'),                                           # no entry point returns void
    ('int occ4d_f(int n, void (*done)(int));', 'occ4d_f'),                      # function-pointer parameter
    ('int occ4d_f(int n, float* out', 'occ4d_f'),                               # truncated: neither `)` nor `;`
    ('int occ4d_f(int n, float* out)\nint occ4d_g(void);', 'occ4d_f'),          # prototype without `;`
    ('int occ4d_f(int n);\nint occ4d_g(int n)', 'occ4d_g'),                     # the last one without `;`
    ('int occ4d_f(int n);\nint occ4d_f(int n);', 'occ4d_f'),                    # declared twice
    ('int occ4d_f(int n);\nextern int something_else;', 'something_else'),      # anything that is no prototype
])
def test_parser_is_strict(text, match):
    with pytest.raises(pk._lib.NativeLibraryError, match=match):
        _parse(text)


def test_constants_parser():
    parse = pk._lib.parse_constants
    assert parse('#ifndef OCC4D_H_\n#define OCC4D_H_\n#define OCC4D_A 7   /* seven */\n# define OCC4D_B (-2)\n#define OTHER x') \
        == {'A': 7, 'B': -2}
    with pytest.raises(pk._lib.NativeLibraryError, match='OCC4D_C'):
        parse('#define OCC4D_C (1 << 3)')


def test_missing_header_fails_loudly(tmp_path):
    import importlib.util
    pkg = tmp_path / 'pkg'
    pkg.mkdir()
    (pkg / '_lib.py').write_text(open(pk._lib.__file__.replace('.pyc', '.py')).read())
    spec = importlib.util.spec_from_file_location('occ4d_lib_without_header', str(pkg / '_lib.py'))
    with pytest.raises(Exception, match='occ4d.h not found') as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(e.value).__name__ == 'NativeLibraryError'


def _kind(t):
    if t in (ctypes.c_float, ctypes.c_double):
        return 'float', ctypes.sizeof(t)
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return 'pointer', ctypes.sizeof(t)
    assert issubclass(t, ctypes._SimpleCData) and t._type_ in 'bBhHiIlLqQ', t
    return 'integer', ctypes.sizeof(t)


def test_derived_signatures_match_the_foreign_callers_stub():
    """tests/test_gpu_cabi_only.py restates the header by hand for the entry points it drives: the independent witness.
    Argument count, and size and kind of the return value and of every argument, equal the derived entry."""
    import test_gpu_cabi_only as stub
    assert len(stub.SIG) == 24
    for name, (res, args) in stub.SIG.items():
        dres, dargs = pk._lib.SIGNATURES[name]
        assert _kind(res) == _kind(dres), name
        assert len(args) == len(dargs), name
        for i, (a, d) in enumerate(zip(args, dargs)):
            assert _kind(a) == _kind(d), (name, i, a, d)
    # the struct pointers of both sides point at the same layout
    for mine, theirs in ((pk._lib.PtLayerWeights, stub.LayerW), (pk._lib.DecoderWeights, stub.DecoderW)):
        assert ctypes.sizeof(mine) == ctypes.sizeof(theirs)
        assert [getattr(mine, n).offset for n, _ in mine._fields_] == [getattr(theirs, n).offset for n, _ in theirs._fields_]


def test_derived_constants_are_the_pinned_abi():
    """The values the binding held as literals before it was derived.  An ABI bump is made HERE, consciously."""
    L = pk._lib
    assert L.ABI_VERSION == 5
    assert (L.OK, L.EINVAL, L.ELAUNCH) == (0, -1, -2)
    assert (L.PATH_DEFAULT, L.PATH_UNFUSED, L.PATH_FIRST_GEN, L.PATH_GENERIC_LINEAR, L.PATH_TRUNK4, L.PATH_FUSED_INTERP,
            L.PATH_BF16X6, L.PATH_BF16X6_TRUNK, L.PATH_SPLIT_F16) == (0, 1, 2, 8, 16, 32, 64, 128, 256)
    assert (L.PROFILE_CROSS_ATTN, L.PROFILE_RESBLOCK, L.PROFILE_ROWLIN) == (1, 2, 3)
    assert (L.MAX_BLOCKS, L.MAX_CROSS) == (16, 4)
    assert L.PROFILE_KINDS == {'cross_attn': 1, 'resblock': 2, 'rowlin': 3}
    assert L.CONSTANTS == {'ABI_VERSION': 5, 'OK': 0, 'EINVAL': -1, 'ELAUNCH': -2, 'PATH_DEFAULT': 0, 'PATH_UNFUSED': 1,
                           'PATH_FIRST_GEN': 2, 'PATH_GENERIC_LINEAR': 8, 'PATH_TRUNK4': 16, 'PATH_FUSED_INTERP': 32,
                           'PATH_BF16X6': 64, 'PATH_BF16X6_TRUNK': 128, 'PATH_SPLIT_F16': 256, 'PROFILE_CROSS_ATTN': 1,
                           'PROFILE_RESBLOCK': 2, 'PROFILE_ROWLIN': 3, 'MAX_BLOCKS': 16, 'MAX_CROSS': 4}


def test_derived_table_covers_the_header():
    sig = pk._lib.SIGNATURES
    assert len(sig) == len(header_symbols()) == 127
    # spot checks of the long ones the last feature pull requests added
    assert len(sig['occ4d_implicit_loss_terms_f32'][1]) == 19 and len(sig['occ4d_adamw_clip_groups_f32'][1]) == 14
    assert sig['occ4d_linear_f32'][1] == [ctypes.POINTER(pk._lib.LinearArgs), ctypes.c_void_p]
    assert sig['occ4d_posenc_f32'][1][5] is ctypes.c_double and sig['occ4d_fps_coop_debug'][1] == [ctypes.c_uint, ctypes.c_int]


def test_twin_stub_for_a_missing_symbol():
    class Handle:                                  # a library that exports nothing
        pass
    h = pk._lib.bind(Handle(), missing=pk._lib._not_in_twin)
    with pytest.raises(NotImplementedError, match='occ4d_knn_f32 is not part of the CPU twin'):
        h.occ4d_knn_f32()
    with pytest.raises(pk._lib.NativeLibraryError, match='stale: symbol occ4d_'):
        pk._lib.bind(Handle())
