"""ctypes binding of libocc4d.so.  The argument types of every entry point and the integer constants are DERIVED from
include/occ4d.h when this module is imported (parse_constants / parse_prototypes below): the header is the one place
where the C ABI is written down; only the four struct layouts are restated here.  Fails loudly when the header or the
library is missing or stale: the product has no CPU / PyTorch fallback path."""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libocc4d.so')
INCLUDE = os.path.join(os.path.dirname(_HERE), 'include')
HEADER_PATH = os.path.join(INCLUDE, 'occ4d.h')
# The feature headers beside occ4d.h (whose symbol set and ABI_VERSION stay as they are): attribute prefix -> file.  Same
# conventions, same parser, same two libraries.  <PREFIX>_HEADER_PATH, <PREFIX>_SIGNATURES and <PREFIX>_CONSTANTS (the header's
# `#define OCC4D_<PREFIX>_*` without that prefix) are made from this table below; a new header is a new row here.
FEATURE_HEADERS = {
    'FRONTEND': 'occ4d_frontend.h',     # the clip front end (frontend.py)
    'EVAL': 'occ4d_eval.h',             # the evaluation statistics (evaluation.EvalStats); the constants: the layout of the two arrays
    'OCCL': 'occ4d_occl.h',             # the id histogram behind the live occlusion fractions (occlusion.py); the bin limit, the extra bins
    'TRACK': 'occ4d_track.h',           # the running merge of the per-instance reruns (inference.perform_inference, track_mode 'all')
    'PROJECT': 'occ4d_project.h',       # the camera projection, the z-buffer and the visibility test (projection.py)
    'INST': 'occ4d_inst.h',             # the instance statistics (evaluation.InstanceStats): the layout of the frame table and the two arrays
    'REFINE': 'occ4d_refine.h',         # the coarse-to-fine decode of the query grid (inference.perform_inference(refine=...))
    'SURFACE': 'occ4d_surface.h',       # the occupancy surface as a quad mesh (surface.py, inference.perform_inference(surface=...))
}
# FEATURE_HEADERS is a closed list: the suite pins it as the occ4d*.h files of include/ itself, its number of rows, and
# ALL_SIGNATURES as the sum of its tables.  Headers that came after it live in include/ext/ and are rows here: the same
# conventions, the same parser, the same two libraries, the same <PREFIX>_HEADER_PATH / _SIGNATURES / _CONSTANTS attributes; their
# symbols are EXTENSION_SIGNATURES, which bind() covers beside ALL_SIGNATURES.
EXTENSION_HEADERS = {
    'RAYCAST': 'ext/occ4d_raycast.h',   # the decoded field ray-cast into camera views (projection.render_field, perform_inference(views=...))
}
# EXTENSION_SIGNATURES is pinned by the suite as well (as the ray-cast's table).  Headers of include/ext/ whose prototypes take the
# structs of occ4d.h are rows here: parsed with those structs, <PREFIX>_HEADER_PATH / _SIGNATURES attributes as above, their symbols
# in STRUCT_EXTENSION_SIGNATURES, which bind() covers too.
STRUCT_EXTENSION_HEADERS = {
    'PRELUDE': 'ext/occ4d_prelude.h',   # the decoder's query prelude (inference.QueryPrelude, LocalPclResnetFC.query_prelude)
}
# The three tables above are pinned by the suite row for row.  ADDON_HEADERS is OPEN BY DESIGN: every later header of include/ext/
# is a row here (parsed with occ4d.h's structs, so a prototype may use them or not): the same <PREFIX>_HEADER_PATH / _SIGNATURES /
# _CONSTANTS attributes, its symbols in ADDON_SIGNATURES, which bind() covers too.  A test of a header checks that its symbols are
# IN the table and in none of the other three, never that the table equals them.
ADDON_HEADERS = {
    'COMPONENTS': 'ext/occ4d_components.h',     # the connected components of the solid set (components.py, perform_inference(components=...))
    'LINK': 'ext/occ4d_link.h',                 # the components of two frames linked: overlaps, tracks (components.Tracker, perform_inference(tracker=...))
    'DISTANCE': 'ext/occ4d_distance.h',         # the distance transform of the solid set: clearance (distance.py, perform_inference(clearance=...))
    'GEODESIC': 'ext/occ4d_geodesic.h',         # shortest free-space paths over the clearance (geodesic.py, perform_inference(route=...))
    'WATERSHED': 'ext/occ4d_watershed.h',       # touching objects split at their necks: watershed segments (watershed.py, perform_inference(segments=...))
    'SIGHT': 'ext/occ4d_sight.h',               # line of sight through the solid set: seen, hidden, by what (sight.py, perform_inference(sight=...))
    'PULL': 'ext/occ4d_pull.h',                 # straight free legs: pairwise line of sight over the clearance, routes pulled into waypoints (geodesic.straight, geodesic.pull, Route(pull=True))
    'VIEWPLAN': 'ext/occ4d_viewplan.h',         # the next best view: which unseen points each candidate viewpoint reveals, a greedy set of them (sight.plan, perform_inference(next_view=...))
    'BOXES': 'ext/occ4d_boxes.h',               # upright oriented boxes of the labelled objects: extents over a table of headings, the least rectangle (components.Boxes, perform_inference(boxes=...))
    'LINZ': 'ext/occ4d_linz.h',                 # the decoder's lin_z terms inside the trunk kernels (ops.rowlin(interp2=...), ops.resblock(addrows=...)); the opt-out bit
    'LAYERS': 'ext/occ4d_layers.h',             # the labelled objects as depth layers in camera views: amodal and visible masks, occlusion order (projection.ObjectLayers, perform_inference(layers=...))
    'CHAIN': 'ext/occ4d_chain.h',               # consecutive residual blocks of the decoder trunk as one launch, their lin_z terms in one pass (ops.resblock_chain, ops.interp_dense); the opt-out bit
}


class NativeLibraryError(RuntimeError):
    pass


def _strip_comments(text):
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def parse_constants(text):
    """{'ABI_VERSION': 5, 'PATH_TRUNK4': 16, ...}: every `#define OCC4D_<NAME> <integer>` of the header text (the value may
    stand in parentheses).  A define with any other value raises; one without a value (the include guard) is none."""
    out = {}
    for name, value in re.findall(r'^[ \t]*#[ \t]*define[ \t]+OCC4D_(\w+)[ \t]+(\S.*?)[ \t]*$', _strip_comments(text), flags=re.M):
        m = re.fullmatch(r'\(\s*(-?\d+)\s*\)|(-?\d+)', value)
        if not m:
            raise NativeLibraryError('include/occ4d.h: cannot parse `#define OCC4D_%s %s` as an integer' % (name, value))
        out[name] = int(m.group(1) or m.group(2))
    return out


_SCALARS = {'int': C.c_int, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'unsigned': C.c_uint, 'float': C.c_float,
            'double': C.c_double}
_POINTEES = set(_SCALARS) | {'void', 'unsigned long long', 'uint32_t'}
_NOT_A_NAME = {'const', 'unsigned', 'signed', 'long', 'short', 'char', 'int', 'float', 'double', 'void', 'struct'}


def _ctype(decl, structs, what, is_return=False):
    """ctypes type of one parameter (or of the return type) `decl`; `what` names the declaration in the error."""
    m = re.fullmatch(r'(?:const\s+)?(unsigned long long|\w+)\s*(\*?)\s*(\w*)', ' '.join(decl.split()))
    if not m or m.group(3) in _NOT_A_NAME or (is_return and m.group(3)):
        raise NativeLibraryError('include/occ4d.h: cannot parse `%s` in %s' % (decl.strip(), what))
    base, star = m.group(1), m.group(2)
    if not star and base in _SCALARS:
        return _SCALARS[base]
    if star and base in structs:
        return C.POINTER(structs[base])
    if star and is_return and base == 'char':
        return C.c_char_p
    if star and base in _POINTEES:
        return C.c_void_p           # device or host: the header cannot tell, and c_void_p takes an address, byref() and arrays
    raise NativeLibraryError('include/occ4d.h: unknown type `%s` in %s' % (decl.strip(), what))


def parse_prototypes(text, structs):
    """name -> (restype, [argtypes]) of every `<type> occ4d_<name>(<parameters>);` of the header text.  `structs`: C struct name
    -> ctypes.Structure for the struct pointers.  Strict: once comments, preprocessor lines, the extern "C" braces and the
    typedef struct bodies are gone, EVERYTHING left must be such a prototype with known types; else NativeLibraryError."""
    text = re.sub(r'^[ \t]*#.*$', '', _strip_comments(text), flags=re.M)
    text = re.sub(r'typedef\s+struct\b[^{};]*\{[^{}]*\}\s*\w+\s*;', '', text)
    text = re.sub(r'extern\s+"C"\s*\{|^[ \t]*\}[ \t]*$', '', text, flags=re.M)
    *decls, rest = text.split(';')
    if rest.strip():
        raise NativeLibraryError('include/occ4d.h: declaration without `;`: `%s`' % ' '.join(rest.split())[:120])
    out = {}
    for decl in decls:
        what = '`%s`' % ' '.join(decl.split())[:120]
        m = re.fullmatch(r'\s*([\w\s*]+?)\s*\b(occ4d_\w+)\s*\(([^()]*)\)\s*', decl)
        if not m or m.group(2) in out:
            raise NativeLibraryError('include/occ4d.h: cannot parse the declaration %s' % what)
        params = [] if m.group(3).strip() == 'void' else m.group(3).split(',')
        out[m.group(2)] = (_ctype(m.group(1), structs, what, is_return=True), [_ctype(p, structs, what) for p in params])
    return out


def _read_header(path):
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise NativeLibraryError('include/%s not found at %s (%s): the ctypes binding is derived from it'
                                 % (os.path.basename(path), path, e))


_HEADER = _read_header(HEADER_PATH)

# ABI_VERSION, OK / EINVAL / ELAUNCH, PATH_*, PROFILE_*, MAX_BLOCKS, MAX_CROSS: the header's `#define OCC4D_*` become module
# attributes of the same name without the prefix (tests/test_abi.py pins their values)
CONSTANTS = parse_constants(_HEADER)
globals().update(CONSTANTS)
ABI_VERSION, OK, EINVAL, ELAUNCH = (CONSTANTS[k] for k in ('ABI_VERSION', 'OK', 'EINVAL', 'ELAUNCH'))
MAX_BLOCKS, MAX_CROSS = CONSTANTS['MAX_BLOCKS'], CONSTANTS['MAX_CROSS']
PROFILE_KINDS = {'cross_attn': CONSTANTS['PROFILE_CROSS_ATTN'], 'resblock': CONSTANTS['PROFILE_RESBLOCK'],
                 'rowlin': CONSTANTS['PROFILE_ROWLIN']}


class LinearArgs(C.Structure):
    """occ4d_linear_args (include/occ4d.h)."""
    _fields_ = [
        ('x', C.c_void_p), ('ldx', C.c_int64),
        ('w', C.c_void_p), ('ldw', C.c_int64),
        ('bias', C.c_void_p),
        ('residual', C.c_void_p), ('ldr', C.c_int64),
        ('y', C.c_void_p), ('ldy', C.c_int64),
        ('M', C.c_int32), ('K', C.c_int32), ('N', C.c_int32),
        ('relu_in', C.c_int32), ('relu_out', C.c_int32),
        ('add_rows', C.c_void_p), ('ld_add', C.c_int64), ('add_div', C.c_int32),
        ('sub_rows', C.c_void_p), ('ld_sub', C.c_int64), ('sub_idx', C.c_void_p),
    ]


class PtLayerWeights(C.Structure):
    """occ4d_pt_layer_weights (include/occ4d.h)."""
    _fields_ = [(n, C.c_int32) for n in ('dim', 'dim2', 'pos_hidden', 'cross', 'd_in', 'd_out', 'reserved0', 'reserved1')] + \
               [(n, C.c_void_p) for n in ('to_q', 'to_k', 'to_v', 'pos0_w', 'pos0_b', 'pos2_w', 'pos2_b', 'attn0_w',
                                          'attn0_b', 'attn2_w', 'attn2_b', 'pre_w', 'pre_b', 'post_w', 'post_b')]


class LaunchEvents(C.Structure):
    """occ4d_launch_events (include/occ4d.h)."""
    _fields_ = [('events', C.POINTER(C.c_void_p)), ('capacity', C.c_int32), ('used', C.c_int32), ('kernel', C.c_int32),
                ('reserved', C.c_int32)]


class DecoderWeights(C.Structure):
    """occ4d_decoder_weights (include/occ4d.h)."""
    _fields_ = [(n, C.c_int32) for n in ('d_in', 'n_freq', 'd_hidden', 'd_out', 'd_latent', 'd_latent_local', 'n_blocks',
                                         'n_cross', 'k_local', 'k_cross', 'activation', 'lin_in_ld')] + \
               [('base_frequency', C.c_float), ('reserved', C.c_float)] + \
               [(n, C.c_void_p) for n in ('lin_in_w', 'lin_in_b', 'lin_out_w', 'lin_out_b')] + \
               [(n, C.c_void_p * MAX_BLOCKS) for n in ('lin_z_w', 'lin_z_b', 'fc0_w', 'fc0_b', 'fc1_w', 'fc1_b')] + \
               [('cross_after', C.c_int32 * MAX_CROSS), ('cross', PtLayerWeights * MAX_CROSS)]


# name -> (restype, argtypes): every symbol include/occ4d.h declares
_STRUCTS = {'occ4d_linear_args': LinearArgs, 'occ4d_pt_layer_weights': PtLayerWeights, 'occ4d_launch_events': LaunchEvents,
            'occ4d_decoder_weights': DecoderWeights}
SIGNATURES = parse_prototypes(_HEADER, _STRUCTS)

# ... and every symbol any header declares; two headers that declare the same one are an error
ALL_SIGNATURES = dict(SIGNATURES)
for _prefix, _name in FEATURE_HEADERS.items():
    _path = os.path.join(INCLUDE, _name)
    _text = _read_header(_path)
    _table = parse_prototypes(_text, {})
    _twice = sorted(set(_table) & set(ALL_SIGNATURES))
    if _twice:
        raise NativeLibraryError('include/%s declares %s, which another header declares too' % (_name, ', '.join(_twice)))
    ALL_SIGNATURES.update(_table)
    globals().update({_prefix + '_HEADER_PATH': _path, _prefix + '_SIGNATURES': _table,
                      _prefix + '_CONSTANTS': {k[len(_prefix) + 1:]: v for k, v in parse_constants(_text).items()}})

# ... and the extension headers' symbols, in a table of their own
EXTENSION_SIGNATURES = {}
for _prefix, _name in EXTENSION_HEADERS.items():
    _path = os.path.join(INCLUDE, *_name.split('/'))
    _text = _read_header(_path)
    _table = parse_prototypes(_text, {})
    _twice = sorted(set(_table) & (set(ALL_SIGNATURES) | set(EXTENSION_SIGNATURES)))
    if _twice or _prefix in FEATURE_HEADERS:
        raise NativeLibraryError('include/%s declares %s, which another header declares too' % (_name, ', '.join(_twice) or _prefix))
    EXTENSION_SIGNATURES.update(_table)
    globals().update({_prefix + '_HEADER_PATH': _path, _prefix + '_SIGNATURES': _table,
                      _prefix + '_CONSTANTS': {k[len(_prefix) + 1:]: v for k, v in parse_constants(_text).items()}})

# ... and those of the extension headers that use occ4d.h's structs
STRUCT_EXTENSION_SIGNATURES = {}
for _prefix, _name in STRUCT_EXTENSION_HEADERS.items():
    _path = os.path.join(INCLUDE, *_name.split('/'))
    _table = parse_prototypes(_read_header(_path), _STRUCTS)
    _twice = sorted(set(_table) & (set(ALL_SIGNATURES) | set(EXTENSION_SIGNATURES) | set(STRUCT_EXTENSION_SIGNATURES)))
    if _twice or _prefix in FEATURE_HEADERS or _prefix in EXTENSION_HEADERS:
        raise NativeLibraryError('include/%s declares %s, which another header declares too' % (_name, ', '.join(_twice) or _prefix))
    STRUCT_EXTENSION_SIGNATURES.update(_table)
    globals().update({_prefix + '_HEADER_PATH': _path, _prefix + '_SIGNATURES': _table})

# ... and the open table
ADDON_SIGNATURES = {}
for _prefix, _name in ADDON_HEADERS.items():
    _path = os.path.join(INCLUDE, *_name.split('/'))
    _text = _read_header(_path)
    _table = parse_prototypes(_text, _STRUCTS)
    _twice = sorted(set(_table) & (set(ALL_SIGNATURES) | set(EXTENSION_SIGNATURES) | set(STRUCT_EXTENSION_SIGNATURES) | set(ADDON_SIGNATURES)))
    if _twice or _prefix in FEATURE_HEADERS or _prefix in EXTENSION_HEADERS or _prefix in STRUCT_EXTENSION_HEADERS:
        raise NativeLibraryError('include/%s declares %s, which another header declares too' % (_name, ', '.join(_twice) or _prefix))
    ADDON_SIGNATURES.update(_table)
    globals().update({_prefix + '_HEADER_PATH': _path, _prefix + '_SIGNATURES': _table,
                      _prefix + '_CONSTANTS': {k[len(_prefix) + 1:]: v for k, v in parse_constants(_text).items()}})

_lib = None
_twin = False            # True only after an explicit load_cpu_twin(): host pointers, no streams (cpu_twin.py)


def is_twin():
    return _twin


def bind(handle, missing=None):
    """Sets restype / argtypes of every symbol of ALL_SIGNATURES, the two extension tables and ADDON_SIGNATURES on a loaded library and returns it.  A symbol the library does
    not export is a stale library (NativeLibraryError) unless `missing` is given: then missing(name) stands in for it."""
    for name, (res, args) in (list(ALL_SIGNATURES.items()) + list(EXTENSION_SIGNATURES.items())
                              + list(STRUCT_EXTENSION_SIGNATURES.items()) + list(ADDON_SIGNATURES.items())):
        try:
            fn = getattr(handle, name)
        except AttributeError:
            if missing is None:
                raise NativeLibraryError('libocc4d.so is stale: symbol %s missing; rebuild it' % name)
            setattr(handle, name, missing(name))
            continue
        fn.restype = res
        fn.argtypes = args
    return handle


def _not_in_twin(name):
    def stub(*_a, **_k):
        raise NotImplementedError('%s is not part of the CPU twin (libocc4d_cpu.so holds the inference path only)' % name)
    return stub


def load_cpu_twin(path):
    """Replaces the process's library handle by the g++ twin at `path`.  Only cpu_twin.enable() calls this; nothing in
    the package does so on its own (no fallback: without this call a missing libocc4d.so raises NativeLibraryError).
    An entry point the twin does not have raises NotImplementedError when CALLED (the HIP library, in contrast, must
    export every symbol of the header)."""
    global _lib, _twin
    twin = bind(C.CDLL(path), missing=_not_in_twin)
    if twin.occ4d_abi_version() != ABI_VERSION or twin.occ4d_is_cpu_twin() != 1:
        raise NativeLibraryError('%s is not the CPU twin of ABI version %d' % (path, ABI_VERSION))
    _lib, _twin = twin, True
    return twin


def unload_cpu_twin():
    global _lib, _twin
    _lib, _twin = None, False


def lib():
    """The loaded library (cached).  Raises NativeLibraryError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            'libocc4d.so not found at %s -- build it with `python occlusions-4d_amd/build.py` '
            '(or __graft_entry__.build()); this package has no CPU/PyTorch fallback.' % LIB_PATH)
    handle = bind(C.CDLL(LIB_PATH))
    if handle.occ4d_abi_version() != ABI_VERSION:
        raise NativeLibraryError('libocc4d.so ABI version %d != expected %d; rebuild it'
                                 % (handle.occ4d_abi_version(), ABI_VERSION))
    _lib = handle
    return _lib


def check(rc):
    """Map a status code to the exception the reference would have raised
    (AssertionError for shape/argument violations)."""
    if rc == OK:
        return
    msg = lib().occ4d_last_error().decode('utf-8', 'replace')
    if rc == EINVAL:
        raise AssertionError(msg)
    raise RuntimeError('libocc4d launch failure: ' + msg)
