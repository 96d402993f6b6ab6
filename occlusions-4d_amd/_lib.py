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
# Every header beside occ4d.h (whose symbol set and ABI_VERSION stay as they are), in the order they are read: (attribute prefix,
# path under include/, group, parsed with occ4d.h's structs).  Same conventions, same parser, same two libraries.  The loader below
# makes <PREFIX>_HEADER_PATH, <PREFIX>_SIGNATURES and <PREFIX>_CONSTANTS (the header's `#define OCC4D_<PREFIX>_*` without that prefix)
# from each row and adds its symbols to its group's table; a new header is a new row.
HEADERS = (
    ('FRONTEND', 'occ4d_frontend.h', 'feature', False),     # the clip front end (frontend.py)
    ('EVAL', 'occ4d_eval.h', 'feature', False),             # the evaluation statistics (evaluation.EvalStats); the constants: the layout of the two arrays
    ('OCCL', 'occ4d_occl.h', 'feature', False),             # the id histogram behind the live occlusion fractions (occlusion.py); the bin limit, the extra bins
    ('TRACK', 'occ4d_track.h', 'feature', False),           # the running merge of the per-instance reruns (inference.perform_inference, track_mode 'all')
    ('PROJECT', 'occ4d_project.h', 'feature', False),       # the camera projection, the z-buffer and the visibility test (projection.py)
    ('INST', 'occ4d_inst.h', 'feature', False),             # the instance statistics (evaluation.InstanceStats): the layout of the frame table and the two arrays
    ('REFINE', 'occ4d_refine.h', 'feature', False),         # the coarse-to-fine decode of the query grid (inference.perform_inference(refine=...))
    ('SURFACE', 'occ4d_surface.h', 'feature', False),       # the occupancy surface as a quad mesh (surface.py, inference.perform_inference(surface=...))
    ('RAYCAST', 'ext/occ4d_raycast.h', 'extension', False),         # the decoded field ray-cast into camera views (projection.render_field, perform_inference(views=...))
    ('PRELUDE', 'ext/occ4d_prelude.h', 'struct_extension', True),   # the decoder's query prelude (inference.QueryPrelude, LocalPclResnetFC.query_prelude); no constants
    ('COMPONENTS', 'ext/occ4d_components.h', 'addon', True),    # the connected components of the solid set (components.py, perform_inference(components=...))
    ('LINK', 'ext/occ4d_link.h', 'addon', True),                # the components of two frames linked: overlaps, tracks (components.Tracker, perform_inference(tracker=...))
    ('DISTANCE', 'ext/occ4d_distance.h', 'addon', True),        # the distance transform of the solid set: clearance (distance.py, perform_inference(clearance=...))
    ('GEODESIC', 'ext/occ4d_geodesic.h', 'addon', True),        # shortest free-space paths over the clearance (geodesic.py, perform_inference(route=...))
    ('WATERSHED', 'ext/occ4d_watershed.h', 'addon', True),      # touching objects split at their necks: watershed segments (watershed.py, perform_inference(segments=...))
    ('SIGHT', 'ext/occ4d_sight.h', 'addon', True),              # line of sight through the solid set: seen, hidden, by what (sight.py, perform_inference(sight=...))
    ('PULL', 'ext/occ4d_pull.h', 'addon', True),                # straight free legs: pairwise line of sight over the clearance, routes pulled into waypoints (geodesic.straight, geodesic.pull, Route(pull=True))
    ('VIEWPLAN', 'ext/occ4d_viewplan.h', 'addon', True),        # the next best view: which unseen points each candidate viewpoint reveals, a greedy set of them (sight.plan, perform_inference(next_view=...))
    ('BOXES', 'ext/occ4d_boxes.h', 'addon', True),              # upright oriented boxes of the labelled objects: extents over a table of headings, the least rectangle (components.Boxes, perform_inference(boxes=...))
    ('LINZ', 'ext/occ4d_linz.h', 'addon', True),                # the decoder's lin_z terms inside the trunk kernels (ops.rowlin(interp2=...), ops.resblock(addrows=...)); the opt-out bit
    ('LAYERS', 'ext/occ4d_layers.h', 'addon', True),            # the labelled objects as depth layers in camera views: amodal and visible masks, occlusion order (projection.ObjectLayers, perform_inference(layers=...))
    ('CHAIN', 'ext/occ4d_chain.h', 'addon', True),              # consecutive residual blocks of the decoder trunk as one launch, their lin_z terms in one pass (ops.resblock_chain, ops.interp_dense); the opt-out bit
    ('SWEEP', 'ext/occ4d_sweep.h', 'addon', True),              # the decoded field scanned by a virtual lidar: ranges, incidence, class and object per ray, rows in the loader's format (sweep.FieldSweep, perform_inference(sweep=...))
    ('EVIDENCE', 'ext/occ4d_evidence.h', 'addon', True),        # measured returns carved into the grid: hits, passed cells, the six codes of prediction against evidence (evidence.Evidence, perform_inference(evidence=...))
)
# prefix -> file, per group
FEATURE_HEADERS, EXTENSION_HEADERS, STRUCT_EXTENSION_HEADERS, ADDON_HEADERS = (
    {prefix: name for prefix, name, group, _ in HEADERS if group == g} for g in ('feature', 'extension', 'struct_extension', 'addon'))


class NativeLibraryError(RuntimeError):
    pass


def _strip_comments(text):
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def parse_constants(text, header='include/occ4d.h'):
    """{'ABI_VERSION': 5, 'PATH_TRUNK4': 16, ...}: every `#define OCC4D_<NAME> <integer>` of the header text (the value may
    stand in parentheses).  A define with any other value raises; one without a value (the include guard) is none.  `header`
    names the file in the error."""
    out = {}
    for name, value in re.findall(r'^[ \t]*#[ \t]*define[ \t]+OCC4D_(\w+)[ \t]+(\S.*?)[ \t]*$', _strip_comments(text), flags=re.M):
        m = re.fullmatch(r'\(\s*(-?\d+)\s*\)|(-?\d+)', value)
        if not m:
            raise NativeLibraryError('%s: cannot parse `#define OCC4D_%s %s` as an integer' % (header, name, value))
        out[name] = int(m.group(1) or m.group(2))
    return out


_SCALARS = {'int': C.c_int, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'unsigned': C.c_uint, 'float': C.c_float,
            'double': C.c_double}
_POINTEES = set(_SCALARS) | {'void', 'unsigned long long', 'uint32_t'}
_NOT_A_NAME = {'const', 'unsigned', 'signed', 'long', 'short', 'char', 'int', 'float', 'double', 'void', 'struct'}


def _ctype(decl, structs, what, is_return=False, header='include/occ4d.h'):
    """ctypes type of one parameter (or of the return type) `decl`; `what` names the declaration and `header` the file in the error."""
    m = re.fullmatch(r'(?:const\s+)?(unsigned long long|\w+)\s*(\*?)\s*(\w*)', ' '.join(decl.split()))
    if not m or m.group(3) in _NOT_A_NAME or (is_return and m.group(3)):
        raise NativeLibraryError('%s: cannot parse `%s` in %s' % (header, decl.strip(), what))
    base, star = m.group(1), m.group(2)
    if not star and base in _SCALARS:
        return _SCALARS[base]
    if star and base in structs:
        return C.POINTER(structs[base])
    if star and is_return and base == 'char':
        return C.c_char_p
    if star and base in _POINTEES:
        return C.c_void_p           # device or host: the header cannot tell, and c_void_p takes an address, byref() and arrays
    raise NativeLibraryError('%s: unknown type `%s` in %s' % (header, decl.strip(), what))


def parse_prototypes(text, structs, header='include/occ4d.h'):
    """name -> (restype, [argtypes]) of every `<type> occ4d_<name>(<parameters>);` of the header text.  `structs`: C struct name
    -> ctypes.Structure for the struct pointers.  Strict: once comments, preprocessor lines, the extern "C" braces and the
    typedef struct bodies are gone, EVERYTHING left must be such a prototype with known types; else NativeLibraryError, which
    names the file as `header`."""
    text = re.sub(r'^[ \t]*#.*$', '', _strip_comments(text), flags=re.M)
    text = re.sub(r'typedef\s+struct\b[^{};]*\{[^{}]*\}\s*\w+\s*;', '', text)
    text = re.sub(r'extern\s+"C"\s*\{|^[ \t]*\}[ \t]*$', '', text, flags=re.M)
    *decls, rest = text.split(';')
    if rest.strip():
        raise NativeLibraryError('%s: declaration without `;`: `%s`' % (header, ' '.join(rest.split())[:120]))
    out = {}
    for decl in decls:
        what = '`%s`' % ' '.join(decl.split())[:120]
        m = re.fullmatch(r'\s*([\w\s*]+?)\s*\b(occ4d_\w+)\s*\(([^()]*)\)\s*', decl)
        if not m or m.group(2) in out:
            raise NativeLibraryError('%s: cannot parse the declaration %s' % (header, what))
        params = [] if m.group(3).strip() == 'void' else m.group(3).split(',')
        out[m.group(2)] = (_ctype(m.group(1), structs, what, is_return=True, header=header),
                           [_ctype(p, structs, what, header=header) for p in params])
    return out


def _read_header(path, header='include/occ4d.h'):
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise NativeLibraryError('%s not found at %s (%s): the ctypes binding is derived from it' % (header, path, e))


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

# ... and every symbol the other headers declare, in the table of the header's group (ALL_SIGNATURES: occ4d.h and the feature
# headers) and in _EVERY_SIGNATURE, which bind() covers; two headers that declare the same symbol, or two rows of one prefix, are
# an error
ALL_SIGNATURES, EXTENSION_SIGNATURES, STRUCT_EXTENSION_SIGNATURES, ADDON_SIGNATURES = dict(SIGNATURES), {}, {}, {}
_GROUP_SIGNATURES = {'feature': ALL_SIGNATURES, 'extension': EXTENSION_SIGNATURES, 'struct_extension': STRUCT_EXTENSION_SIGNATURES,
                     'addon': ADDON_SIGNATURES}
_EVERY_SIGNATURE, _prefixes = dict(SIGNATURES), set()
for _prefix, _name, _group, _with_structs in HEADERS:
    _path = os.path.join(INCLUDE, *_name.split('/'))
    _text = _read_header(_path, 'include/' + _name)
    _table = parse_prototypes(_text, _STRUCTS if _with_structs else {}, 'include/' + _name)
    _twice = sorted(set(_table) & set(_EVERY_SIGNATURE))
    if _twice or _prefix in _prefixes:
        raise NativeLibraryError('include/%s declares %s, which another header declares too' % (_name, ', '.join(_twice) or _prefix))
    _EVERY_SIGNATURE.update(_table)
    _prefixes.add(_prefix)
    _GROUP_SIGNATURES[_group].update(_table)
    globals().update({_prefix + '_HEADER_PATH': _path, _prefix + '_SIGNATURES': _table})
    if _group != 'struct_extension':            # (the prelude's header defines no constants and publishes no table of them)
        globals()[_prefix + '_CONSTANTS'] = {k[len(_prefix) + 1:]: v for k, v in parse_constants(_text, 'include/' + _name).items()}

_lib = None
_twin = False            # True only after an explicit load_cpu_twin(): host pointers, no streams (cpu_twin.py)


def is_twin():
    return _twin


def bind(handle, missing=None):
    """Sets restype / argtypes of every symbol of every header on a loaded library and returns it.  A symbol the library does not
    export is a stale library (NativeLibraryError) unless `missing` is given: then missing(name) stands in for it."""
    for name, (res, args) in _EVERY_SIGNATURE.items():
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
