"""ctypes binding of librelpose_hip.so, derived from include/relpose_hip.h.

The header is the one definition of the C ABI: the structures, the RP_* constants and every entry point's
argument and return types are parsed from it at import -- nothing is restated here.  The parser is written for
that header, not for C, and raises on any text it does not recognise.  load() gives every entry point that
launches work (int return, `void* stream` last) an errcheck, so a non-zero status raises at the call.

PyTorch is only plumbing here: it owns device memory and the HIP stream; every hot-path op goes through this
C ABI.  There is NO fallback: a missing library or a non-zero return code raises."""
import ctypes
import keyword
import os
import re
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_longlong, c_size_t, c_void_p

import torch  # noqa: F401  (must be imported first: it loads the HIP runtime this library binds to)

from . import _build

_LIB = None
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "relpose_hip.h")

_SCALARS = {"int": c_int, "float": c_float, "long long": c_longlong, "size_t": c_size_t}
_POINTEES = ("void", "float", "double", "int", "unsigned char")        # data pointers: all passed as c_void_p
_DEFINE = re.compile(r"#\s*define\s+(RP_\w+)\s+(-?\d+|\(-?\d+\))")
_DECL = re.compile(r"(const\s+)?(unsigned\s+char|long\s+long|\w+)\s*(\*?)\s*([A-Za-z_]\w*(?:\s*,\s*[A-Za-z_]\w*)*)?")
_ITEM = re.compile(r"\s*(?:typedef\s+struct\s+(\w+)\s*\{([^{}]*);\s*\}\s*(\w+)\s*;"      # 1-3: a structure
                   r"|([\w\s*]+?)\b(rp_\w+)\s*\(([^()]*)\)\s*;"                         # 4-6: a prototype
                   r'|extern\s+"C"\s*\{|\})')


def _declaration(text, structs, header="relpose_hip.h"):
    """(ctypes type, [names]) of `type name`, `type a, b, c` or a bare `type`, as the header writes them."""
    m = _DECL.fullmatch(text.strip())
    if not m:
        raise ValueError("%s: cannot parse declaration %r" % (header, text.strip()))
    const, base, star, names = m.groups()
    base, names = " ".join(base.split()), re.split(r"\s*,\s*", names) if names else []
    if star and base in structs and len(names) <= 1:
        return POINTER(structs[base]), names
    if star and base in _POINTEES and len(names) <= 1:
        return c_void_p, names
    if not star and not const and base in _SCALARS:
        return _SCALARS[base], names
    raise ValueError("%s: unknown type in %r" % (header, text.strip()))


def _header_contract(text, header="relpose_hip.h"):
    """(RP_* constants, structures, prototypes, status names) read from the text of include/<header> -- the single definition
    the library is compiled against and this binding is made from.  prototypes: name -> (restype, argtypes), in header order;
    status names: the entry points whose last parameter is `void* stream` -- they enqueue work and return 0 / RP_E* / hipError_t,
    every other int is a count.  Anything the header does not use today (arrays, function pointers, other types) raises."""
    consts, structs, sigs, status = {}, {}, {}, set()
    lines = re.sub(r"/\*.*?\*/", " ", text, flags=re.S).split("\n")
    for i, line in enumerate(lines):
        if line.lstrip().startswith("#"):                    # preprocessor: only the RP_* constants matter
            m = _DEFINE.fullmatch(line.strip())
            if m:
                consts[m.group(1)] = int(m.group(2).strip("()"))
            elif re.match(r"\s*#\s*define\s+RP_", line):
                raise ValueError("%s: cannot parse %r" % (header, line.strip()))
            lines[i] = ""
    code, pos = "\n".join(lines).rstrip(), 0
    while pos < len(code):
        m = _ITEM.match(code, pos)
        if not m:
            raise ValueError("%s: cannot parse %r" % (header, code[pos:].strip()[:80]))
        pos = m.end()
        tag, body, alias, ret, name, params = m.groups()
        if tag:
            if tag != alias or tag in structs:
                raise ValueError("%s: cannot parse struct %s" % (header, tag))
            fields = []
            for decl in body.split(";"):
                ctype, names = _declaration(decl, structs, header)
                if not names:
                    raise ValueError("%s: field without a name in struct %s: %r" % (header, tag, decl.strip()))
                fields += [(n + "_" if keyword.iskeyword(n) else n, ctype) for n in names]
            structs[tag] = type(tag, (Structure,), {"_fields_": fields})
        elif name:
            ret, params = " ".join(ret.split()), [p.strip() for p in params.split(",")]
            args = [] if params == ["void"] else [_declaration(p, structs, header) for p in params]
            if name in sigs or any(len(names) != 1 for _, names in args):
                raise ValueError("%s: cannot parse prototype of %s" % (header, name))
            res = None if ret == "void" else c_char_p if ret == "const char*" else _declaration(ret, structs, header)[0]
            if re.fullmatch(r"void\s*\*\s*stream", params[-1]):
                if res is not c_int:
                    raise ValueError("%s: %s takes a stream but does not return int" % (header, name))
                status.add(name)
            sigs[name] = (res, [ctype for ctype, _ in args])
    return consts, structs, sigs, status


with open(HEADER) as _f:
    _CONSTS, _STRUCTS, _PROTOTYPES, _STATUS = _header_contract(_f.read())
ABI_VERSION, ABI_EXPORTS = _CONSTS["RP_ABI_VERSION"], _CONSTS["RP_ABI_EXPORTS"]
RP_COLSUM_MAX, RP_SPLITK_MAX, RP_TRANSPOSE_MAX = _CONSTS["RP_COLSUM_MAX"], _CONSTS["RP_SPLITK_MAX"], _CONSTS["RP_TRANSPOSE_MAX"]
_ERROR_TEXT = {"RP_EBADSHAPE": "bad shape", "RP_EALIGN": "misaligned pointer/stride", "RP_EWORKSPACE": "workspace too small",
               "RP_EUNSUPPORTED": "unsupported"}
RP_ERRORS = {code: _ERROR_TEXT[name] for name, code in _CONSTS.items() if name.startswith("RP_E")}   # KeyError: a code without a text
RpGemm, RpColsumTask, RpBnMask, RpSplitkTask, RpTransposeTask = (
    _STRUCTS[n] for n in ("RpGemm", "RpColsumTask", "RpBnMask", "RpSplitkTask", "RpTransposeTask"))
EXPORTS = tuple(_PROTOTYPES)
DECLARED = set(EXPORTS)


# the readout library (include/relpose_readout.h -> librelpose_readout.so): the same parser, the same errcheck, the RP_E* codes above
_READOUT_LIB = None
READOUT_HEADER = os.path.join(os.path.dirname(HEADER), "relpose_readout.h")
with open(READOUT_HEADER) as _f:
    _READOUT_CONSTS, _, _READOUT_PROTOTYPES, _READOUT_STATUS = _header_contract(_f.read(), "relpose_readout.h")
READOUT_ABI_VERSION = _READOUT_CONSTS["RP_READOUT_ABI_VERSION"]
READOUT_EXPORTS = tuple(_READOUT_PROTOTYPES)


# the eight-point library (include/relpose_eightpoint.h -> librelpose_eightpoint.so): again the same parser, errcheck and RP_E* codes
_EIGHTPOINT_LIB = None
EIGHTPOINT_HEADER = os.path.join(os.path.dirname(HEADER), "relpose_eightpoint.h")
with open(EIGHTPOINT_HEADER) as _f:
    _EIGHTPOINT_CONSTS, _, _EIGHTPOINT_PROTOTYPES, _EIGHTPOINT_STATUS = _header_contract(_f.read(), "relpose_eightpoint.h")
EIGHTPOINT_ABI_VERSION = _EIGHTPOINT_CONSTS["RP_EIGHTPOINT_ABI_VERSION"]
EIGHTPOINT_MAX_P, EIGHTPOINT_MAX_ITERS = _EIGHTPOINT_CONSTS["RP_EIGHTPOINT_MAX_P"], _EIGHTPOINT_CONSTS["RP_EIGHTPOINT_MAX_ITERS"]
EIGHTPOINT_EXPORTS = tuple(_EIGHTPOINT_PROTOTYPES)


# the refinement library (include/relpose_refine.h -> librelpose_refine.so): once more the same parser, errcheck and RP_E* codes
_REFINE_LIB = None
REFINE_HEADER = os.path.join(os.path.dirname(HEADER), "relpose_refine.h")
with open(REFINE_HEADER) as _f:
    _REFINE_CONSTS, _, _REFINE_PROTOTYPES, _REFINE_STATUS = _header_contract(_f.read(), "relpose_refine.h")
REFINE_ABI_VERSION = _REFINE_CONSTS["RP_REFINE_ABI_VERSION"]
REFINE_MAX_P, REFINE_MAX_ITERS = _REFINE_CONSTS["RP_REFINE_MAX_P"], _REFINE_CONSTS["RP_REFINE_MAX_ITERS"]
REFINE_EXPORTS = tuple(_REFINE_PROTOTYPES)


# the consensus library (include/relpose_consensus.h -> librelpose_consensus.so): the same parser, errcheck and RP_E* codes a fifth time
_CONSENSUS_LIB = None
CONSENSUS_HEADER = os.path.join(os.path.dirname(HEADER), "relpose_consensus.h")
with open(CONSENSUS_HEADER) as _f:
    _CONSENSUS_CONSTS, _, _CONSENSUS_PROTOTYPES, _CONSENSUS_STATUS = _header_contract(_f.read(), "relpose_consensus.h")
CONSENSUS_ABI_VERSION = _CONSENSUS_CONSTS["RP_CONSENSUS_ABI_VERSION"]
CONSENSUS_MAX_P, CONSENSUS_MAX_M = _CONSENSUS_CONSTS["RP_CONSENSUS_MAX_P"], _CONSENSUS_CONSTS["RP_CONSENSUS_MAX_M"]
CONSENSUS_EXPORTS = tuple(_CONSENSUS_PROTOTYPES)


# the sub-token localisation library (include/relpose_submatch.h -> librelpose_submatch.so): the same parser, errcheck and RP_E* codes a sixth time
_SUBMATCH_LIB = None
SUBMATCH_HEADER = os.path.join(os.path.dirname(HEADER), "relpose_submatch.h")
with open(SUBMATCH_HEADER) as _f:
    _SUBMATCH_CONSTS, _, _SUBMATCH_PROTOTYPES, _SUBMATCH_STATUS = _header_contract(_f.read(), "relpose_submatch.h")
SUBMATCH_ABI_VERSION = _SUBMATCH_CONSTS["RP_SUBMATCH_ABI_VERSION"]
SUBMATCH_EXPORTS = tuple(_SUBMATCH_PROTOTYPES)


# the five-point consensus library (include/relpose_fivepoint.h -> librelpose_fivepoint.so): the same parser, errcheck and RP_E* codes a seventh time
_FIVEPOINT_LIB = None
FIVEPOINT_HEADER = os.path.join(os.path.dirname(HEADER), "relpose_fivepoint.h")
with open(FIVEPOINT_HEADER) as _f:
    _FIVEPOINT_CONSTS, _, _FIVEPOINT_PROTOTYPES, _FIVEPOINT_STATUS = _header_contract(_f.read(), "relpose_fivepoint.h")
FIVEPOINT_ABI_VERSION = _FIVEPOINT_CONSTS["RP_FIVEPOINT_ABI_VERSION"]
FIVEPOINT_MAX_P, FIVEPOINT_MAX_M, FIVEPOINT_ROOTS = (_FIVEPOINT_CONSTS[k] for k in ("RP_FIVEPOINT_MAX_P", "RP_FIVEPOINT_MAX_M", "RP_FIVEPOINT_ROOTS"))
FIVEPOINT_EXPORTS = tuple(_FIVEPOINT_PROTOTYPES)


# the homography library (include/relpose_homography.h -> librelpose_homography.so): the same parser, errcheck and RP_E* codes an eighth time
_HOMOGRAPHY_LIB = None
HOMOGRAPHY_HEADER = os.path.join(os.path.dirname(HEADER), "relpose_homography.h")
with open(HOMOGRAPHY_HEADER) as _f:
    _HOMOGRAPHY_CONSTS, _, _HOMOGRAPHY_PROTOTYPES, _HOMOGRAPHY_STATUS = _header_contract(_f.read(), "relpose_homography.h")
HOMOGRAPHY_ABI_VERSION = _HOMOGRAPHY_CONSTS["RP_HOMOGRAPHY_ABI_VERSION"]
HOMOGRAPHY_MAX_P, HOMOGRAPHY_MAX_M, HOMOGRAPHY_MAX_ITERS = (_HOMOGRAPHY_CONSTS[k] for k in ("RP_HOMOGRAPHY_MAX_P", "RP_HOMOGRAPHY_MAX_M", "RP_HOMOGRAPHY_MAX_ITERS"))
HOMOGRAPHY_EXPORTS = tuple(_HOMOGRAPHY_PROTOTYPES)


# the triangulation library (include/relpose_triangulate.h -> librelpose_triangulate.so): the same parser, errcheck and RP_E* codes a ninth time
_TRIANGULATE_LIB = None
TRIANGULATE_HEADER = os.path.join(os.path.dirname(HEADER), "relpose_triangulate.h")
with open(TRIANGULATE_HEADER) as _f:
    _TRIANGULATE_CONSTS, _, _TRIANGULATE_PROTOTYPES, _TRIANGULATE_STATUS = _header_contract(_f.read(), "relpose_triangulate.h")
TRIANGULATE_ABI_VERSION = _TRIANGULATE_CONSTS["RP_TRIANGULATE_ABI_VERSION"]
TRIANGULATE_MAX_P = _TRIANGULATE_CONSTS["RP_TRIANGULATE_MAX_P"]
TRIANGULATE_EXPORTS = tuple(_TRIANGULATE_PROTOTYPES)


# the 5x5 input-gradient library (include/relpose_conv5x5.h -> librelpose_conv5x5.so): the same parser, errcheck and RP_E* codes a tenth time
_CONV5X5_LIB = None
CONV5X5_HEADER = os.path.join(os.path.dirname(HEADER), "relpose_conv5x5.h")
with open(CONV5X5_HEADER) as _f:
    _CONV5X5_CONSTS, _, _CONV5X5_PROTOTYPES, _CONV5X5_STATUS = _header_contract(_f.read(), "relpose_conv5x5.h")
CONV5X5_ABI_VERSION = _CONV5X5_CONSTS["RP_CONV5X5_ABI_VERSION"]
CONV5X5_EXPORTS = tuple(_CONV5X5_PROTOTYPES)


# the guided-matching library (include/relpose_guided.h -> librelpose_guided.so): the same parser, errcheck and RP_E* codes an eleventh time
_GUIDED_LIB = None
GUIDED_HEADER = os.path.join(os.path.dirname(HEADER), "relpose_guided.h")
with open(GUIDED_HEADER) as _f:
    _GUIDED_CONSTS, _, _GUIDED_PROTOTYPES, _GUIDED_STATUS = _header_contract(_f.read(), "relpose_guided.h")
GUIDED_ABI_VERSION = _GUIDED_CONSTS["RP_GUIDED_ABI_VERSION"]
GUIDED_EXPORTS = tuple(_GUIDED_PROTOTYPES)


# the pure-rotation library (include/relpose_rotation.h -> librelpose_rotation.so): the same parser, errcheck and RP_E* codes a twelfth time
_ROTATION_LIB = None
ROTATION_HEADER = os.path.join(os.path.dirname(HEADER), "relpose_rotation.h")
with open(ROTATION_HEADER) as _f:
    _ROTATION_CONSTS, _, _ROTATION_PROTOTYPES, _ROTATION_STATUS = _header_contract(_f.read(), "relpose_rotation.h")
ROTATION_ABI_VERSION = _ROTATION_CONSTS["RP_ROTATION_ABI_VERSION"]
ROTATION_MAX_P, ROTATION_MAX_M, ROTATION_MAX_ITERS = (_ROTATION_CONSTS[k] for k in ("RP_ROTATION_MAX_P", "RP_ROTATION_MAX_M", "RP_ROTATION_MAX_ITERS"))
ROTATION_EXPORTS = tuple(_ROTATION_PROTOTYPES)


# the model-selection library (include/relpose_select.h -> librelpose_select.so): the same parser, errcheck and RP_E* codes a thirteenth time
_SELECT_LIB = None
SELECT_HEADER = os.path.join(os.path.dirname(HEADER), "relpose_select.h")
with open(SELECT_HEADER) as _f:
    _SELECT_CONSTS, _, _SELECT_PROTOTYPES, _SELECT_STATUS = _header_contract(_f.read(), "relpose_select.h")
SELECT_ABI_VERSION = _SELECT_CONSTS["RP_SELECT_ABI_VERSION"]
SELECT_MAX_P, SELECT_MAX_C = _SELECT_CONSTS["RP_SELECT_MAX_P"], _SELECT_CONSTS["RP_SELECT_MAX_C"]
SELECT_EXPORTS = tuple(_SELECT_PROTOTYPES)


# the pose-covariance library (include/relpose_covariance.h -> librelpose_covariance.so): the same parser, errcheck and RP_E* codes a fourteenth time
_COVARIANCE_LIB = None
COVARIANCE_HEADER = os.path.join(os.path.dirname(HEADER), "relpose_covariance.h")
with open(COVARIANCE_HEADER) as _f:
    _COVARIANCE_CONSTS, _, _COVARIANCE_PROTOTYPES, _COVARIANCE_STATUS = _header_contract(_f.read(), "relpose_covariance.h")
COVARIANCE_ABI_VERSION = _COVARIANCE_CONSTS["RP_COVARIANCE_ABI_VERSION"]
COVARIANCE_MAX_P, COVARIANCE_SWEEPS = _COVARIANCE_CONSTS["RP_COVARIANCE_MAX_P"], _COVARIANCE_CONSTS["RP_COVARIANCE_SWEEPS"]
COVARIANCE_EXPORTS = tuple(_COVARIANCE_PROTOTYPES)


# the resection library (include/relpose_resection.h -> librelpose_resection.so): the same parser, errcheck and RP_E* codes a fifteenth time
_RESECTION_LIB = None
RESECTION_HEADER = os.path.join(os.path.dirname(HEADER), "relpose_resection.h")
with open(RESECTION_HEADER) as _f:
    _RESECTION_CONSTS, _, _RESECTION_PROTOTYPES, _RESECTION_STATUS = _header_contract(_f.read(), "relpose_resection.h")
RESECTION_ABI_VERSION = _RESECTION_CONSTS["RP_RESECTION_ABI_VERSION"]
RESECTION_MAX_P, RESECTION_MAX_M, RESECTION_MAX_ITERS = (_RESECTION_CONSTS[k] for k in ("RP_RESECTION_MAX_P", "RP_RESECTION_MAX_M", "RP_RESECTION_MAX_ITERS"))
RESECTION_EXPORTS = tuple(_RESECTION_PROTOTYPES)


def lib_path():
    return _build.LIB


def load():
    """Load (building if the .so is absent) and type the C ABI.  Raises on any failure."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = _build.LIB
    if _build.needs_build():           # missing, or older than a kernel source / the header (never a silently stale .so)
        _build.build(verbose=False)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError("rel_pose_amd: cannot load HIP extension %s (%s); there is no CPU fallback" % (path, e))
    lib.rp_abi_version.restype = c_int
    if lib.rp_abi_version() != ABI_VERSION:
        raise RuntimeError("rel_pose_amd: %s has ABI version %d, this package binds version %d -- rebuild with "
                           "`python -m rel_pose_amd._build --force`" % (path, lib.rp_abi_version(), ABI_VERSION))
    if len(EXPORTS) != ABI_EXPORTS:
        raise RuntimeError("rel_pose_amd: include/relpose_hip.h declares %d entry points (RP_ABI_EXPORTS = %d)" % (len(EXPORTS), ABI_EXPORTS))
    lib.rp_abi_export_count.restype = c_int
    if lib.rp_abi_export_count() != ABI_EXPORTS:
        raise RuntimeError("rel_pose_amd: %s was compiled with %d entry points, the header declares %d -- rebuild"
                           % (path, lib.rp_abi_export_count(), ABI_EXPORTS))
    for name, (res, args) in _PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError = symbol missing = broken build
        fn.restype = res
        fn.argtypes = args
        if name in _STATUS:
            fn.errcheck = _raise_on_status
    _LIB = lib
    return lib


def load_readout():
    """Load (building if absent or stale) and type librelpose_readout.so.  Raises on any failure: there is no fallback."""
    global _READOUT_LIB
    if _READOUT_LIB is not None:
        return _READOUT_LIB
    path = _build.READOUT_LIB
    if _build.readout_needs_build():
        _build.build(verbose=False)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError("rel_pose_amd: cannot load HIP extension %s (%s); there is no CPU fallback" % (path, e))
    lib.rp_readout_abi_version.restype = c_int
    if lib.rp_readout_abi_version() != READOUT_ABI_VERSION:
        raise RuntimeError("rel_pose_amd: %s has ABI version %d, this package binds version %d -- rebuild with "
                           "`python -m rel_pose_amd._build --force`" % (path, lib.rp_readout_abi_version(), READOUT_ABI_VERSION))
    for name, (res, args) in _READOUT_PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError = symbol missing = broken build
        fn.restype = res
        fn.argtypes = args
        if name in _READOUT_STATUS:
            fn.errcheck = _raise_on_status
    _READOUT_LIB = lib
    return lib


def load_eightpoint():
    """Load (building if absent or stale) and type librelpose_eightpoint.so.  Raises on any failure: there is no fallback."""
    global _EIGHTPOINT_LIB
    if _EIGHTPOINT_LIB is not None:
        return _EIGHTPOINT_LIB
    path = _build.EIGHTPOINT_LIB
    if _build.eightpoint_needs_build():
        _build.build(verbose=False)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError("rel_pose_amd: cannot load HIP extension %s (%s); there is no CPU fallback" % (path, e))
    lib.rp_eightpoint_abi_version.restype = c_int
    if lib.rp_eightpoint_abi_version() != EIGHTPOINT_ABI_VERSION:
        raise RuntimeError("rel_pose_amd: %s has ABI version %d, this package binds version %d -- rebuild with "
                           "`python -m rel_pose_amd._build --force`" % (path, lib.rp_eightpoint_abi_version(), EIGHTPOINT_ABI_VERSION))
    for name, (res, args) in _EIGHTPOINT_PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError = symbol missing = broken build
        fn.restype = res
        fn.argtypes = args
        if name in _EIGHTPOINT_STATUS:
            fn.errcheck = _raise_on_status
    _EIGHTPOINT_LIB = lib
    return lib


def load_refine():
    """Load (building if absent or stale) and type librelpose_refine.so.  Raises on any failure: there is no fallback."""
    global _REFINE_LIB
    if _REFINE_LIB is not None:
        return _REFINE_LIB
    path = _build.REFINE_LIB
    if _build.refine_needs_build():
        _build.build(verbose=False)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError("rel_pose_amd: cannot load HIP extension %s (%s); there is no CPU fallback" % (path, e))
    lib.rp_refine_abi_version.restype = c_int
    if lib.rp_refine_abi_version() != REFINE_ABI_VERSION:
        raise RuntimeError("rel_pose_amd: %s has ABI version %d, this package binds version %d -- rebuild with "
                           "`python -m rel_pose_amd._build --force`" % (path, lib.rp_refine_abi_version(), REFINE_ABI_VERSION))
    for name, (res, args) in _REFINE_PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError = symbol missing = broken build
        fn.restype = res
        fn.argtypes = args
        if name in _REFINE_STATUS:
            fn.errcheck = _raise_on_status
    _REFINE_LIB = lib
    return lib


def load_consensus():
    """Load (building if absent or stale) and type librelpose_consensus.so.  Raises on any failure: there is no fallback."""
    global _CONSENSUS_LIB
    if _CONSENSUS_LIB is not None:
        return _CONSENSUS_LIB
    path = _build.CONSENSUS_LIB
    if _build.consensus_needs_build():
        _build.build(verbose=False)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError("rel_pose_amd: cannot load HIP extension %s (%s); there is no CPU fallback" % (path, e))
    lib.rp_consensus_abi_version.restype = c_int
    if lib.rp_consensus_abi_version() != CONSENSUS_ABI_VERSION:
        raise RuntimeError("rel_pose_amd: %s has ABI version %d, this package binds version %d -- rebuild with "
                           "`python -m rel_pose_amd._build --force`" % (path, lib.rp_consensus_abi_version(), CONSENSUS_ABI_VERSION))
    for name, (res, args) in _CONSENSUS_PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError = symbol missing = broken build
        fn.restype = res
        fn.argtypes = args
        if name in _CONSENSUS_STATUS:
            fn.errcheck = _raise_on_status
    _CONSENSUS_LIB = lib
    return lib


def load_submatch():
    """Load (building if absent or stale) and type librelpose_submatch.so.  Raises on any failure: there is no fallback."""
    global _SUBMATCH_LIB
    if _SUBMATCH_LIB is not None:
        return _SUBMATCH_LIB
    path = _build.SUBMATCH_LIB
    if _build.submatch_needs_build():
        _build.build(verbose=False)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError("rel_pose_amd: cannot load HIP extension %s (%s); there is no CPU fallback" % (path, e))
    lib.rp_submatch_abi_version.restype = c_int
    if lib.rp_submatch_abi_version() != SUBMATCH_ABI_VERSION:
        raise RuntimeError("rel_pose_amd: %s has ABI version %d, this package binds version %d -- rebuild with "
                           "`python -m rel_pose_amd._build --force`" % (path, lib.rp_submatch_abi_version(), SUBMATCH_ABI_VERSION))
    for name, (res, args) in _SUBMATCH_PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError = symbol missing = broken build
        fn.restype = res
        fn.argtypes = args
        if name in _SUBMATCH_STATUS:
            fn.errcheck = _raise_on_status
    _SUBMATCH_LIB = lib
    return lib


def load_fivepoint():
    """Load (building if absent or stale) and type librelpose_fivepoint.so.  Raises on any failure: there is no fallback."""
    global _FIVEPOINT_LIB
    if _FIVEPOINT_LIB is not None:
        return _FIVEPOINT_LIB
    path = _build.FIVEPOINT_LIB
    if _build.fivepoint_needs_build():
        _build.build(verbose=False)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError("rel_pose_amd: cannot load HIP extension %s (%s); there is no CPU fallback" % (path, e))
    lib.rp_fivepoint_abi_version.restype = c_int
    if lib.rp_fivepoint_abi_version() != FIVEPOINT_ABI_VERSION:
        raise RuntimeError("rel_pose_amd: %s has ABI version %d, this package binds version %d -- rebuild with "
                           "`python -m rel_pose_amd._build --force`" % (path, lib.rp_fivepoint_abi_version(), FIVEPOINT_ABI_VERSION))
    for name, (res, args) in _FIVEPOINT_PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError = symbol missing = broken build
        fn.restype = res
        fn.argtypes = args
        if name in _FIVEPOINT_STATUS:
            fn.errcheck = _raise_on_status
    _FIVEPOINT_LIB = lib
    return lib


def load_homography():
    """Load (building if absent or stale) and type librelpose_homography.so.  Raises on any failure: there is no fallback."""
    global _HOMOGRAPHY_LIB
    if _HOMOGRAPHY_LIB is not None:
        return _HOMOGRAPHY_LIB
    path = _build.HOMOGRAPHY_LIB
    if _build.homography_needs_build():
        _build.build(verbose=False)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError("rel_pose_amd: cannot load HIP extension %s (%s); there is no CPU fallback" % (path, e))
    lib.rp_homography_abi_version.restype = c_int
    if lib.rp_homography_abi_version() != HOMOGRAPHY_ABI_VERSION:
        raise RuntimeError("rel_pose_amd: %s has ABI version %d, this package binds version %d -- rebuild with "
                           "`python -m rel_pose_amd._build --force`" % (path, lib.rp_homography_abi_version(), HOMOGRAPHY_ABI_VERSION))
    for name, (res, args) in _HOMOGRAPHY_PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError = symbol missing = broken build
        fn.restype = res
        fn.argtypes = args
        if name in _HOMOGRAPHY_STATUS:
            fn.errcheck = _raise_on_status
    _HOMOGRAPHY_LIB = lib
    return lib


def load_triangulate():
    """Load (building if absent or stale) and type librelpose_triangulate.so.  Raises on any failure: there is no fallback."""
    global _TRIANGULATE_LIB
    if _TRIANGULATE_LIB is not None:
        return _TRIANGULATE_LIB
    path = _build.TRIANGULATE_LIB
    if _build.triangulate_needs_build():
        _build.build(verbose=False)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError("rel_pose_amd: cannot load HIP extension %s (%s); there is no CPU fallback" % (path, e))
    lib.rp_triangulate_abi_version.restype = c_int
    if lib.rp_triangulate_abi_version() != TRIANGULATE_ABI_VERSION:
        raise RuntimeError("rel_pose_amd: %s has ABI version %d, this package binds version %d -- rebuild with "
                           "`python -m rel_pose_amd._build --force`" % (path, lib.rp_triangulate_abi_version(), TRIANGULATE_ABI_VERSION))
    for name, (res, args) in _TRIANGULATE_PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError = symbol missing = broken build
        fn.restype = res
        fn.argtypes = args
        if name in _TRIANGULATE_STATUS:
            fn.errcheck = _raise_on_status
    _TRIANGULATE_LIB = lib
    return lib


def load_conv5x5():
    """Load (building if absent or stale) and type librelpose_conv5x5.so.  Raises on any failure: there is no fallback."""
    global _CONV5X5_LIB
    if _CONV5X5_LIB is not None:
        return _CONV5X5_LIB
    path = _build.CONV5X5_LIB
    if _build.conv5x5_needs_build():
        _build.build(verbose=False)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError("rel_pose_amd: cannot load HIP extension %s (%s); there is no CPU fallback" % (path, e))
    lib.rp_conv5x5_abi_version.restype = c_int
    if lib.rp_conv5x5_abi_version() != CONV5X5_ABI_VERSION:
        raise RuntimeError("rel_pose_amd: %s has ABI version %d, this package binds version %d -- rebuild with "
                           "`python -m rel_pose_amd._build --force`" % (path, lib.rp_conv5x5_abi_version(), CONV5X5_ABI_VERSION))
    for name, (res, args) in _CONV5X5_PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError = symbol missing = broken build
        fn.restype = res
        fn.argtypes = args
        if name in _CONV5X5_STATUS:
            fn.errcheck = _raise_on_status
    _CONV5X5_LIB = lib
    return lib


def load_guided():
    """Load (building if absent or stale) and type librelpose_guided.so.  Raises on any failure: there is no fallback."""
    global _GUIDED_LIB
    if _GUIDED_LIB is not None:
        return _GUIDED_LIB
    path = _build.GUIDED_LIB
    if _build.guided_needs_build():
        _build.build(verbose=False)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError("rel_pose_amd: cannot load HIP extension %s (%s); there is no CPU fallback" % (path, e))
    lib.rp_guided_abi_version.restype = c_int
    if lib.rp_guided_abi_version() != GUIDED_ABI_VERSION:
        raise RuntimeError("rel_pose_amd: %s has ABI version %d, this package binds version %d -- rebuild with "
                           "`python -m rel_pose_amd._build --force`" % (path, lib.rp_guided_abi_version(), GUIDED_ABI_VERSION))
    for name, (res, args) in _GUIDED_PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError = symbol missing = broken build
        fn.restype = res
        fn.argtypes = args
        if name in _GUIDED_STATUS:
            fn.errcheck = _raise_on_status
    _GUIDED_LIB = lib
    return lib


def load_rotation():
    """Load (building if absent or stale) and type librelpose_rotation.so.  Raises on any failure: there is no fallback."""
    global _ROTATION_LIB
    if _ROTATION_LIB is not None:
        return _ROTATION_LIB
    path = _build.ROTATION_LIB
    if _build.rotation_needs_build():
        _build.build(verbose=False)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError("rel_pose_amd: cannot load HIP extension %s (%s); there is no CPU fallback" % (path, e))
    lib.rp_rotation_abi_version.restype = c_int
    if lib.rp_rotation_abi_version() != ROTATION_ABI_VERSION:
        raise RuntimeError("rel_pose_amd: %s has ABI version %d, this package binds version %d -- rebuild with "
                           "`python -m rel_pose_amd._build --force`" % (path, lib.rp_rotation_abi_version(), ROTATION_ABI_VERSION))
    for name, (res, args) in _ROTATION_PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError = symbol missing = broken build
        fn.restype = res
        fn.argtypes = args
        if name in _ROTATION_STATUS:
            fn.errcheck = _raise_on_status
    _ROTATION_LIB = lib
    return lib


def load_select():
    """Load (building if absent or stale) and type librelpose_select.so.  Raises on any failure: there is no fallback."""
    global _SELECT_LIB
    if _SELECT_LIB is not None:
        return _SELECT_LIB
    path = _build.SELECT_LIB
    if _build.select_needs_build():
        _build.build(verbose=False)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError("rel_pose_amd: cannot load HIP extension %s (%s); there is no CPU fallback" % (path, e))
    lib.rp_select_abi_version.restype = c_int
    if lib.rp_select_abi_version() != SELECT_ABI_VERSION:
        raise RuntimeError("rel_pose_amd: %s has ABI version %d, this package binds version %d -- rebuild with "
                           "`python -m rel_pose_amd._build --force`" % (path, lib.rp_select_abi_version(), SELECT_ABI_VERSION))
    for name, (res, args) in _SELECT_PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError = symbol missing = broken build
        fn.restype = res
        fn.argtypes = args
        if name in _SELECT_STATUS:
            fn.errcheck = _raise_on_status
    _SELECT_LIB = lib
    return lib


def load_covariance():
    """Load (building if absent or stale) and type librelpose_covariance.so.  Raises on any failure: there is no fallback."""
    global _COVARIANCE_LIB
    if _COVARIANCE_LIB is not None:
        return _COVARIANCE_LIB
    path = _build.COVARIANCE_LIB
    if _build.covariance_needs_build():
        _build.build(verbose=False)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError("rel_pose_amd: cannot load HIP extension %s (%s); there is no CPU fallback" % (path, e))
    lib.rp_covariance_abi_version.restype = c_int
    if lib.rp_covariance_abi_version() != COVARIANCE_ABI_VERSION:
        raise RuntimeError("rel_pose_amd: %s has ABI version %d, this package binds version %d -- rebuild with "
                           "`python -m rel_pose_amd._build --force`" % (path, lib.rp_covariance_abi_version(), COVARIANCE_ABI_VERSION))
    for name, (res, args) in _COVARIANCE_PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError = symbol missing = broken build
        fn.restype = res
        fn.argtypes = args
        if name in _COVARIANCE_STATUS:
            fn.errcheck = _raise_on_status
    _COVARIANCE_LIB = lib
    return lib


def load_resection():
    """Load (building if absent or stale) and type librelpose_resection.so.  Raises on any failure: there is no fallback."""
    global _RESECTION_LIB
    if _RESECTION_LIB is not None:
        return _RESECTION_LIB
    path = _build.RESECTION_LIB
    if _build.resection_needs_build():
        _build.build(verbose=False)
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise RuntimeError("rel_pose_amd: cannot load HIP extension %s (%s); there is no CPU fallback" % (path, e))
    lib.rp_resection_abi_version.restype = c_int
    if lib.rp_resection_abi_version() != RESECTION_ABI_VERSION:
        raise RuntimeError("rel_pose_amd: %s has ABI version %d, this package binds version %d -- rebuild with "
                           "`python -m rel_pose_amd._build --force`" % (path, lib.rp_resection_abi_version(), RESECTION_ABI_VERSION))
    for name, (res, args) in _RESECTION_PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError = symbol missing = broken build
        fn.restype = res
        fn.argtypes = args
        if name in _RESECTION_STATUS:
            fn.errcheck = _raise_on_status
    _RESECTION_LIB = lib
    return lib


def _raise_on_status(rc, func, args):
    """ctypes errcheck of every entry point that launches work: its return value is a status, never a count."""
    check(rc, func.__name__)
    return rc


def check(rc, what):
    if rc != 0:
        if rc < 0:
            raise RuntimeError("rel_pose_amd: %s failed: %s (RP error %d)" % (what, RP_ERRORS.get(rc, "?"), rc))
        raise RuntimeError("rel_pose_amd: %s failed: hipError %d" % (what, rc))
