"""ctypes binding of libonepose_hip.so (the C-ABI in include/onepose_hip.h).

This is the binding a maintainer of the reference would drop in: plain
pointers from ``torch.Tensor.data_ptr()``, the current HIP stream, and an int status mapped
to exceptions.  The library is loaded from the package directory (built in-tree by
``onepose_amd.build``); there is no fallback -- if it is missing, every call raises.

The header is the one source of the signatures: ``SIGNATURES`` is parsed from it at import,
``load()`` types every function from it, and ``call`` / ``run`` take their arguments by the
header's parameter names.
"""
from __future__ import annotations

import ctypes
import keyword
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# ONEPOSE_LIB: an alternative in-tree build of the same library (A/B measurement, tools/ab.sh)
LIB_PATH = os.environ.get("ONEPOSE_LIB") or os.path.join(_HERE, "libonepose_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "onepose_hip.h")
# Families added after ABI 9 declare themselves in headers of their own, which onepose_hip.h
# includes: SIGNATURES / PROTOTYPES stay the ABI-9 header's table, FAMILY_SIGNATURES holds theirs.
FAMILY_HEADERS = ("onepose_two_view.h",)
# Later families: one table per header in FAMILIES ({header: signatures}), so that the tables
# above stay what they were when their tests pinned them.
LATER_HEADERS = ("onepose_superglue_counts.h", "onepose_match_counts.h", "onepose_global_ba.h")

c_int, c_int64, c_size_t, c_float, c_double = (ctypes.c_int, ctypes.c_int64, ctypes.c_size_t,
                                               ctypes.c_float, ctypes.c_double)
c_void_p, c_char_p = ctypes.c_void_p, ctypes.c_char_p

# onepose_allgather_fn: int (*)(size_t bytes_per_rank, void* stream, void* user)
ALLGATHER_FN = ctypes.CFUNCTYPE(c_int, c_size_t, c_void_p, c_void_p)
# the constants below mirror the header's enums (tests/test_binding.py compares them)
ABI_VERSION = 9
DEVERR_STALE_CACHE = 1   # ONEPOSE_DEVERR_STALE_CACHE
STAGE_INPUTS, STAGE_LAYER0, STAGE_FINAL, STAGE_SCORE, STAGE_WINNERS = 0, 1, 13, 14, 15  # ABI 6
REGION_STATE2D, REGION_STATE3D, REGION_DESC2D, REGION_DESC3D = 0, 1, 2, 3   # ABI 7
WHERE_WORKSPACE, WHERE_OBJECT_CACHE = 0, 1   # ONEPOSE_WHERE_*
OBJ_GAT_TABLES = 1   # ONEPOSE_OBJ_GAT_TABLES
DT_F32, DT_F16 = 0, 1   # ONEPOSE_DT_*


class OnePoseError(RuntimeError):
    pass


_VALUE_TYPES = {"int": c_int, "int64_t": c_int64, "size_t": c_size_t, "float": c_float,
                "double": c_double, "unsigned": ctypes.c_uint, "uint64_t": ctypes.c_uint64,
                "onepose_allgather_fn": ALLGATHER_FN}
_DECL = re.compile(r"(.+?)\b(onepose_\w+)\s*\((.*)\)", re.S)


def parse_header(text):
    """The header's declarations and enums:
    ({name: (restype, ((param_name, ctype), ...))}, {ENUM_NAME: value}).
    Every pointer is c_void_p (a ``const char*`` return c_char_p).  Strict: a statement that is
    not a declaration, or a type that has no ctype here, raises and names the declaration."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r'^\s*(#.*|extern "C" \{|\})$', " ", text, flags=re.M)   # (extern "C"'s braces)
    enums = {}

    def take_enum(m):
        for item in m.group(1).split(","):
            name, eq, value = (x.strip() for x in item.partition("="))
            if not eq or not re.fullmatch(r"\w+", name):
                raise OnePoseError(f"onepose_hip.h: enum item {item.strip()!r} is not NAME = value")
            enums[name] = int(value, 0)
        return " "
    text = re.sub(r"\benum\s*\{(.*?)\}\s*;", take_enum, text, flags=re.S)

    def take_typedef(m):
        if m.group(1) not in _VALUE_TYPES:
            raise OnePoseError(f"onepose_hip.h: typedef {m.group(1)} has no ctypes type")
        return " "
    text = re.sub(r"\btypedef\b[^;]*?\(\s*\*\s*(\w+)\s*\)[^;]*;", take_typedef, text)

    def ctype(decl, what, name):
        if "*" in decl:
            return c_void_p
        t = re.sub(r"\bconst\b", " ", decl).strip()
        if t not in _VALUE_TYPES:
            raise OnePoseError(f"onepose_hip.h: {name}: {what} type {decl.strip()!r} has no "
                               "ctypes type")
        return _VALUE_TYPES[t]

    signatures = {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = _DECL.fullmatch(stmt)
        if m is None:
            raise OnePoseError(f"onepose_hip.h: not a declaration: {' '.join(stmt.split())!r}")
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        if name in signatures:
            raise OnePoseError(f"onepose_hip.h: {name} is declared twice")
        if re.sub(r"\s+", "", ret) == "constchar*":
            restype = c_char_p
        elif ret == "void":
            restype = None
        elif "*" in ret:
            raise OnePoseError(f"onepose_hip.h: {name}: return type {ret!r} has no ctypes type")
        else:
            restype = ctype(ret, "return", name)
        args = []
        for p in ([] if params == "void" else params.split(",")):
            pm = re.fullmatch(r"\s*(.*?[\s*])(\w+)\s*", p, re.S)
            if pm is None:
                raise OnePoseError(f"onepose_hip.h: {name}: parameter {p.strip()!r} has no name")
            args.append((pm.group(2), ctype(pm.group(1), f"parameter {pm.group(2)}'s", name)))
        signatures[name] = (restype, tuple(args))
    return signatures, enums


def _read_header(path=None):
    path = path or HEADER_PATH
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise OnePoseError(f"{path} is missing ({e.strerror}): onepose_amd reads the "
                           "library's signatures from it (in-tree layout)") from None


# name -> (restype, ((param_name, ctype), ...)), and the header's enum values
SIGNATURES, ENUMS = parse_header(_read_header())
# name -> (restype, [argtypes])
PROTOTYPES = {name: (res, [t for _, t in params]) for name, (res, params) in SIGNATURES.items()}
# the family headers' declarations, same shape as SIGNATURES / PROTOTYPES
FAMILY_SIGNATURES = {}
for _h in FAMILY_HEADERS:
    _sigs, _ = parse_header(_read_header(os.path.join(os.path.dirname(HEADER_PATH), _h)))
    if set(_sigs) & (set(SIGNATURES) | set(FAMILY_SIGNATURES)):
        raise OnePoseError(f"{_h}: declares a function that another header declares")
    FAMILY_SIGNATURES.update(_sigs)
FAMILY_PROTOTYPES = {name: (res, [t for _, t in params])
                     for name, (res, params) in FAMILY_SIGNATURES.items()}
# header -> that header's declarations (same shape as SIGNATURES), and all of them in one table
FAMILIES = {}
LATER_SIGNATURES = {}
for _h in LATER_HEADERS:
    _sigs, _ = parse_header(_read_header(os.path.join(os.path.dirname(HEADER_PATH), _h)))
    if set(_sigs) & (set(SIGNATURES) | set(FAMILY_SIGNATURES) | set(LATER_SIGNATURES)):
        raise OnePoseError(f"{_h}: declares a function that another header declares")
    FAMILIES[_h] = _sigs
    LATER_SIGNATURES.update(_sigs)
LATER_PROTOTYPES = {name: (res, [t for _, t in params])
                    for name, (res, params) in LATER_SIGNATURES.items()}
# name -> (keyword names in order, indices of the pointer parameters); a parameter named like
# a Python keyword takes a trailing underscore (onepose_affine_partial_ransac's from_)
_ORDER = {name: (tuple(n + "_" * keyword.iskeyword(n) for n, _ in params),
                 tuple(i for i, (_, t) in enumerate(params) if t is c_void_p))
          for name, (_, params) in {**SIGNATURES, **FAMILY_SIGNATURES,
                                    **LATER_SIGNATURES}.items()}

_lib = None


def load():
    """Load the shared library (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OnePoseError(
                f"{LIB_PATH} is missing: build it with `python -m onepose_amd.build` "
                "(onepose_amd has no CPU fallback)")
        lib = ctypes.CDLL(LIB_PATH)
        # A/B measurement only: an older build named by ONEPOSE_LIB may predate the newest
        # entry points (ABI >= 3); callers fall back where one is missing (size_query)
        ab = bool(os.environ.get("ONEPOSE_LIB"))
        for name, (res, args) in {**PROTOTYPES, **FAMILY_PROTOTYPES, **LATER_PROTOTYPES}.items():
            if ab and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.onepose_abi_version() != ABI_VERSION and not (ab and lib.onepose_abi_version() >= 3):
            raise OnePoseError(f"{LIB_PATH}: ABI version {lib.onepose_abi_version()}, "
                               f"expected {ABI_VERSION}: rebuild with `python -m onepose_amd.build`")
        _lib = lib
    return _lib


def call(name, **args):
    """lib.<name>(...) with the arguments given by the header's parameter names; returns the
    function's raw result.  A tensor in a pointer slot goes as its data_ptr(), None as a null
    pointer.  Every parameter must be given (no defaults, `stream` included) and no other: a
    missing or unknown one raises TypeError before the library is entered.  Nothing is
    allocated or synchronised, so it can be used inside a graph capture."""
    try:
        names, pointers = _ORDER[name]
    except KeyError:
        raise TypeError(f"{name} is not declared in onepose_hip.h or a family header") from None
    try:
        vals = [args[n] for n in names]
    except KeyError as e:
        raise TypeError(f"{name}: missing argument {e.args[0]!r}") from None
    if len(args) != len(names):
        raise TypeError(f"{name}: unknown argument {sorted(set(args) - set(names))[0]!r}")
    for i in pointers:
        if hasattr(vals[i], "data_ptr"):
            vals[i] = vals[i].data_ptr()
    return getattr(_lib or load(), name)(*vals)


def run(name, **args) -> None:
    """call() for a function that returns a status: raises OnePoseError unless it is 0."""
    check(call(name, **args), name)


def workspace_bytes(lib, B, n1, n3, L, with_conf, precision) -> int:
    """onepose_match_workspace_bytes_ex (this precision's need), or the every-precision query
    on an older A/B build without it."""
    if hasattr(lib, "onepose_match_workspace_bytes_ex"):
        return call("onepose_match_workspace_bytes_ex", batch=B, n1=n1, n3=n3, num_leaf=L,
                    with_conf=int(with_conf), precision=int(precision))
    return lib.onepose_match_workspace_bytes(B, n1, n3, L, int(with_conf))


def object_cache_bytes(lib, n3, L, flags, precision) -> int:
    if hasattr(lib, "onepose_object_cache_bytes_ex"):
        return lib.onepose_object_cache_bytes_ex(n3, L, flags, int(precision))
    return lib.onepose_object_cache_bytes(n3, L, flags)


def workspace_region(lib, B, n1, n3, L, with_conf, precision, region, after_stage):
    """onepose_match_workspace_region: (where, byte offset, byte count) of `region` (REGION_*)
    after the stages up to `after_stage` of a cached forward; where is WHERE_*."""
    where, off, nbytes = c_int(0), c_size_t(0), c_size_t(0)
    run("onepose_match_workspace_region", batch=B, n1=n1, n3=n3, num_leaf=L,
        with_conf=int(with_conf), precision=int(precision), region=int(region),
        after_stage=int(after_stage), where=ctypes.byref(where), offset=ctypes.byref(off),
        bytes=ctypes.byref(nbytes))
    return int(where.value), int(off.value), int(nbytes.value)


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().onepose_last_error().decode(errors="replace")
        raise OnePoseError(f"{what or 'onepose_hip'} failed (status {rc}): {msg}")


def stream_ptr(device=None) -> int:
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def device_errors(clear: bool = False) -> int:
    """The library's sticky device-side error bits (DEVERR_*; onepose_device_errors).
    Synchronises with the device."""
    lib = load()
    v = ctypes.c_uint(0)
    check(lib.onepose_device_errors(1 if clear else 0, ctypes.byref(v)), "device_errors")
    return int(v.value)
