"""ctypes binding of libdram_hip.so, read from include/dram_hip.h.

The header is the only description of the C ABI on the host side: at import it is parsed into ``SIGNATURES``
(name -> (restype, argtypes)), the ``ctypes.Structure`` classes of its structs and its integer ``#define`` constants.
``load()`` sets these prototypes on a library that carries the fingerprint of the same header file.

The product path has NO fallback: if the library is missing or fails to load,
``load()`` raises.  ``import torch`` happens first on purpose -- libdram_hip.so needs
``libamdhip64.so.7`` and must bind to the HIP runtime PyTorch has already loaded
(same soname), so that torch's streams and device pointers are valid inside it.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_void_p

import torch  # noqa: F401  (must precede CDLL: loads the HIP runtime we bind to)

from . import _build

# C type -> ctypes type, for parameters, return values and struct fields; `typedef void* NAME;` adds NAME (dram_stream_t)
_SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong,
            "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
_POINTEES = set(_SCALARS) | {"void", "char", "uint8_t", "int16_t"}     # ... and the header's structs; any pointer is a c_void_p
_ID = r"[A-Za-z_]\w*"
_DECLARATOR = re.compile(rf"(const\s+)?({_ID}(?:\s+{_ID})*?)(?:\s*(\*)\s*|\s+)({_ID})((?:\s*\[\d+\])*)")
_FUNCTION = re.compile(rf"(const\s+char\s*\*|{_ID}(?:\s+{_ID})*?\s)\s*(dram_\w+)\s*\((.*)\)", re.S)


def parse_header(text: str):
    """The text of a dram_hip.h -> (signatures {name: (restype, argtypes)}, {name: ctypes.Structure class},
    {name: value} of the `#define DRAM_NAME <integer>` lines).  Knows exactly the subset of C the header is written
    in and raises ValueError with the declaration's text on anything else -- it never guesses or skips: a wrong
    prototype calls a kernel with shifted arguments."""
    def bad(what, decl):
        return ValueError(f"dram_hip.h: {what}: {' '.join(decl.split())!r}")

    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    named = set(re.findall(r"\b(dram_\w+)\s*\(", text))
    consts = {}
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(DRAM_\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M):
        if not re.fullmatch(r"-?\d+|\(-?\d+\)", m[2]):
            raise bad(f"{m[1]} is not an integer constant", m[0])
        consts[m[1]] = int(m[2].strip("()"))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'\A\s*extern\s+"C"\s*\{(.*)\}\s*\Z', r"\1", text, flags=re.S)
    text = re.sub(r"\benum\s*\{[^{}]*\}\s*;", "", text)
    types, structs, sigs = dict(_SCALARS), {}, {}

    def declarator(decl, what):
        m = _DECLARATOR.fullmatch(decl.strip())
        if not m:
            raise bad(f"{what}: a type and a name are required", decl)
        const, base, ptr, name, dims = m.groups()
        if base not in ((_POINTEES | set(structs)) if ptr else types):
            raise bad(f"{what} {name!r}: no ctypes mapping for type {base!r}", decl)
        ctype = (ctypes.POINTER(structs[base]) if const and base == "DramConvDesc" else c_void_p) if ptr else types[base]
        for n in reversed(re.findall(r"\d+", dims)):
            ctype = ctype * int(n)
        return name, ctype, base

    def handle_typedef(m):
        types[m[1]] = c_void_p
        return ""

    def struct_typedef(m):
        tag, body, name = m.groups()
        if tag != name:
            raise bad("struct tag and typedef name differ", m[0])
        fields = []
        for stmt in filter(str.strip, body.split(";")):
            first, *more = stmt.split(",")                      # int32_t D, H, W, Cin;
            fname, ctype, base = declarator(first, f"field of {name}")
            fields.append((fname, ctype))
            fields += [declarator(f"{base} {d}", f"field of {name}")[:2] for d in more]
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
        return ""

    text = re.sub(rf"\btypedef\s+void\s*\*\s*({_ID})\s*;", handle_typedef, text)
    text = re.sub(rf"\btypedef\s+struct\s+({_ID})\s*\{{([^{{}}]*)\}}\s*({_ID})\s*;", struct_typedef, text)
    *decls, rest = text.split(";")
    for decl in decls:
        m = _FUNCTION.fullmatch(decl.strip())
        if not m:
            raise bad("not a function declaration", decl)
        ret, name, params = m[1].strip(), m[2], m[3]
        if not ret.endswith("*") and ret not in types:
            raise bad(f"{name}: no ctypes mapping for return type {ret!r}", decl)
        if name in sigs:
            raise bad(f"{name} is declared twice", decl)
        args = [declarator(p, f"parameter of {name}")[1] for p in ([] if params.strip() == "void" else params.split(","))]
        if any(issubclass(a, ctypes.Array) for a in args):
            raise bad(f"{name}: array parameter", decl)
        sigs[name] = (ctypes.c_char_p if ret.endswith("*") else types[ret], args)
    if rest.strip():
        raise bad("text after the last declaration", rest)
    if named != set(sigs):
        raise ValueError(f"dram_hip.h: `dram_...(` without a declaration of that name: {sorted(named - set(sigs))}")
    return sigs, structs, consts


with open(os.path.join(_build.INCLUDE, "dram_hip.h")) as _f:
    SIGNATURES, _STRUCTS, _CONSTANTS = parse_header(_f.read())
# the header's structs (DramConvDesc, DramTensorRef, DramChunkRef, DramPackRef, DramProfRecord, DramAugment) and integer
# constants (DRAM_ERR_*, DRAM_CONV_*, DRAM_FOLD_TICKET_DOUBLES, ...) under their C names
globals().update(_STRUCTS)
globals().update(_CONSTANTS)
ABI_VERSION = _CONSTANTS["DRAM_ABI_VERSION"]
OPT_CHUNK = _CONSTANTS["DRAM_OPT_CHUNK"]
_LIB = None


def lib_path() -> str:
    return _build.LIB_PATH


def load(build: bool = True) -> ctypes.CDLL:
    """Load libdram_hip.so.  With hipcc present the (content-hash incremental) build runs first,
    so a library older than the sources is never loaded; either way the library must carry the
    fingerprint of THIS include/dram_hip.h, the file SIGNATURES was parsed from -- a build from
    another header would be called with shifted arguments (wild device writes), so it is refused."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if build and _build.have_hipcc():
        _build.build_library()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here == header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    if lib.dram_version() != ABI_VERSION:
        raise RuntimeError("libdram_hip.so ABI version mismatch")
    got, want = lib.dram_abi_hash().decode(), _build.abi_hash()
    if got != want:
        raise RuntimeError(f"libdram_hip.so was built from another include/dram_hip.h (library {got}, header {want}): "
                           "rebuild with __graft_entry__.build()")
    _LIB = lib
    return lib
