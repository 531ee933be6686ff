"""ctypes binding of libguidegen_hip.so, derived from its public header include/guidegen_hip.h.

The header is the one statement of the C-ABI: the constants, the descriptor structs and every prototype below are read from its text
at import (parse_header), so an entry point or a field is added in the header and nowhere else.  tests/test_capi_cpu.py checks the
result against the compiler (struct layouts) and against a second reading of the declarations.

There is NO fallback: if the header or the shared library is missing or a symbol is absent this module raises, and every product op
raises RuntimeError when a call returns a negative gg_status (message from gg_last_error()).
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libguidegen_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "guidegen_hip.h")

# by-value C types; a name outside this map is an error, never a guess
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
# one declarator with its type: "const float *bias", "int32_t N", "int32_t plan[4]", "void *stream", and the bare "const char *" of a result
_DECL = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w*)\s*(\[\w*\])?$")


def _ctype(base: str, pointer: bool, structs: dict, what: str):
    if pointer:
        return C.POINTER(structs[base]) if base in structs else C.c_void_p
    if base not in _SCALARS:
        raise ValueError(f"{what}: no ctypes type for {base!r}")
    return _SCALARS[base]


def parse_header(text: str):
    """(constants, structs, signatures) of a header in the C subset guidegen_hip.h is written in: `#define GG_X <int>`, `typedef enum`,
    `typedef struct` of scalars and pointers, and prototypes.  Anything else raises ValueError naming the declaration."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    constants = {m[1]: int(m[2], 0) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(GG_\w+)[ \t]+(-?\w+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus.*?^[ \t]*#[ \t]*endif[^\n]*$", "", text, flags=re.S | re.M)   # extern "C" { ... }
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    for m in re.finditer(r"typedef\s+enum\s*\{(.*?)\}\s*\w+\s*;", text, flags=re.S):
        value = 0
        for item in filter(None, (s.strip() for s in m[1].split(","))):
            name, _, given = (s.strip() for s in item.partition("="))
            value = int(given, 0) if given else value
            constants[name] = value
            value += 1
    structs = {}
    for m in re.finditer(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for stmt in filter(None, (s.strip() for s in m[1].split(";"))):
            first, *more = (s.strip() for s in stmt.split(","))                 # "int32_t N, D" / "const void *q, *k": one type, several names
            d = _DECL.match(first)
            if not d or not d[3] or d[4]:
                raise ValueError(f"{m[2]}: cannot read the field declaration {stmt!r}")
            for star, name in [(d[2], d[3])] + [re.fullmatch(r"(\*?)\s*(\w+)", s).groups() for s in more]:
                fields.append((name, _ctype(d[1], bool(star), {}, f"{m[2]}.{name}")))
        structs[m[2]] = type(m[2], (C.Structure,), {"_fields_": fields})
    signatures = {}
    for stmt in filter(None, (s.strip() for s in re.sub(r"typedef\s+(?:struct|enum)\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S).split(";"))):
        m = re.fullmatch(r"(.*?)\b(\w+)\s*\((.*)\)", stmt, flags=re.S)
        res = m and _DECL.match(m[1].strip())
        if not res or res[3] or res[4]:
            raise ValueError(f"cannot read the declaration {stmt!r}")
        restype = C.c_char_p if (res[1], res[2]) == ("char", "*") else _ctype(res[1], bool(res[2]), structs, m[2])
        argtypes = []
        for arg in ([] if m[3].strip() == "void" else (a.strip() for a in m[3].split(","))):
            d = _DECL.match(arg)
            if not d or not d[3]:
                raise ValueError(f"{m[2]}: cannot read the parameter {arg!r}")
            argtypes.append(_ctype(d[1], bool(d[2] or d[4]), structs, f"{m[2]}({arg})"))        # an array parameter is a pointer
        signatures[m[2]] = (restype, argtypes)
    return constants, structs, signatures


def _header_text(path: str) -> str:
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: the ctypes binding is derived from the C header, which ships with the package's source tree")
    with open(path) as fh:
        return fh.read()


# GG_OK, GG_ERR_*, GG_BF16, GG_F32, GG_LOSS_*, GG_DDPM_* become module attributes; SIGNATURES: name -> (restype, argtypes)
CONSTANTS, STRUCTS, SIGNATURES = parse_header(_header_text(HEADER_PATH))
globals().update(CONSTANTS)
GG_BF16, GG_F32 = CONSTANTS["GG_BF16"], CONSTANTS["GG_F32"]
ConvDesc, AttentionDesc = STRUCTS["gg_conv_desc"], STRUCTS["gg_attention_desc"]

_lib = None


def load() -> C.CDLL:
    """Load the library once; raises (never falls back) if it is absent or incomplete."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is mandatory (there is no CPU fallback). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'` or jointimagegeneration_amd/csrc/build.sh")
    # torch FIRST: its wheel bundles its own HIP runtime (torch/lib/libamdhip64.so); loaded before this library, the dynamic loader binds
    # libguidegen_hip.so's `libamdhip64.so.7` to that same copy.  The other order leaves TWO HIP runtimes in the process, and launches
    # through the second one fail with "no ROCm-capable device is detected" on tensors the first one owns.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise RuntimeError(f"libguidegen_hip.so does not export {name}")
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().gg_last_error()
        raise RuntimeError(f"{what} failed with gg_status {rc}: {msg.decode() if msg else ''}")


def call(name: str, *args) -> None:
    """Call a status-returning entry point of the loaded library; a failure raises with the library's message."""
    check(getattr(load(), name)(*args), name)
