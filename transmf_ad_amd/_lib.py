"""ctypes binding of libtmf_hip.so, DERIVED from its C ABI header include/tmf_hip.h.

parse_header() reads the header at import and yields everything the binding needs, so nothing is kept in step by hand:
  PROTOTYPES   name -> (restype, argtypes) of every declared function;
  the Structure classes (tmf_snet_desc -> SnetDesc, tmf_xformer_params -> XformerParams, ...);
  the integer #defines without their TMF_ prefix (POOL_MAX2, SNET_ALONE, ADAM_MAX_TENSORS, ...; all of them in CONSTANTS).
The header states the conventions the parser relies on.  It fails closed: a declaration, parameter type, struct field or
#define it cannot map raises HeaderError with the line, it never guesses.

There is NO fallback: if the library is missing, or a call returns non-zero, this
module raises.  The product path never routes around the HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import os
import re

from .build import ABI_HEADER

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtmf_hip.so")

_SCALARS = {"int": C.c_int, "long": C.c_long, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong,
            "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
_FIELD_SCALARS = dict(_SCALARS, int32_t=C.c_int32)
_POINTEES = set(_FIELD_SCALARS) | {"void", "char", "unsigned char", "unsigned", "int64_t"}      # what a plain (void*) pointer may point to
_DEVICE_STRUCTS = {"tmf_augment_decision"}      # records in device memory: a pointer to one is a device pointer
_TYPE_WORDS = {"const", "unsigned", "void", "char"} | set(_FIELD_SCALARS) | _POINTEES


class HeaderError(ValueError):
    pass


def parse_header(text: str):
    """-> (constants: TMF_NAME -> int, structs: C name -> Structure class, prototypes: name -> (restype, argtypes))."""
    blank = lambda m: re.sub(r"[^\n]", " ", m.group())          # erase, keeping every line where it was
    text = re.sub(r"/\*.*?\*/", blank, text, flags=re.S)

    def fail(pos, what):
        raise HeaderError(f"include/tmf_hip.h:{text.count(chr(10), 0, pos) + 1}: {what}")

    constants = {}
    for m in re.finditer(r"^#define[ \t]+(\w+)(\(\w*\))?[ \t]*(.*)$", text, flags=re.M):
        name, macro_args, value = m.group(1), m.group(2), m.group(3).strip()
        if macro_args or not value:             # function-like macro / include guard
            continue
        try:
            constants[name] = int(value, 0)
        except ValueError:
            fail(m.start(), f"#define {name} {value!r} is not an integer")
    text = re.sub(r"^#ifdef __cplusplus\n.*?\n#endif", blank, text, flags=re.S | re.M)
    text = re.sub(r"^#.*$", blank, text, flags=re.M)

    structs = {}

    def ctype_of(pos, decl, what, is_return=False):
        """The ctypes type of `decl` = a C type without its name (parameter or return type)."""
        base = " ".join(w for w in decl.replace("*", " ").split() if w != "const")
        stars = decl.count("*")
        if stars == 0:
            if base == "void" and is_return:
                return None
            if base in _SCALARS:
                return _SCALARS[base]
        elif stars == 1 and base == "char":
            return C.c_char_p
        elif stars == 1 and base in structs:
            return C.c_void_p if base in _DEVICE_STRUCTS else C.POINTER(structs[base])
        elif base in _POINTEES:
            return C.c_void_p
        fail(pos, f"{what}: unknown type {decl.strip()!r}")

    def struct_of(m):
        cname, body = m.group(1), m.group(2)
        if m.group(3) != cname:
            fail(m.start(), f"typedef struct {cname} is named {m.group(3)}")
        fields = []
        for d in re.finditer(r"[^;]+", body):
            if not d.group().strip():
                continue
            t = re.fullmatch(r"\s*(?:const\s+)?((?:unsigned\s+)?(?:long\s+long|\w+))\s*(.+)", d.group(), flags=re.S)
            if not t:
                fail(m.start(2) + d.start(), f"{cname}: cannot read field {d.group().strip()!r}")
            for item in t.group(2).split(","):
                f = re.fullmatch(r"\s*(\*?)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", item)
                base = " ".join(t.group(1).split())
                if not f or f.group(2) in _TYPE_WORDS or base not in (_POINTEES if f and f.group(1) else _FIELD_SCALARS):
                    fail(m.start(2) + d.start(), f"{cname}: cannot map field {item.strip()!r} of type {base!r}")
                ct = C.c_void_p if f.group(1) else _FIELD_SCALARS[base]
                if f.group(3):
                    n = int(f.group(3)) if f.group(3).isdigit() else constants.get(f.group(3))
                    if not isinstance(n, int) or n <= 0:
                        fail(m.start(2) + d.start(), f"{cname}.{f.group(2)}: unknown array size {f.group(3)!r}")
                    ct = ct * n
                fields.append((f.group(2), ct))
        pyname = "".join(w.capitalize() for w in cname[4:].split("_"))
        structs[cname] = type(pyname, (C.Structure,), {"_fields_": fields, "__doc__": f"{cname} (include/tmf_hip.h)"})
        return blank(m)

    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", struct_of, text, flags=re.S)

    prototypes = {}
    for d in re.finditer(r"[^;]+", text):
        if not d.group().strip():
            continue
        pos = d.start() + len(d.group()) - len(d.group().lstrip())
        m = re.fullmatch(r"\s*([\w\s\*]+?)\b(tmf_\w+)\s*\(([^()]*)\)\s*", d.group())
        if not m:
            fail(pos, f"not a function declaration: {' '.join(d.group().split())[:80]!r}")
        name, args = m.group(2), []
        for p in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
            a = re.fullmatch(r"\s*(.*\S)\s*\b(\w+)\s*", p, flags=re.S)
            if not a or a.group(2) in _TYPE_WORDS:
                fail(pos, f"{name}: unnamed parameter {' '.join(p.split())!r}")
            args.append(ctype_of(pos, a.group(1), f"{name}, parameter {a.group(2)}"))
        prototypes[name] = (ctype_of(pos, m.group(1), f"{name}, return", is_return=True), args)
    return constants, structs, prototypes


with open(ABI_HEADER) as _f:
    CONSTANTS, STRUCTS, PROTOTYPES = parse_header(_f.read())
globals().update({k[4:]: v for k, v in CONSTANTS.items()})                  # TMF_POOL_MAX2 -> POOL_MAX2, ...
globals().update({s.__name__: s for s in STRUCTS.values()})                 # tmf_snet_desc -> SnetDesc, ...


_c = lambda name: CONSTANTS["TMF_" + name]
_POOL = {None: _c("POOL_NONE"), "none": _c("POOL_NONE"), "max": _c("POOL_MAX2"), "avg": _c("POOL_AVG2")}
PRECISION = {"fp32": _c("PREC_FP32"), "bf16": _c("PREC_BF16"), "fp32x": _c("PREC_FP32X")}     # tmf_snet_desc.precision


def snet_algo_wino(m: int) -> int:
    """TMF_SNET_ALGO_WINO(m): the conv_wino field of a tmf_snet_desc.flags word (a function-like macro, not parsed)."""
    return (m & 3) << 9


_names = lambda cname: tuple(n for n, _t in STRUCTS[cname]._fields_)
# the name tuples the ops iterate over, in the structs' own field order
HEADS_PARAMS = _names("tmf_heads_grads")
HEADS_BUFFERS = tuple(n for n in _names("tmf_heads_params") if n not in HEADS_PARAMS)
HEADS_CNN_PARAMS = _names("tmf_heads_cnn_grads")
XFORMER_PTRS = _names("tmf_xformer_params")[:_names("tmf_xformer_params").index("eps1")]

_lib = None


class TmfError(RuntimeError):
    pass


def load():
    """dlopen libtmf_hip.so (once) and attach prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("TMF_LIB", LIB_PATH)      # TMF_LIB: another build of the same library (kernel A/B runs)
    if not os.path.exists(path):
        raise TmfError(
            f"{path} is missing: build it with `python -m transmf_ad_amd.build` "
            "(hipcc --offload-arch=gfx950). transmf_ad_amd has no CPU or PyTorch fallback.")
    if "TMF_LIB" not in os.environ and os.environ.get("TMF_SKIP_STAMP_CHECK", "0") != "1":
        # a library built from other sources / other compile flags than the ones next to it must not run silently
        from . import build as _build
        try:
            with open(path + ".stamp") as f:
                stamp = f.read().strip()
        except OSError:
            stamp = None
        if stamp != _build.source_digest():
            raise TmfError(
                f"{path} is stale: it was not built from the current csrc/*.hip + headers + compile flags "
                "(stamp mismatch). Rebuild with `python -m transmf_ad_amd.build`.")
    lib = C.CDLL(path)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def pool_code(pool):
    return _POOL[pool]


def call(name, *args):
    """Call an int-returning entry point; raise TmfError with the library's message on failure."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.tmf_last_error_string()
        raise TmfError(f"{name} failed (rc={rc}): {msg.decode() if msg else ''}")


def query(name, *args):
    """Call a size/count query (no error code)."""
    return getattr(load(), name)(*args)
