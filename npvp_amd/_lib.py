"""ctypes binding of libnpvp_hip.so.  include/npvp_hip.h is the one declaration of the C ABI: the library is compiled against it,
and SIGNATURES below is parsed from it at import (there is no hand-written table to keep in step).  There is NO fallback: if the
shared object or the header is missing or a call fails, a RuntimeError is raised - the product path never computes on the CPU or
through torch ops in place of a HIP kernel."""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnpvp_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "npvp_hip.h")

# C type of a value parameter or return -> ctypes type (size_t: LP64).  Every pointer parameter and npvp_stream_t is a c_void_p.
# A type the header uses and this map does not cover is an error: extending the ABI's vocabulary is an edit here.
c_int, c_ll, c_f, c_u, c_p = ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_uint, ctypes.c_void_p
_VALUE_TYPES = {"int": c_int, "long long": c_ll, "size_t": c_ll, "float": c_f, "unsigned int": c_u}
_RETURN_TYPES = dict(_VALUE_TYPES, **{"const char*": ctypes.c_char_p, "void*": c_p})
_VALUE_TYPES["npvp_stream_t"] = c_p


def parse_header(text):
    """{name: (C return type, [C parameter types])} of every prototype in the text of a header written like include/npvp_hip.h:
    comments, preprocessor lines, the extern "C" braces and typedefs are dropped, and every statement left must be a prototype
    `type name(type name, ...)` or `type name(void)` - anything else raises."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    text = re.sub(r"\btypedef\b[^;{]*(\{[^}]*\}[^;{]*)?;", " ", text)
    *statements, tail = text.split(";")
    if tail.strip() not in ("", "}"):
        raise RuntimeError(f"npvp_hip.h: unterminated text after the last prototype: {tail.strip()!r}")
    protos = {}
    for st in statements:
        st = " ".join(st.split())
        m = re.fullmatch(r"([\w\s]+?[\s*]+)(npvp_\w+) ?\((.*)\)", st)
        if not m or m.group(2) in protos:
            raise RuntimeError(f"npvp_hip.h: not a prototype, or declared twice: {st!r}")
        params = []
        for p in ([] if m.group(3).strip() == "void" else m.group(3).split(",")):
            pm = re.fullmatch(r"\s*([\w\s]+?[\s*]+)\w+\s*", p)
            if not pm:
                raise RuntimeError(f"npvp_hip.h: parameter {p.strip()!r} of {m.group(2)} is not `type name`: {st!r}")
            params.append(re.sub(r"\s*\*\s*", "*", pm.group(1)).strip())
        protos[m.group(2)] = (re.sub(r"\s*\*\s*", "*", m.group(1)).strip(), params)
    return protos


def signatures(protos):
    """{name: (restype, [argtypes])} for ctypes from parse_header's result; a type outside the maps above raises and names the prototype."""
    out = {}
    for name, (ret, params) in protos.items():
        unmapped = [t for t in params if not t.endswith("*") and t not in _VALUE_TYPES] + [ret] * (ret not in _RETURN_TYPES)
        if unmapped:
            raise RuntimeError(f"npvp_hip.h: {name}: no ctypes mapping for C type {unmapped[0]!r} (npvp_amd/_lib.py _VALUE_TYPES / _RETURN_TYPES)")
        out[name] = (_RETURN_TYPES[ret], [c_p if t.endswith("*") else _VALUE_TYPES[t] for t in params])
    return out


if not os.path.exists(HEADER_PATH):
    raise RuntimeError(f"{HEADER_PATH} is missing - npvp_amd reads the C ABI of libnpvp_hip.so from the public header of its "
                       "repository tree. npvp_amd has no CPU fallback.")
with open(HEADER_PATH) as _f:
    PROTOTYPES = parse_header(_f.read())     # name -> (C return type, [C parameter types]); build.py casts to these
SIGNATURES = signatures(PROTOTYPES)          # name -> (restype, argtypes)

_lib = None


def bind(cdll, names=SIGNATURES):
    """give the named entry points of a loaded library (all of them by default) the header's restype / argtypes; returns cdll"""
    for name in names:
        fn = getattr(cdll, name)          # AttributeError here = header/library mismatch
        fn.restype, fn.argtypes = SIGNATURES[name]
    return cdll


def lib():
    """Load (once) and return the bound library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing - the HIP extension has not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `python npvp_amd/build.py`). "
                "npvp_amd has no CPU fallback.")
        L = bind(ctypes.CDLL(LIB_PATH, mode=os.RTLD_NOW))        # resolve every symbol now: a broken build fails here
        bound = _Bound()
        for name in SIGNATURES:
            setattr(bound, name, getattr(L, name))
        bound._cdll = L
        # The same entry points through C-API wrappers (npvp_amd/_npvp_fast.so, generated by build.py from the same header): ctypes spends
        # ~0.25 us per argument on its prototype machinery - 7 - 8 ms of a host-bound 8-clip step.  Same functions of the same
        # library, same arguments, same return values; NPVP_FASTCALL=0 keeps ctypes (A/B runs), and so does a missing module.
        bound._fast = 0
        if os.environ.get("NPVP_FASTCALL", "1") == "1":
            try:
                from . import _npvp_fast as F
            except ImportError as e:
                import warnings
                warnings.warn(f"npvp_amd._npvp_fast is not built ({e}): every call goes through ctypes (same kernels, more host time)")
            else:
                for name in SIGNATURES:
                    f = getattr(F, name, None)
                    if f is not None:
                        setattr(bound, name, f)
                        bound._fast += 1
        _lib = bound
    return _lib


class _Bound:
    """the bound entry points of libnpvp_hip.so as plain attributes (C-API wrapper where there is one, ctypes function otherwise)"""


def check(rc, what):
    if rc != 0:
        msg = lib().npvp_last_error()
        raise RuntimeError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")
