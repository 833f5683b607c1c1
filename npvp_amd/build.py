"""Build libnpvp_hip.so (gfx950) in-tree from npvp_amd/csrc/*.hip with hipcc.

The shared object lives next to this file (npvp_amd/libnpvp_hip.so): it is git-ignored but
travels to the GPU box with the repo snapshot.  Incremental: a source is recompiled only when it
(or a header of csrc/, or include/npvp_hip.h) is newer than its object file.

include/npvp_hip.h is the one declaration of the C ABI: every source includes it (through csrc/common.h), so a definition that
disagrees with its prototype stops the build ("conflicting types"), and the generated call wrappers include it too.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")          # the public header npvp_hip.h
OBJ = os.path.join(CSRC, "obj")
LIB = os.path.join(HERE, "libnpvp_hip.so")
FAST = os.path.join(HERE, "_npvp_fast.so")          # CPython call wrappers of the same entry points (see build_fastcall)
ARCH = "gfx950"
FLAGS = ["-O3", "-fPIC", "-std=c++17", f"--offload-arch={ARCH}", "-fno-gpu-rdc", "-Wno-unused-result", f"-I{INCLUDE}"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.sep not in c or os.path.exists(c)):
            return c
    raise RuntimeError("hipcc not found")


def _newer(a, b):
    return (not os.path.exists(b)) or os.path.getmtime(a) > os.path.getmtime(b)


def build(force=False, verbose=True):
    os.makedirs(OBJ, exist_ok=True)
    srcs = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join(INCLUDE, "npvp_hip.h")]
    hipcc = _hipcc()
    jobs = []
    for s in srcs:
        src, obj = os.path.join(CSRC, s), os.path.join(OBJ, s[:-4] + ".o")
        if force or _newer(src, obj) or any(_newer(h, obj) for h in hdrs):
            jobs.append((src, obj))

    def cc(job):
        src, obj = job
        # NPVP_HIPCC_EXTRA: extra flags for one-off builds on the GPU box (e.g. -save-temps, -Rpass-analysis=kernel-resource-usage); never set
        # by the product build
        cmd = [hipcc] + FLAGS + os.environ.get("NPVP_HIPCC_EXTRA", "").split() + ["-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stderr}")
        if verbose:
            print(f"[npvp_amd.build] compiled {os.path.basename(src)}", file=sys.stderr)

    with ThreadPoolExecutor(max_workers=min(4, max(1, len(jobs)))) as ex:
        list(ex.map(cc, jobs))
    objs = [os.path.join(OBJ, s[:-4] + ".o") for s in srcs]
    stale = [f for f in os.listdir(OBJ) if f.endswith(".o") and os.path.join(OBJ, f) not in objs]
    for f in stale:                      # a source file was removed: its object must not linger in the library
        os.remove(os.path.join(OBJ, f))
    if force or jobs or stale or not os.path.exists(LIB) or any(_newer(o, LIB) for o in objs):
        # --no-undefined: a symbol dropped from one translation unit must fail HERE, not at first call on the GPU box
        cmd = [hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-Wl,--no-undefined", "-o", LIB] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr}")
        if verbose:
            print(f"[npvp_amd.build] linked {LIB}", file=sys.stderr)
    try:
        build_fastcall(verbose=verbose)
    except (OSError, RuntimeError) as e:
        # _npvp_fast is optional (npvp_amd._lib falls back to ctypes): no g++, or a compile / link error, must not fail the build
        # of the library itself.  A stale module generated for an older header must not be imported either.
        print(f"[npvp_amd.build] WARNING: the C-API call wrappers were not built ({e}); calls go through ctypes", file=sys.stderr)
        if os.path.exists(FAST):
            os.remove(FAST)
    return LIB


# how a wrapper reads an argument of each ctypes kind: (C variable, reader).  (LP64: ctypes.c_longlong IS ctypes.c_long, its
# __name__ is "c_long")
_ARG_READ = {"c_int": ("long long", "arg_ll"), "c_longlong": ("long long", "arg_ll"), "c_long": ("long long", "arg_ll"),
             "c_float": ("float", "arg_f"), "c_uint": ("unsigned int", "arg_u"), "c_void_p": ("void*", "arg_p")}


def fastcall_source():
    """C source of npvp_amd/_npvp_fast: one METH_FASTCALL wrapper per entry point of include/npvp_hip.h (as _lib parses it) that
    returns an int or a long long.  The source includes the header and casts every argument to the parameter type declared there,
    so the C++ compiler checks each call against the prototype the library itself was compiled against.
    ctypes converts every argument through its prototype machinery - 0.25 us per argument, 11 us for the 42 arguments
    of npvp_gemm_f32, 7 - 8 ms of a host-bound 8-clip step's 36 ms; these wrappers read the same Python ints / floats / None with
    the C API (~30 ns per argument) and call the SAME exported function of libnpvp_hip.so.  Argument meaning, order and the
    return value are those of the header; a wrong argument count or type raises TypeError."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_npvp_lib_sigs", os.path.join(HERE, "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = ["/* generated by npvp_amd/build.py from include/npvp_hip.h - do not edit */", "#define PY_SSIZE_T_CLEAN", "#include <Python.h>",
           "#include \"npvp_hip.h\"", "",
           "static inline int arg_ll(PyObject* o, long long* v) { *v = PyLong_AsLongLong(o); return !(*v == -1 && PyErr_Occurred()); }",
           "static inline int arg_u(PyObject* o, unsigned int* v) { unsigned long long t = PyLong_AsUnsignedLongLongMask(o); if (t == (unsigned long long)-1 && PyErr_Occurred()) return 0; *v = (unsigned int)t; return 1; }",
           "static inline int arg_f(PyObject* o, float* v) { double d = PyFloat_AsDouble(o); if (d == -1.0 && PyErr_Occurred()) return 0; *v = (float)d; return 1; }",
           "/* a pointer argument: None, an int (tensor.data_ptr(), ctypes.addressof) or a ctypes pointer object (its .value) */",
           "static int arg_p(PyObject* o, void** v) { if (o == Py_None) { *v = NULL; return 1; } if (!PyLong_Check(o)) { PyObject* val = PyObject_GetAttrString(o, \"value\"); if (!val) return 0; int ok = arg_p(val, v); Py_DECREF(val); return ok; } unsigned long long t = PyLong_AsUnsignedLongLongMask(o); if (t == (unsigned long long)-1 && PyErr_Occurred()) return 0; *v = (void*)(uintptr_t)t; return 1; }",
           ""]
    table = []
    for name, (res, args) in mod.SIGNATURES.items():
        rname = getattr(res, "__name__", "")
        if rname not in ("c_int", "c_longlong", "c_long"):
            continue
        rt, ctexts = mod.PROTOTYPES[name]
        out.append(f"static PyObject* w_{name}(PyObject* self, PyObject* const* a, Py_ssize_t n) {{")
        out.append(f"  if (n != {len(args)}) {{ PyErr_Format(PyExc_TypeError, \"{name} takes {len(args)} arguments (%zd given)\", n); return NULL; }}")
        call = []
        for i, (t, arg) in enumerate(zip(ctexts, args)):
            var, read = _ARG_READ[arg.__name__]
            out.append(f"  {var} v{i}; if (!{read}(a[{i}], &v{i})) return NULL;")
            call.append(f"({t})v{i}")
        out.append(f"  {rt} r;")
        out.append("  Py_BEGIN_ALLOW_THREADS")
        out.append(f"  r = {name}({', '.join(call)});")
        out.append("  Py_END_ALLOW_THREADS")
        out.append("  return PyLong_FromLongLong((long long)r);")
        out.append("}")
        table.append(name)
    out.append("static PyMethodDef methods[] = {")
    for name in table:
        out.append(f"  {{\"{name}\", (PyCFunction)(void(*)(void))w_{name}, METH_FASTCALL, \"{name} of include/npvp_hip.h\"}},")
    out.append("  {NULL, NULL, 0, NULL}};")
    out.append("static struct PyModuleDef moddef = {PyModuleDef_HEAD_INIT, \"_npvp_fast\", \"C-API call wrappers of libnpvp_hip.so\", -1, methods};")
    out.append("PyMODINIT_FUNC PyInit__npvp_fast(void) { return PyModule_Create(&moddef); }")
    return "\n".join(out) + "\n"


def build_fastcall(verbose=True):
    """npvp_amd/_npvp_fast.so next to the library (g++, links libnpvp_hip.so with an $ORIGIN rpath).  Optional: _lib falls back
    to ctypes when it is missing (the kernels are the same either way)."""
    import sysconfig
    inc = sysconfig.get_paths()["include"]
    if not os.path.exists(os.path.join(inc, "Python.h")):
        if verbose:
            print("[npvp_amd.build] Python.h not found: the ctypes binding stays the only one", file=sys.stderr)
        return None
    src = os.path.join(OBJ, "_npvp_fast.cpp")
    text = fastcall_source()
    if os.path.exists(src) and open(src).read() == text and os.path.exists(FAST) and not _newer(LIB, FAST):
        return FAST
    with open(src, "w") as f:
        f.write(text)
    cmd = ["g++", "-O2", "-fPIC", "-shared", "-std=c++17", f"-I{inc}", f"-I{INCLUDE}", src, "-o", FAST, f"-L{HERE}", "-l:libnpvp_hip.so",
           "-Wl,-rpath,$ORIGIN"]          # (Python's own symbols come from the interpreter, as for every extension module)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"building {FAST} failed:\n{r.stderr}")
    if verbose:
        print(f"[npvp_amd.build] built {FAST}", file=sys.stderr)
    return FAST


if __name__ == "__main__":
    build(force="--force" in sys.argv)
