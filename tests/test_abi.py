"""CPU: the C-ABI library builds/loads and exports every symbol include/npvp_hip.h declares; the product
package fails loudly (no CPU fallback) and never imports the oracle."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from npvp_amd import build
    return build.build(verbose=False)


def test_header_symbols_exported(built):
    from npvp_amd._lib import lib, SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "npvp_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(npvp_[a-z0-9_]+)\s*\(", hdr))
    assert len(names) >= 25
    L = lib()
    for n in sorted(names):
        assert hasattr(L, n), f"{n} declared in include/npvp_hip.h but not exported"
        assert n in SIGNATURES, f"{n} has no ctypes signature in npvp_amd/_lib.py"
    assert set(SIGNATURES) <= names
    assert L.npvp_version() >= 100


def _dynamic_defined_symbols(path):
    """names of the dynamic defined symbols of a shared object, read with the binary tools of the hipcc in use: llvm-nm beside hipcc
    or beside its clang; where the toolchain ships no llvm-nm, the llvm-readelf of the same directory"""
    import shutil
    import subprocess
    from npvp_amd import build
    hipcc = shutil.which(build._hipcc())
    clang = subprocess.run([hipcc, "--print-prog-name=clang"], capture_output=True, text=True).stdout.strip()
    dirs = [os.path.dirname(os.path.realpath(hipcc))] + ([os.path.dirname(os.path.realpath(clang))] if os.path.sep in clang else [])
    for tool, args, defined in (("llvm-nm", ["-D", "--defined-only", "--format=posix"], lambda f: f[0] if len(f) >= 2 else None),
                                ("llvm-readelf", ["--dyn-syms", "-W"],
                                 lambda f: f[7].split("@")[0] if len(f) == 8 and f[0].rstrip(":").isdigit() and f[6] != "UND" else None)):
        for d in dirs:
            if os.path.exists(os.path.join(d, tool)):
                out = subprocess.run([os.path.join(d, tool)] + args + [path], capture_output=True, text=True, check=True).stdout
                return {n for n in (defined(line.split()) for line in out.splitlines()) if n}
    raise AssertionError(f"neither llvm-nm nor llvm-readelf in {dirs}")


def test_c_linkage_exports_are_exactly_the_header(built):
    """The library's dynamic defined symbols that start with npvp_ (C linkage: C++-mangled names start with _Z and are not counted)
    are the names include/npvp_hip.h declares - nothing internal leaks into the C export list, nothing declared is missing."""
    from npvp_amd import _lib
    exported = {n for n in _dynamic_defined_symbols(built) if n.startswith("npvp_")}
    declared = set(_lib.PROTOTYPES)
    assert len(declared) == len(_lib.SIGNATURES) >= 106
    assert exported - declared == set(), "exported with C linkage but not declared in include/npvp_hip.h"
    assert declared - exported == set(), "declared in include/npvp_hip.h but not exported"


def test_header_parser_reads_comments_multiline_and_void():
    import ctypes
    from npvp_amd import _lib
    protos = _lib.parse_header("""
/* a header
 * int npvp_in_a_comment(int x); */
#ifndef X
#define X
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef struct ihipStream_t* npvp_stream_t; /* == hipStream_t */
typedef struct npvp_rec { const float* a; int b, c; } npvp_rec_t;   /* plain data */
int npvp_a(void);
const char* npvp_b(void);  // trailing comment
void* npvp_c(int* least,
             int *greatest);
float npvp_d(void* e0, void* e1);
long long npvp_e(const float* x /* nullable */, long long rows, size_t n, unsigned int salt,
                 const unsigned long long* seed, float p /* in [0, 1) */,
                 npvp_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
""")
    assert protos == {"npvp_a": ("int", []), "npvp_b": ("const char*", []), "npvp_c": ("void*", ["int*", "int*"]),
                      "npvp_d": ("float", ["void*", "void*"]),
                      "npvp_e": ("long long", ["const float*", "long long", "size_t", "unsigned int", "const unsigned long long*", "float",
                                               "npvp_stream_t"])}
    sig = _lib.signatures(protos)
    P = ctypes.c_void_p
    # the four return kinds that stay with ctypes or are wrapped: int / long long, const char*, void*, float
    assert sig["npvp_a"] == (ctypes.c_int, []) and sig["npvp_b"] == (ctypes.c_char_p, [])
    assert sig["npvp_c"] == (P, [P, P]) and sig["npvp_d"] == (ctypes.c_float, [P, P])
    assert sig["npvp_e"][0] is ctypes.c_longlong
    assert all(x is y for x, y in zip(sig["npvp_e"][1], [P, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_uint, P, ctypes.c_float, P]))


@pytest.mark.parametrize("proto, named", [
    ("int npvp_x(double eps);", "double"),                       # a value type outside the map
    ("int npvp_x(int n, unsigned long long seed);", "unsigned long long"),
    ("double npvp_x(int n);", "double"),                         # ... as a return
    ("float* npvp_x(int n);", "float*"),                         # a pointer return other than const char* / void*
    ("npvp_stream_t npvp_x(void);", "npvp_stream_t"),
    ("int npvp_x(int);", "int"),                                 # a parameter without a name
    ("int npvp_x(int (*cb)(int));", "npvp_x"),                   # not `type name`
    ("int npvp_x(int n)", "npvp_x"),                             # no terminating semicolon
    ("int npvp_x(int n); int npvp_x(int n);", "npvp_x"),         # declared twice
    ("int g_counter;", "g_counter"),                             # not a prototype
])
def test_header_parser_is_strict(proto, named):
    """Whatever the type map or the prototype grammar does not cover raises at import and names the prototype or the type."""
    from npvp_amd import _lib
    with pytest.raises(RuntimeError, match=re.escape(named)):
        _lib.signatures(_lib.parse_header(proto))


def test_argument_errors_do_not_need_a_gpu(built):
    """Bad arguments are rejected on the host before any launch, with a message."""
    from npvp_amd._lib import lib
    L = lib()
    rc = L.npvp_gemm_f32(1, 1, 128, 128, 33, None, 36, None, 36, None, 128, None, 0, None, None, None, 0, 0.0, 0, 1, 1,
                         None, 0, 1.0, 0, None, None, 0, None, None, None, None, None, 0.0, 1, 1, 0, None, 0, None)
    assert rc == -1 and b"multiple of 32" in L.npvp_last_error()
    assert L.npvp_layernorm_fwd(None, None, None, None, None, None, 4, 500, 1e-5, 0, None, None) == -1
    assert L.npvp_attn_fwd(None, 512, None, 512, None, 512, None, 512, 1, 1, 64, 8, 0, 200, 200, 8, 64, 0, 0.0, None, 0, None, None) == -1
    assert b"[1,128]" in L.npvp_last_error()            # (sequence lengths 33 .. 128 are legal since round 5: the generic kernels)
    assert L.npvp_gemm_workspace_bytes(2048, 512, 20480) > 0 and L.npvp_gemm_workspace_bytes(20480, 512, 512) == 0
    # round 6: the scalar losses and the graph node census
    assert L.npvp_l1_mean(None, None, 16, 1.0, None, None, 0, None) == -1 and b"l1_mean" in L.npvp_last_error()
    assert L.npvp_l1_mean_bwd(None, None, 16, None, 1.0, None, None) == -1
    assert L.npvp_sum_all(None, 0, None, None, 0, None) == -1 and b"sum_all" in L.npvp_last_error()
    assert L.npvp_graph_node_counts(None, None, None, 0) == -1 and b"graph_node_counts" in L.npvp_last_error()


def test_c_api_wrappers_cover_the_abi_and_agree_with_ctypes(built):
    """npvp_amd/_npvp_fast (generated from _lib.SIGNATURES, built next to the library) wraps every entry point that returns an
    int / long long; on the host-side argument checks it returns what the ctypes binding returns, it takes ints, None and ctypes
    pointer objects for pointers, and it raises TypeError on a wrong argument count or type."""
    import ctypes
    from npvp_amd import _lib
    from npvp_amd import _npvp_fast as F
    L = _lib.lib()
    raw = L._cdll
    missing = [n for n in _lib.SIGNATURES if not hasattr(F, n)]
    # (char* / pointer / float returns stay with ctypes)
    assert missing == ["npvp_last_error", "npvp_stream_create_low_priority", "npvp_event_create", "npvp_event_elapsed_ms"], missing
    assert L._fast == len(_lib.SIGNATURES) - 4 and L.npvp_gemm_f32 is F.npvp_gemm_f32
    calls = [("npvp_gemm_f32", (1, 1, 128, 128, 33, None, 36, None, 36, None, 128, None, 0, None, None, None, 0, 0.0, 0, 1, 1, None, 0,
                                1.0, 0, None, None, 0, None, None, None, None, None, 0.0, 1, 1, 0, None, 0, None)),
             ("npvp_layernorm_fwd", (None, None, None, None, None, None, 4, 500, 1e-5, 0, None, None)),
             ("npvp_layernorm_fwd", (ctypes.c_void_p(0), None, None, None, None, None, 4, 500, 1e-5, 0, None, ctypes.c_void_p(0))),
             ("npvp_gemm_workspace_bytes", (2048, 512, 20480)), ("npvp_gemm_kernel_id", (1, 1, 114688, 512, 512, 6, 1)),
             ("npvp_gemm_kernel_id", (True, 1, 8192, 512, 512, 6, 0))]
    for name, args in calls:
        assert getattr(F, name)(*args) == getattr(raw, name)(*args), name
    with pytest.raises(TypeError):
        F.npvp_gemm_kernel_id(1, 1, 512)
    with pytest.raises(TypeError):
        F.npvp_gemm_kernel_id(1, 1, "512", 512, 512, 6, 1)
    with pytest.raises((TypeError, AttributeError)):
        F.npvp_layernorm_fwd("x", None, None, None, None, None, 4, 500, 1e-5, 0, None, None)


def test_row_group_magic_division_is_exact(tmp_path):
    """csrc/common.h div_magic: the multiply-shift the kernels use for (row / g1) % g2 of a DropPath site - host-compiled from the
    header itself and compared with `/` for every numerator class that matters (dense low range, multiples of d and their
    predecessors, the top of the 31-bit range, random pairs)."""
    import subprocess
    src = tmp_path / "div_magic_check.hip"
    src.write_text(r'''#include "common.h"
#include <cstdio>
#include <cstdlib>
int main() {
  unsigned ds[] = {1, 2, 3, 5, 7, 13, 16, 28, 64, 100, 448, 1792, 1793, 4096, 65535, 65536, 65537, 114688, 1000003, 1u << 30, (1u << 30) + 1, 0x7fffffffu};
  for (unsigned d : ds) {
    unsigned m; int s;
    npvp::div_magic(d, m, s);
    for (unsigned long long n = 0; n < (1ull << 31); n += (n < 70000 ? 1 : 9973))
      if ((unsigned)((n * m) >> s) != (unsigned)(n / d)) { printf("BAD d=%u n=%llu\n", d, n); return 1; }
    for (unsigned long long k = 1; k < 3000; ++k)
      for (int o = -1; o <= 0; ++o) { unsigned long long x = k * d + o; if (x < (1ull << 31) && (unsigned)((x * m) >> s) != (unsigned)(x / d)) { printf("BAD d=%u n=%llu\n", d, x); return 1; } }
    unsigned long long x = (1ull << 31) - 1;
    if ((unsigned)((x * m) >> s) != (unsigned)(x / d)) { printf("BAD top d=%u\n", d); return 1; }
  }
  srand(1);
  for (int t = 0; t < 300000; ++t) {
    unsigned d = (unsigned)(rand() % 2000000) + 1, m; int s;
    npvp::div_magic(d, m, s);
    unsigned long long n = (((unsigned long long)rand() << 16) ^ rand()) & 0x7fffffff;
    if ((unsigned)((n * m) >> s) != (unsigned)(n / d)) { printf("BAD rnd d=%u n=%llu\n", d, n); return 1; }
  }
  printf("ok\n");
  return 0;
}
''')
    exe = tmp_path / "div_magic_check"
    csrc = os.path.join(ROOT, "npvp_amd", "csrc")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_mask_hash_statistics_on_the_host(tmp_path):
    """csrc/common.h rng_u32 (two keyed finalizer rounds per element), host-compiled from the header: on sequential and strided
    counters (row stride 512 / 2048, column walks) the top, middle and low byte are uniform (chi-square per degree of freedom
    within 0.75 .. 1.3), keep rates at p = 0.1 / 0.5 sit within 4.5 sigma, masks of different sites (salts) and steps (seeds) and
    lagged copies of one mask are uncorrelated within 4.5 sigma.  (tests/test_hip_dropout.py::test_mask_statistics repeats the
    mask part through the kernels.)"""
    import subprocess
    import numpy as np
    src = tmp_path / "hash_dump.hip"
    src.write_text(r'''#include "common.h"
#include <cstdio>
#include <cstdlib>
// usage: prog seed salt stride offset count  -> count raw 32-bit hashes of idx = offset + i * stride on stdout
int main(int argc, char** argv) {
  const unsigned long long seed = strtoull(argv[1], nullptr, 0), stride = strtoull(argv[3], nullptr, 0), off = strtoull(argv[4], nullptr, 0);
  const unsigned int salt = (unsigned int)strtoul(argv[2], nullptr, 0);
  const long n = atol(argv[5]);
  unsigned int* buf = (unsigned int*)malloc(n * 4);
  for (long i = 0; i < n; ++i) buf[i] = npvp::rng_u32(seed, salt, off + (unsigned long long)i * stride);
  fwrite(buf, 4, n, stdout);
  return 0;
}
''')
    exe = tmp_path / "hash_dump"
    csrc = os.path.join(ROOT, "npvp_amd", "csrc")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    n = 1 << 21

    def hashes(seed, salt, stride=1, off=0):
        out = subprocess.run([str(exe), str(seed), str(salt), str(stride), str(off), str(n)], capture_output=True, timeout=120)
        assert out.returncode == 0
        return np.frombuffer(out.stdout, dtype=np.uint32)

    seed0 = 0x1E3779B97F4A7C15
    for stride, off in [(1, 0), (512, 3), (2048, 5), (4, 1), (114688, 0)]:
        for k in range(2):
            h = hashes(seed0 + k * 0x632BE5AB, 3 + k, stride, off)
            for shift in (24, 12, 0):
                c = np.bincount((h >> shift) & 255, minlength=256)
                chi = float(((c - n / 256.0) ** 2 / (n / 256.0)).sum() / 255.0)
                assert 0.75 < chi < 1.3, f"stride {stride}, byte at bit {shift}: chi-square / dof {chi:.2f}"
    sig = 1.0 / np.sqrt(n)
    for p in (0.1, 0.5):
        thr = int(p * 4294967296.0)
        masks = [(hashes(seed0 + k * 0x632BE5AB, s) >= thr).astype(np.float64) for k in range(3) for s in (1, 2, 50)]
        for m in masks:
            assert abs(m.mean() - (1 - p)) < 4.5 * np.sqrt(p * (1 - p)) * sig
        z = [(m - m.mean()) / m.std() for m in masks]
        for i in range(len(z)):
            for j in range(i + 1, len(z)):
                assert abs((z[i] * z[j]).mean()) < 4.5 * sig, f"p={p}: masks {i}, {j} correlate"
        for lag in (1, 2, 3, 4, 8, 64, 512, 2048, 4096):
            assert abs((z[0][:-lag] * z[0][lag:]).mean()) < 4.5 * sig, f"p={p}: lag {lag}"


def test_window_row_quotient_in_fp32_is_exact():
    """csrc/attn.hip attn_row takes m / ws for the rows of a local window as (int)((m + 0.5f) * (1.f / ws)) - restated here in numpy
    float32: exact for every window side up to 32 and every row index a window of that side can have (and far beyond)."""
    import numpy as np
    m = np.arange(0, 4096, dtype=np.int64)
    for ws in range(1, 33):
        inv = np.float32(1.0) / np.float32(ws)
        q = ((m.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int64)
        assert np.array_equal(q, m // ws), f"ws = {ws}: first mismatch at m = {int(m[q != m // ws][0])}"


def test_no_cpu_fallback():
    import npvp_amd
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        npvp_amd.ops.layernorm(torch.zeros(4, 512), torch.ones(512), torch.zeros(512))
    m = npvp_amd.MlpDWBN(8, 8, 512, 2048, 512)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 1, 8, 8, 512))


def test_product_never_imports_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "npvp_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f"{f} imports the oracle"


def test_state_dict_keys_match_oracle():
    import npvp_amd, oracle
    h = torch.linspace(0, 7, 8)
    args = (8, 8, 20, h, h, torch.linspace(0, 9, 10), torch.linspace(10, 19, 10), 512, 'Add', 'layer', 256, 1, True, 8)
    kw = dict(evt_former=True, learn_evt_token=False, evt_former_num_layers=4)
    a, b = oracle.Predictor(*args, **kw), npvp_amd.Predictor(*args, **kw)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys()) and len(b.state_dict()) == 603
    assert all(x.shape == y.shape for x, y in zip(a.state_dict().values(), b.state_dict().values()))


def test_lr_schedule_matches_torch():
    import npvp_amd
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.AdamW([p], lr=1e-4)
    sch = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, 150, T_mult=1, eta_min=1e-7)
    for e in (0.0, 0.37, 12.5, 149.99, 150.0, 151.25, 449.5):
        sch.step(e)
        assert abs(opt.param_groups[0]["lr"] - npvp_amd.cosine_warm_restarts_lr(1e-4, 1e-7, 150, e)) < 1e-12


def test_context_modes_host_logic():
    """VFI / random-context batch shaping (ref/models/Predictor.py:30-40,241-259, ref/utils/dataset.py:162-178)."""
    import npvp_amd
    P = {"VFI": True, "context_num_p": 2, "context_num_f": 2, "num_interpolate": 3}
    to, tp = npvp_amd.context_lists(P, 4, 3)
    assert to.tolist() == [0, 1, 5, 6] and tp.tolist() == [2, 3, 4]
    to2, tp2 = npvp_amd.context_lists({"VFI": False}, 3, 2)
    assert to2.tolist() == [0.0, 1.0, 2.0] and tp2.tolist() == [3.0, 4.0]
    past, fut = torch.arange(4).view(1, 4, 1).float(), torch.arange(4, 7).view(1, 3, 1).float()
    ctx, tgt = npvp_amd.vfi_batch_process((past, fut), to, tp)
    assert ctx.flatten().tolist() == [0, 1, 5, 6] and tgt.flatten().tolist() == [2, 3, 4]
    clip = torch.arange(10).view(1, 10, 1).float().repeat(3, 1, 1)
    g = torch.Generator().manual_seed(5)
    co, cp, io, ip = npvp_amd.rand_context_collate(clip, 4, 6, generator=g)
    assert 4 <= io.numel() <= 6 and io.numel() + ip.numel() == 10
    assert sorted(io.tolist() + ip.tolist()) == list(range(10))
    assert co[0].flatten().tolist() == [float(i) for i in io.tolist()] and cp.shape == (3, ip.numel(), 1)
    # the unified predictor keeps every (t,h,w) coordinate and lets the harness choose rows per batch
    h = torch.linspace(0, 7, 8)
    tl = torch.linspace(0, 6, 7)
    m = npvp_amd.Predictor(8, 8, 7, h, h, tl[:3], tl[3:], 512, 'Add', 'layer', 256, 1, False, 1, evt_former_num_layers=1,
                           rand_context=True)
    assert m.observed_coor is None and m.all_coor.shape == (7, 8, 8, 3)
    npvp_amd.rand_context_batch_process(m, (None, None, torch.tensor([6, 1]), torch.tensor([0, 3, 2])))
    assert m.observed_coor.shape == (2 * 64, 3) and m.predict_coor.shape == (3 * 64, 3) and m.TP == 3
    assert torch.equal(m.observed_coor[:64], m.all_coor[6].flatten(0, 1))


def test_lightning_checkpoint_wire_format(tmp_path):
    """A checkpoint in the reference's layout (state_dict keys prefixed predictor. / VPTR_Enc. / VPTR_Dec.,
    ref/models/Predictor.py:17-19,43) written by torch.save loads into the HIP-backed modules and round-trips."""
    import npvp_amd
    import oracle
    from oracle import ops as O
    h = torch.linspace(0, 7, 8)
    mk = lambda cls: cls(8, 8, 5, h, h, torch.linspace(0, 1, 2), torch.linspace(2, 4, 3), 512, 'Add', 'layer', 256, 1, True, 1,
                         evt_former_num_layers=1)
    src = mk(oracle.Predictor)                       # stands in for a reference-trained predictor (same 603-key layout rules)
    O.key_hashed_fill(src, 7)
    enc, dec = npvp_amd.build_frozen_autoencoder({"ngf": 8, "n_downsampling": 3, "num_res_blocks": 1, "out_layer": "Tanh",
                                                  "learn_3d": False}, 1)
    sd = {"predictor." + k: v for k, v in src.state_dict().items()}
    sd.update({"VPTR_Enc." + k: v for k, v in enc.state_dict().items()})
    sd.update({"VPTR_Dec." + k: v for k, v in dec.state_dict().items()})
    path = str(tmp_path / "ref_style.ckpt")
    torch.save({"state_dict": sd, "epoch": 12, "global_step": 3400}, path)
    dst = mk(npvp_amd.Predictor)
    enc2, dec2 = npvp_amd.build_frozen_autoencoder({"ngf": 8, "n_downsampling": 3, "num_res_blocks": 1, "out_layer": "Tanh",
                                                    "learn_3d": False}, 1)
    assert npvp_amd.load_lightning_checkpoint(path, dst, enc2, dec2) == (12, 3400)
    for k, v in src.state_dict().items():
        assert torch.equal(dst.state_dict()[k], v), k
    assert dst.EVT_Former.norm.weight is dst.transformer.norm.weight          # still tied after loading
    path2 = str(tmp_path / "ours.ckpt")
    npvp_amd.save_lightning_checkpoint(path2, dst, enc2, dec2, epoch=13, global_step=3500)
    ck = torch.load(path2, weights_only=False)
    assert set(ck["state_dict"]) == set(sd) and ck["epoch"] == 13
    back = mk(oracle.Predictor)
    back.load_state_dict({k[len("predictor."):]: v for k, v in ck["state_dict"].items() if k.startswith("predictor.")})


def test_range_guard_fallback_is_retried_and_backs_off():
    """sched.RangeGuardState: a range event arms the bf16x6 fallback of THIS trainer; after `retry_after` clean polls
    the fp16 weight gradients are tried again; an event within PROBATION polls of a retry doubles the interval, a clean probation
    resets it.  Pure host logic: driven here with a CPU word in place of the device counter."""
    from npvp_amd import sched
    g = sched.RangeGuardState(None)
    g.RETRY_AFTER, g.PROBATION = 4, 2
    g.retry_after = 4
    f = torch.zeros(1, dtype=torch.int32)
    assert g._note(f, 0) == 0 and not g.fallback
    f[0] = 3
    assert g._note(f, 3) == 3 and g.fallback and g.events == 3 and int(f[0]) == 0
    for _ in range(3):
        g._note(f, 0)
        assert g.fallback
    g._note(f, 0)
    assert not g.fallback and g._probation == 2                 # the retry
    g._note(f, 1)                                               # ... and the event is back at once
    assert g.fallback and g.retry_after == 8 and g.events == 4
    for _ in range(8):
        assert g.fallback
        g._note(f, 0)
    assert not g.fallback
    g._note(f, 0); g._note(f, 0)                                # a clean probation
    assert g._probation == 0 and g.retry_after == 4 and not g.fallback
    g.reset()
    assert g.events == 0 and g.retry_after == g.RETRY_AFTER


def test_import_selects_the_safe_graph_replay_mode():
    """`import npvp_amd` puts DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 into the environment (the ROCm 7.2 packet-capture replay path computes
    wrong steps for this workload: DESIGN 7) unless NPVP_GRAPH_PACKET_CAPTURE=1 asks for the runtime's default, and never overrides a
    value the caller set.  Run in fresh interpreters: the variable only matters before the HIP runtime initialises."""
    import subprocess, sys
    code = "import os, npvp_amd; print(os.environ.get('DEBUG_CLR_GRAPH_PACKET_CAPTURE'), npvp_amd.graph_packet_capture())"
    def run(**env):
        e = {k: v for k, v in os.environ.items() if k not in ("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "NPVP_GRAPH_PACKET_CAPTURE")}
        e.update(env)
        return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300).stdout.split()
    assert run() == ["0", "False"]
    assert run(NPVP_GRAPH_PACKET_CAPTURE="1") == ["None", "True"]
    assert run(DEBUG_CLR_GRAPH_PACKET_CAPTURE="1") == ["1", "True"]


def test_bench_takes_the_replay_of_a_host_bound_step_unless_eager_clearly_wins():
    """bench.py's mode rule restated on its numbers: the driver record of round 5 (eager trial 30.2 ms with 33 ms of
    host per step, replay 31.7 ms) must come out as the REPLAY; a GPU-bound step keeps whichever is faster."""
    import ast
    src = open(os.path.join(ROOT, "bench.py")).read()
    fn = next(n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef) and n.name == "prefer_replay")
    ns = {}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "bench.py", "exec"), ns)
    prefer = ns["prefer_replay"]
    assert prefer(30.23, 33.5, 31.68) is True             # round 5's driver box: host bound, eager only 4.6 % ahead in the trial
    assert prefer(29.0, 28.0, 31.0) is False              # host bound, but eager wins by more than 5 %
    assert prefer(230.0, 34.0, 236.0) is False            # not host bound: the rule does not apply (the caller compares the times)
    assert prefer(30.0, 29.0, None) is False              # the capture failed
