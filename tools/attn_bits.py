"""A fingerprint of the attention entry points (csrc/attn.hip): npvp_attn_fwd / _bwd, npvp_attn_long_fwd / _bwd and
npvp_attn_samples_fwd through the C ABI only, on seeded inputs, every output buffer pre-filled with a sentinel, one SHA-256 per case over
every output (o, dq, dk, dv, the amax slots as the kernels leave them, the streaming backward's statistics workspace).  Two builds of
the library that print the same lines compute the same bits: run it before and after a change of these entry points or their kernels
that is meant to move none.  Needs a GPU.

The cases are the smallest that reach every kernel instantiation and every ragged edge: 2 heads (C = 128); temporal geometry with
N = 1, P = 3 (6 waves: the last 4-wave block of the MFMA kernels is ragged), every case with dropout off and with p = 0.1 under a
fixed seed and salt, the encoder mask on where Tq = Tk; spatial windows on two frames with q | k (and dq | dk) packed in one buffer
of row stride 2C; the sampler's kernel at S = 3, N = 2 with the library's chunk and a ragged forced one.

    python tools/attn_bits.py [--lib path/to/libnpvp_hip.so]
    python tools/attn_bits.py --time --lib parent.so --lib change.so [--lib copy_of_parent.so]

--time: the libraries in ONE process, alternated, at the workload's sizes (N = 64 clips, P = 64 pixels, 8 heads: the c2 shapes of
tools/attn_bench.py, the generic / streaming kernels at 40 and 128 rows, the sampler at tools/sample_bench.py's BAIR shape): 0.5 s of
warm-up, then medians of 7 interleaved rounds per library (the method of tools/attn_bench.py --long).  With a byte copy of the first
library as the third, the largest relative difference between the two copies over all cases is the spread of the method, and the
last column says whether the second library's median is within that spread of the first's."""
import argparse
import ctypes
import hashlib
import os
import statistics
import sys
import time

import torch                      # (before the library: both must use the HIP runtime that torch loads)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from npvp_amd import _lib  # noqa: E402  (the argument types of include/npvp_hip.h; the libraries are the ones --lib names)

NAMES = ("npvp_attn_fwd", "npvp_attn_bwd", "npvp_attn_long_fwd", "npvp_attn_long_bwd", "npvp_attn_long_bwd_workspace_bytes",
         "npvp_attn_samples_fwd", "npvp_last_error")
HD, SALT, SEED = 64, 77, 0x9E3779B97F4A7C15 >> 1
DROPS = (0.0, 0.1)
SHORT = [(1, 1), (3, 3), (16, 16), (10, 28), (18, 2), (17, 17), (28, 28), (32, 32)]      # <1,1> x3, <1,2>, <2,1>, <2,2> x3
GENERIC = [(33, 33), (48, 5), (5, 40), (128, 128)]
STREAM = [(10, 10), (64, 64), (65, 65), (130, 2), (5, 150), (137, 137)]
WINDOWS = [(3, 6, 9, False), (5, 10, 5, False), (4, 8, 8, False), (8, 8, 8, False), (8, 8, 8, True)]     # (ws, H, W, streaming)
SAMPLES = [(4, 3), (18, 2), (10, 28), (28, 28)]


def load(path):
    return _lib.bind(ctypes.CDLL(path), NAMES)


class Case:
    """the buffers of one forward + backward call: mode 1 (temporal, dim0 clips, separate q / k / v) or mode 0 (dim0 frames of an
    H x W grid, q | k packed with row stride 2C, dq | dk likewise)"""

    def __init__(self, mode, dim0, heads, P, W, ws, Tq, Tk, mask, p, seed, clips_q=None, rng="cpu"):
        self.mode, self.dim0, self.heads, self.P, self.W, self.ws, self.Tq, self.Tk, self.mask, self.p = mode, dim0, heads, P, W, ws, Tq, Tk, mask, p
        C = self.C = heads * HD
        rq, rk = (dim0 * P, dim0 * P) if mode == 0 else ((clips_q or dim0) * Tq * P, dim0 * Tk * P)
        gen = torch.Generator(device=rng).manual_seed(seed)         # (the fingerprint's inputs come from the CPU generator)
        rnd = lambda *s: torch.randn(*s, generator=gen, device=rng).cuda()
        new = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device="cuda")   # (an element no kernel writes is hashed as this)
        if mode == 0:
            self.qk, self.dqk = rnd(rq, 2 * C), new(rq, 2 * C)
            self.q = (self.qk.data_ptr(), 2 * C); self.k = (self.qk.data_ptr() + 4 * C, 2 * C)
            self.dq = (self.dqk.data_ptr(), 2 * C); self.dk = (self.dqk.data_ptr() + 4 * C, 2 * C)
            self.grads = [self.dqk]
        else:
            self.qt, self.kt, self.dqt, self.dkt = rnd(rq, C), rnd(rk, C), new(rq, C), new(rk, C)
            self.q, self.k, self.dq, self.dk = (self.qt.data_ptr(), C), (self.kt.data_ptr(), C), (self.dqt.data_ptr(), C), (self.dkt.data_ptr(), C)
            self.grads = [self.dqt, self.dkt]
        self.v, self.go, self.o, self.dv = rnd(rk, C), rnd(rq, C), new(rq, C), new(rk, C)
        self.slots = torch.zeros(4, 512, dtype=torch.float32, device="cuda")      # o, dq, dk, dv: a fresh slot is zeros
        self.seed = torch.tensor([SEED], dtype=torch.int64, device="cuda") if p > 0 else None
        self.work = None

    def geometry(self):
        return (self.mode, self.dim0, self.P, self.W, self.ws, self.Tq, self.Tk, self.heads, HD, self.mask, self.p,
                self.seed.data_ptr() if self.seed is not None else None, SALT)

    def fwd(self, L, long):
        fn = L.npvp_attn_long_fwd if long else L.npvp_attn_fwd
        return fn(*self.q, *self.k, self.v.data_ptr(), self.C, self.o.data_ptr(), self.C, *self.geometry(), self.slots[0].data_ptr(), None)

    def bwd(self, L, long):
        args = (*self.q, *self.k, self.v.data_ptr(), self.C, self.go.data_ptr(), self.C, *self.dq, *self.dk, self.dv.data_ptr(), self.C,
                *self.geometry(), self.slots[1].data_ptr(), self.slots[2].data_ptr(), self.slots[3].data_ptr())
        if not long:
            return L.npvp_attn_bwd(*args, None)
        if self.work is None:
            nbytes = L.npvp_attn_long_bwd_workspace_bytes(self.mode, self.dim0, self.P, self.W, self.ws, self.Tq, self.Tk, self.heads)
            self.work = torch.full((nbytes // 4,), -7.0, dtype=torch.float32, device="cuda")
        return L.npvp_attn_long_bwd(*args, self.work.data_ptr(), self.work.numel() * 4, None)

    def samples(self, L, S, chunk):
        return L.npvp_attn_samples_fwd(*self.q, *self.k, self.v.data_ptr(), self.C, self.o.data_ptr(), self.C, S, self.dim0, self.P, self.Tq,
                                       self.Tk, self.heads, HD, chunk, self.slots[0].data_ptr(), None)

    def digest(self):
        torch.cuda.synchronize()
        outs = [self.o] + self.grads + [self.dv, self.slots] + ([self.work] if self.work is not None else [])
        return hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in outs)).hexdigest()


def ok(L, rc):
    assert rc == 0, L.npvp_last_error()


def fingerprint(L):
    seed = 27100
    for name, shapes, long in (("short    ", SHORT, False), ("generic  ", GENERIC, False), ("streaming", STREAM, True)):
        for Tq, Tk in shapes:
            for p in DROPS:
                seed += 1
                c = Case(1, 1, 2, 3, 8, 0, Tq, Tk, int(Tq == Tk), p, seed)
                ok(L, c.fwd(L, long)); ok(L, c.bwd(L, long))
                print(f"{name} temporal {Tq:3d} x {Tk:3d} mask {c.mask} drop {p}  {c.digest()}")
    for ws, H, W, long in WINDOWS:
        for p in DROPS:
            seed += 1
            c = Case(0, 2, 2, H * W, W, ws, 0, 0, 0, p, seed)
            ok(L, c.fwd(L, long)); ok(L, c.bwd(L, long))
            print(f"{'streaming' if long else 'short/gen'} windows ws {ws} on {H}x{W}, 2 frames, drop {p}  {c.digest()}")
    for Tq, Tk in SAMPLES:
        for chunk in (0, 2):
            seed += 1
            c = Case(1, 2, 2, 3, 8, 0, Tq, Tk, 0, 0.0, seed, clips_q=3 * 2)
            ok(L, c.samples(L, 3, chunk))
            print(f"samples   S 3 N 2 {Tq:3d} x {Tk:3d} chunk {chunk}  {c.digest()}")


def timing(libs, paths):
    """[(case, [median seconds per library])] at the workload's sizes, printed as a table"""
    N, P, heads = 64, 64, 8
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def measure(name, fns, rounds=7):
        iters = []
        for fn in fns:                            # calls per timed sample: about 20 ms worth
            fn(); torch.cuda.synchronize()
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            iters.append(max(1, min(50, int(20.0 / max(e0.elapsed_time(e1), 1e-3)))))
        t_end = time.time() + 0.5
        while time.time() < t_end:
            for fn in fns:
                fn()
            torch.cuda.synchronize()
        samples = [[] for _ in fns]
        for _ in range(rounds):
            for i, fn in enumerate(fns):
                e0.record()
                for _ in range(iters[i]):
                    fn()
                e1.record(); torch.cuda.synchronize()
                samples[i].append(e0.elapsed_time(e1) / iters[i] * 1e-3)
        med = [statistics.median(s) for s in samples]
        print(f"  {name:46s} " + " ".join(f"{m * 1e6:10.1f}" for m in med), flush=True)
        return name, med

    def pair(tag, c, long):
        def call(L, f):
            def run():
                ok(L, f(L, long))
            return run
        return [measure(f"{tag} fwd", [call(L, c.fwd) for L in libs]), measure(f"{tag} bwd", [call(L, c.bwd) for L in libs])]

    print(f"# {torch.cuda.get_device_name(0)}, ROCm {torch.version.hip}; N = {N} clips, P = {P} pixels, {heads} heads; us per call, "
          "medians of 7 interleaved rounds after 0.5 s of warm-up")
    for i, p in enumerate(paths):
        print(f"# library {i}: {p}  sha256 {hashlib.sha256(open(p, 'rb').read()).hexdigest()[:16]}")
    print(f"  {'case':46s} " + " ".join(f"{'lib ' + str(i):>10s}" for i in range(len(libs))))
    rows = []
    for Tq, Tk in [(28, 28), (28, 2), (18, 18), (10, 10), (2, 2)]:
        for p in (0.1, 0.0):
            rows += pair(f"temporal {Tq} x {Tk} drop {p}", Case(1, N, heads, P, 8, 0, Tq, Tk, int(Tq == Tk), p, 1, rng="cuda"), False)
    rows += pair("spatial 4x4 windows, 1920 frames, drop 0.1", Case(0, 30 * N, heads, 64, 8, 4, 0, 0, 0, 0.1, 2, rng="cuda"), False)
    for T in (40, 128):
        for long in (False, True):
            torch.cuda.empty_cache()
            rows += pair(f"{'streaming' if long else 'generic'} {T} x {T} drop 0.1", Case(1, N, heads, P, 8, 0, T, T, 1, 0.1, 3, rng="cuda"), long)
    torch.cuda.empty_cache()
    c = Case(1, 8, heads, P, 8, 0, 28, 2, 0, 0.0, 4, clips_q=32 * 8, rng="cuda")
    rows.append(measure("samples S 32 N 8 28 x 2", [(lambda L=L: ok(L, c.samples(L, 32, 0))) for L in libs]))
    if len(libs) >= 3:
        spread = max(abs(m[2] - m[0]) / m[0] for _, m in rows)
        print(f"# spread of the method (largest relative difference between library 0 and its copy, library 2): {100 * spread:.2f} %")
        for name, m in rows:
            d = (m[1] - m[0]) / m[0]
            print(f"  {name:46s} library 1 vs 0 {100 * d:+6.2f} %   copy vs 0 {100 * (m[2] - m[0]) / m[0]:+6.2f} %   "
                  f"{'within the spread' if d <= spread else 'SLOWER THAN THE SPREAD'}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", action="append", help="library to load (repeat for --time); default: the tree's")
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    paths = a.lib or [os.path.join(ROOT, "npvp_amd", "libnpvp_hip.so")]
    libs = [load(p) for p in paths]
    if a.time:
        timing(libs, paths)
    else:
        assert len(libs) == 1, "one --lib per fingerprint: compare the printed lines of two runs"
        fingerprint(libs[0])


if __name__ == "__main__":
    main()
