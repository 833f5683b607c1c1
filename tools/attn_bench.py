"""Attention cores at the c2 size (BAIR B=64: 64 clips x 64 pixels x 8 heads), forward and backward, against their
ALGORITHMIC bytes (q, k, v [, dO] read once, o [dq, dk, dv] written once, fp32) - SURVEY 8(d).
Usage: python tools/attn_bench.py [--clips 64]
       python tools/attn_bench.py --long [--clips 64]      the streaming kernels (npvp_attn_long_*): against the generic route on
                                                           the same inputs at 33 .. 128 rows, and alone above 128"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from npvp_amd import ops
from npvp_amd.ops import AttnCfg

dev = "cuda:0"
N = int(sys.argv[sys.argv.index("--clips") + 1]) if "--clips" in sys.argv else 64
P, C, PEAK = 64, 512, 8000.0
torch.manual_seed(0)


def timeit(fn, iters=20):
    fn(); fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def report(name, nbytes, t):
    print(f"{name:52s} {t*1e6:8.1f} us  {nbytes/1e6:8.1f} MB algorithmic  {nbytes/t/1e9:7.0f} GB/s  {100*nbytes/t/1e9/PEAK:5.1f} % of 8 TB/s", flush=True)


def long_mode():
    """Interleaved rounds after a long warm-up, medians (DESIGN: a kernel timed first runs on a GPU that has just idled).  The route
    is chosen by ops.ATTN_LONG_MIN at call time, forward and backward alike: 129 = the shipped routing (generic kernels up to 128),
    1 = everything on the streaming kernels."""
    import hashlib, statistics
    from npvp_amd import _lib
    print(f"# libnpvp_hip.so sha256 {hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest()}")
    print(f"# ROCm (torch.version.hip) {torch.version.hip}, torch {torch.__version__}, {torch.cuda.get_device_name(0)}")
    print(f"# N = {N} clips, P = {P} pixels, 8 heads, C = {C}, attention dropout 0.1; medians of 7 interleaved rounds after 0.5 s of warm-up")

    def routed(lo, fn):
        def f():
            old = ops.ATTN_LONG_MIN
            ops.ATTN_LONG_MIN = lo
            try:
                return fn()
            finally:
                ops.ATTN_LONG_MIN = old
        return f

    def measure(variants, rounds=7):
        """variants: [(name, algorithmic bytes, fn)] -> prints one line each"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        iters = {}
        for name, _, fn in variants:              # calls per timed sample: about 20 ms worth
            fn(); torch.cuda.synchronize()
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            iters[name] = max(1, min(50, int(20.0 / max(e0.elapsed_time(e1), 1e-3))))
        import time
        t_end = time.time() + 0.5
        while time.time() < t_end:
            for _, _, fn in variants:
                fn()
            torch.cuda.synchronize()
        samples = {name: [] for name, _, _ in variants}
        for _ in range(rounds):
            for name, _, fn in variants:
                e0.record()
                for _ in range(iters[name]):
                    fn()
                e1.record(); torch.cuda.synchronize()
                samples[name].append(e0.elapsed_time(e1) / iters[name] * 1e-3)
        for name, nbytes, _ in variants:
            report(name, nbytes, statistics.median(samples[name]))

    def temporal(Tq, Tk, both):
        Rq, Rk = N * Tq * P, N * Tk * P
        cfg = AttnCfg(1, N, P, 8, 0, Tq, Tk, 8, 0, 0.1)
        if Tq == Tk:
            qk = torch.randn(Rq, 2 * C, device=dev, requires_grad=True); v = torch.randn(Rk, C, device=dev, requires_grad=True)
            ins, fwd = [qk, v], lambda: ops.attn_packed(qk.detach(), v.detach(), cfg)
            y = ops.attn_packed(qk, v, cfg)          # (the graph is route-free: the kernels are chosen when a node runs)
        else:
            q = torch.randn(Rq, C, device=dev, requires_grad=True); k = torch.randn(Rk, C, device=dev, requires_grad=True)
            v = torch.randn(Rk, C, device=dev, requires_grad=True)
            ins, fwd = [q, k, v], lambda: ops.attn(q.detach(), k.detach(), v.detach(), cfg)
            y = ops.attn(q, k, v, cfg)
        go = torch.randn_like(y)
        bwd = lambda: torch.autograd.grad(y, ins, go, retain_graph=True)
        bq, bk = Rq * C * 4, Rk * C * 4
        tag = f"Tq={Tq} Tk={Tk} ({Rq} query rows)"
        vs = []
        if both:
            vs += [(f"generic   fwd  {tag}", 2 * bq + 2 * bk, routed(129, fwd)), (f"generic   bwd  {tag}", 3 * bq + 4 * bk, routed(129, bwd))]
        vs += [(f"streaming fwd  {tag}", 2 * bq + 2 * bk, routed(1, fwd)), (f"streaming bwd  {tag}", 3 * bq + 4 * bk, routed(1, bwd))]
        measure(vs)

    print("# against the generic route, same inputs")
    temporal(40, 40, True)
    temporal(128, 128, True)
    F_ = N * 30
    R = F_ * P
    qk = torch.randn(R, 2 * C, device=dev, requires_grad=True); v = torch.randn(R, C, device=dev, requires_grad=True)
    cfg = AttnCfg(0, F_, 64, 8, 8, 0, 0, 8, 0, 0.1)
    y = ops.attn_packed(qk, v, cfg); go = torch.randn_like(y)
    fwd = lambda: ops.attn_packed(qk.detach(), v.detach(), cfg)
    bwd = lambda: torch.autograd.grad(y, [qk, v], go, retain_graph=True)
    tag = f"spatial 8x8 window ({F_} frames)"
    measure([(f"generic   fwd  {tag}", 4 * R * C * 4, routed(129, fwd)), (f"generic   bwd  {tag}", 7 * R * C * 4, routed(129, bwd)),
             (f"streaming fwd  {tag}", 4 * R * C * 4, routed(1, fwd)), (f"streaming bwd  {tag}", 7 * R * C * 4, routed(1, bwd))])
    del qk, v, y, go
    print("# streaming kernels alone (no other kernel takes these lengths)")
    for Tq, Tk in [(160, 160), (256, 256), (256, 4)]:
        torch.cuda.empty_cache()
        temporal(Tq, Tk, False)


if "--long" in sys.argv:
    long_mode()
    sys.exit(0)

for Tq, Tk, mask, pdrop in [(28, 28, 0, 0.1), (28, 2, 0, 0.1), (18, 18, 0, 0.1), (10, 10, 1, 0.1), (2, 2, 1, 0.1)]:
    Rq, Rk = N * Tq * P, N * Tk * P
    cfg = AttnCfg(1, N, P, 8, 0, Tq, Tk, 8, mask, pdrop)
    if Tq == Tk:       # self attention: q | k packed in one [R, 2C] projection output, as in the model
        qk = torch.randn(Rq, 2 * C, device=dev, requires_grad=True); v = torch.randn(Rk, C, device=dev, requires_grad=True)
        ins, fwd = [qk, v], lambda: ops.attn_packed(qk.detach(), v.detach(), cfg)
        y = ops.attn_packed(qk, v, cfg)
    else:
        q = torch.randn(Rq, C, device=dev, requires_grad=True); k = torch.randn(Rk, C, device=dev, requires_grad=True)
        v = torch.randn(Rk, C, device=dev, requires_grad=True)
        ins, fwd = [q, k, v], lambda: ops.attn(q.detach(), k.detach(), v.detach(), cfg)
        y = ops.attn(q, k, v, cfg)
    go = torch.randn_like(y)
    bq, bk = Rq * C * 4, Rk * C * 4
    report(f"temporal fwd  Tq={Tq} Tk={Tk} mask={mask}", 2 * bq + 2 * bk, timeit(fwd))
    report(f"temporal bwd  Tq={Tq} Tk={Tk} mask={mask}", 3 * bq + 4 * bk, timeit(lambda: torch.autograd.grad(y, ins, go, retain_graph=True)))

F_ = N * 30
R = F_ * P
qk = torch.randn(R, 2 * C, device=dev, requires_grad=True); v = torch.randn(R, C, device=dev, requires_grad=True)
cfg = AttnCfg(0, F_, 64, 8, 4, 0, 0, 8, 0, 0.1)
y = ops.attn_packed(qk, v, cfg); go = torch.randn_like(y)
report("spatial 4x4 windows fwd (1920 frames)", 4 * R * C * 4, timeit(lambda: ops.attn_packed(qk.detach(), v.detach(), cfg)))
report("spatial 4x4 windows bwd", 7 * R * C * 4, timeit(lambda: torch.autograd.grad(y, [qk, v], go, retain_graph=True)))
