"""GEMM micro-benchmark on the predictor's shapes (R token rows x the linears' (N_out, K_in)): algorithmic TFLOP/s of the
forward / dgrad / weight-gradient GEMMs and max error against an fp64 product.
Usage: python tools/gemm_bench.py [--rows R] [--iters N] [--mode bf16x6|f32] [--check]
       python tools/gemm_bench.py --f16x1 [--rows R] [--iters N] [--rounds N]
--f16x1: forward-only.  The forward GEMM of every shape in the inference arithmetic f16x1 (ops.eval_arithmetic: one fp16 term per
operand) against f16x3 on the SAME operands and planes, in the same process: after a warm-up of both, `--rounds` rounds ALTERNATE
between the two (each round = `--iters` launches between two events), so that clock and cache state drift hits both alike.  Per
shape: the tile variant the launch takes, the median and the spread (min .. max) of the rounds of each arithmetic, the ratio of the
medians, and whether f16x1 beats f16x3 by more than the spread of the rounds (its slowest round is faster than f16x3's fastest)."""
import sys, os, argparse
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from npvp_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="*", default=[114688, 20480, 8192])      # c2 decoder, c1, c2 encoder / c4 shard
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--mode", default="bf16x6")
ap.add_argument("--check", action="store_true")
ap.add_argument("--grad-scale", type=float, default=1.0, help="magnitude of dy (gradient-sized operands: 1e-8)")
ap.add_argument("--heavy", action="store_true", help="log-normal magnitudes on dy (heavy tail) and per-row scales over 1e-3..1e3")
ap.add_argument("--f16x1", action="store_true", help="forward only: f16x1 against f16x3, alternated rounds")
ap.add_argument("--rounds", type=int, default=7)
args = ap.parse_args()
if args.f16x1:
    args.mode = "f16x3"
dev = "cuda:0"
shapes = [(512, 512), (1024, 512), (2048, 512), (512, 2048), (512, 1024)]      # (N_out, K_in) of the linears
torch.manual_seed(0)
ops.set_gemm_precision(args.mode)


def timeit(fn):
    fn(); fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters * 1e-3


def err(a, ref):
    return float((a.double() - ref).norm() / ref.norm())


def one_term_rounds():
    import ctypes
    import statistics
    from npvp_amd._lib import lib
    route = (ctypes.c_int * 4)()
    verdicts = {}
    for R in args.rows:
        for N, K in shapes:
            x = torch.randn(R, K, device=dev); w = torch.nn.Parameter(torch.randn(N, K, device=dev) / K ** 0.5)
            b = torch.randn(N, device=dev)
            lib().npvp_gemm_route(1, 1, R, N, K, 7, int(R >= 256), 0, ctypes.addressof(route))
            fl = 2.0 * R * N * K
            arith = ("f16x3", "f16x1")
            t = {a: [] for a in arith}
            with torch.no_grad():
                def run(a):
                    with ops.eval_arithmetic(a) as blk:
                        ops.linear_fwd(x, w, b)
                    return blk.switched

                assert run("f16x1") == (1 if route[0] in (5, 7) else 0) and run("f16x3") == 0
                for a in arith:                      # warm-up of both before the first timed round
                    for _ in range(3):
                        run(a)
                torch.cuda.synchronize()
                for _ in range(args.rounds):
                    for a in arith:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        with ops.eval_arithmetic(a):
                            e0.record()
                            for _ in range(args.iters):
                                ops.linear_fwd(x, w, b)
                            e1.record()
                        torch.cuda.synchronize()
                        t[a].append(e0.elapsed_time(e1) / args.iters * 1e-3)
            m3, m1 = statistics.median(t["f16x3"]), statistics.median(t["f16x1"])
            wins = max(t["f16x1"]) < min(t["f16x3"])
            verdicts.setdefault((route[0], route[1]), []).append(wins)
            print(f"R={R:6d} N={N:5d} K={K:5d} id {route[0]} variant {route[1]}  f16x3 {fl/m3/1e12:6.1f} TF {m3*1e6:8.1f} us "
                  f"({min(t['f16x3'])*1e6:.1f} .. {max(t['f16x3'])*1e6:.1f})  f16x1 {fl/m1/1e12:6.1f} TF {m1*1e6:8.1f} us "
                  f"({min(t['f16x1'])*1e6:.1f} .. {max(t['f16x1'])*1e6:.1f})  x{m3/m1:.2f}  "
                  f"{'beats f16x3 beyond the spread' if wins else 'NOT beyond the spread'}", flush=True)
    for (kid, v), ws in sorted(verdicts.items()):
        print(f"id {kid} variant {v}: f16x1 beyond the spread on {sum(ws)} of {len(ws)} shapes", flush=True)


if args.f16x1:
    one_term_rounds()
    sys.exit(0)

for R in args.rows:
    tot_t, tot_f = [0.0, 0.0, 0.0], 0.0
    for N, K in shapes:
        x = torch.randn(R, K, device=dev); w = torch.nn.Parameter(torch.randn(N, K, device=dev) / K ** 0.5)
        dy = torch.randn(R, N, device=dev) * args.grad_scale; b = torch.randn(N, device=dev)
        if args.heavy:
            dy = dy * torch.exp(2 * torch.randn(R, N, device=dev)) * torch.exp(torch.empty(R, 1, device=dev).uniform_(-7, 7))
        fl = 2.0 * R * N * K
        t1 = timeit(lambda: ops.linear_fwd(x, w, b))
        t2 = timeit(lambda: ops.linear_dgrad(dy, w))
        t3 = timeit(lambda: ops.linear_wgrad(dy, x))
        for i, t in enumerate((t1, t2, t3)):
            tot_t[i] += t
        tot_f += fl
        extra = ""
        if args.check:
            n = min(R, 4096)
            e1 = err(ops.linear_fwd(x, w, b)[:n], x[:n].double() @ w.double().T + b.double())
            e2 = err(ops.linear_dgrad(dy, w)[:n], dy[:n].double() @ w.double())
            dgr, ref = ops.linear_dgrad(dy, w)[:n].double(), dy[:n].double() @ w.double()
            e2r = float(((dgr - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)).max())
            m = min(R, 16384)
            e3 = err(ops.linear_wgrad(dy[:m].contiguous(), x[:m].contiguous()), dy[:m].double().T @ x[:m].double())
            t32 = err((x[:n] @ w.T + b), x[:n].double() @ w.double().T + b.double())
            extra = f"  err fwd {e1:.1e} (torch fp32 {t32:.1e}) dgrad {e2:.1e} (worst row {e2r:.1e}) wgrad[{m}] {e3:.1e}"
        print(f"R={R:6d} N={N:5d} K={K:5d}  fwd {fl/t1/1e12:6.1f} TF ({t1*1e6:7.1f} us)  dgrad {fl/t2/1e12:6.1f} TF ({t2*1e6:7.1f} us)  "
              f"wgrad {fl/t3/1e12:6.1f} TF ({t3*1e6:7.1f} us){extra}", flush=True)
    print(f"R={R:6d} all shapes: fwd {tot_f/tot_t[0]/1e12:.1f}  dgrad {tot_f/tot_t[1]/1e12:.1f}  wgrad {tot_f/tot_t[2]/1e12:.1f} TF", flush=True)
