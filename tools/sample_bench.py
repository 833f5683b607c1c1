"""Predictor.sample (S futures per clip, the context encoded once) against S eval forwards of the same commit.
Shapes: KTH (To 10, Tp 20), BAIR (To 2, Tp 28) at N = 8 clips, and BAIR at N = 1; 8 x 8 x 512 features, 4 encoder + 8 decoder
blocks; S in {1, 8, 32}.  Both sides run under no_grad in eval mode on the same module and input; each timed sample is one whole
call (sample) or one whole loop of S forwards, between device events with a synchronise after; the two are alternated in every
round after a warm-up of every shape, and the table holds the median and the spread (min .. max) of the rounds.
Usage: python tools/sample_bench.py [--out profiles/sample_bench.txt] [--rounds 5]
       python tools/sample_bench.py --arithmetic f16x1 [--out profiles/sample_bench_f16x1.txt] [--rounds 5]
--arithmetic f16x1: sample() in the training arithmetic (f16x3) against sample(arithmetic="f16x1") - one fp16 term per operand in the
forward GEMMs - on the same module, input and seed, alternated in the same rounds; then, per shape at S = 8 and one seed, how far the
two results are apart (rel-L2) and what that does to best-of-S PSNR / SSIM.  The clips of that last part are synthetic: a frame is a
feature map pixel-shuffled to 2 x 128 x 128 and squashed to [0, 1], the target the same picture of a random feature map, so the
metrics' VALUES mean nothing - only their shift between the two arithmetics does.  It carries no bar."""
import hashlib
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import npvp_amd
from npvp_amd import _lib

DEV = "cuda:0"
SHAPES = [("KTH  To 10 Tp 20 N 8", 10, 20, 8), ("BAIR To  2 Tp 28 N 8", 2, 28, 8), ("BAIR To  2 Tp 28 N 1", 2, 28, 1)]
SAMPLES = (1, 8, 32)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def build(To, Tp):
    h = torch.linspace(0, 7, 8)
    torch.manual_seed(0)
    m = npvp_amd.Predictor(8, 8, To + Tp, h, h, torch.linspace(0, To - 1, To), torch.linspace(To, To + Tp - 1, Tp), 512, 'Add', 'layer',
                           256, 1, True, 8, evt_former=True, learn_evt_token=False, evt_former_num_layers=4)
    return m.to(DEV).eval()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def frames_of(feats):
    """(..., 512, 8, 8) features -> (..., 2, 128, 128) synthetic frames in [0, 1]"""
    return torch.sigmoid(torch.nn.functional.pixel_shuffle(feats, 16))


def main_arithmetic(name):
    """sample() in f16x3 against sample(arithmetic=name), alternated; then the shift of the result and of best-of-S metrics"""
    from npvp_amd import metrics as M
    out_path, rounds = arg("--out", os.path.join("profiles", "sample_bench_f16x1.txt")), int(arg("--rounds", 5))
    lines = [f"# libnpvp_hip.so sha256 {hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest()}",
             f"# ROCm (torch.version.hip) {torch.version.hip}, torch {torch.__version__}, {torch.cuda.get_device_name(0)}",
             f"# 4 encoder + 8 decoder blocks, 8 x 8 x 512 features, eval, no_grad; ms per call: median (min .. max) of {rounds} alternated rounds",
             f"# {'shape':22s} {'S':>3s} {'sample() f16x3':>28s} {'sample() ' + name:>28s} {'f16x3 / ' + name:>13s} {'switched':>8s}"]
    for line in lines:
        print(line, flush=True)
    shifts = []
    for sname, To, Tp, N in SHAPES:
        m = build(To, Tp)
        past = torch.randn(N, To, 512, 8, 8, device=DEV).relu_()
        for S in SAMPLES:
            def three():
                return m.sample(past, S, seed=1)

            def one():
                return m.sample(past, S, seed=1, arithmetic=name)

            three(); one(); three()
            with npvp_amd.eval_arithmetic(name) as blk:          # (the block around the call is the same thing: counts the launches)
                m.sample(past, S, seed=1)
            torch.cuda.synchronize()
            t3, t1 = [], []
            for _ in range(rounds):
                t3.append(timed(three))
                t1.append(timed(one))
            f = lambda v: f"{statistics.median(v):9.2f} ({min(v):8.2f} .. {max(v):8.2f})"
            line = f"  {sname:22s} {S:3d} {f(t3)} {f(t1)} {statistics.median(t3) / statistics.median(t1):13.3f} {blk.switched:8d}"
            lines.append(line)
            print(line, flush=True)
        a, b = m.sample(past, 8, seed=7), m.sample(past, 8, seed=7, arithmetic=name)
        target = frames_of(torch.randn(N, Tp, 512, 8, 8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)).relu_())
        row = f"  {sname:22s} S 8 seed 7: rel-L2 between the arithmetics {float((b - a).norm() / a.norm()):.3e}"
        for fn, label in ((M.PSNR, "PSNR"), (M.SSIM(), "SSIM")):
            ia, best_a, _ = M.best_of_samples(frames_of(a), target, fn)
            ib, best_b, _ = M.best_of_samples(frames_of(b), target, fn)
            row += (f"; best-of-8 {label} f16x3 {float(best_a.mean()):.5f} {name} {float(best_b.mean()):.5f} "
                    f"(shift {float(best_b.mean() - best_a.mean()):+.2e}, same best sample on {int((ia == ib).sum())} of {N} clips)")
        shifts.append(row)
        del m, past
        torch.cuda.empty_cache()
    lines.append("# synthetic clips (pixel-shuffled feature maps): only the shift between the arithmetics means anything")
    lines += shifts
    for row in shifts:
        print(row, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/sample_bench.py measures on an MI355X: no device is visible (nothing is measured on the CPU)")
    if "--arithmetic" in sys.argv:
        return main_arithmetic(arg("--arithmetic", "f16x1"))
    out_path, rounds = arg("--out", os.path.join("profiles", "sample_bench.txt")), int(arg("--rounds", 5))
    lines = [f"# libnpvp_hip.so sha256 {hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest()}",
             f"# ROCm (torch.version.hip) {torch.version.hip}, torch {torch.__version__}, {torch.cuda.get_device_name(0)}",
             f"# 4 encoder + 8 decoder blocks, 8 x 8 x 512 features, eval, no_grad; ms per call: median (min .. max) of {rounds} alternated rounds",
             f"# {'shape':22s} {'S':>3s} {'sample()':>28s} {'S eval forwards':>28s} {'loop / sample':>13s}"]
    for line in lines:
        print(line, flush=True)
    for name, To, Tp, N in SHAPES:
        m = build(To, Tp)
        past = torch.randn(N, To, 512, 8, 8, device=DEV).relu_()
        for S in SAMPLES:
            def sample():
                return m.sample(past, S, seed=1)

            def loop():
                with torch.no_grad():
                    for _ in range(S):
                        m(past)

            sample(); loop(); sample(); loop()          # warm-up of this shape: code objects, weight planes, allocator
            torch.cuda.synchronize()
            ts, tl = [], []
            for _ in range(rounds):
                ts.append(timed(sample))
                tl.append(timed(loop))
            f = lambda v: f"{statistics.median(v):9.2f} ({min(v):8.2f} .. {max(v):8.2f})"
            line = f"  {name:22s} {S:3d} {f(ts)} {f(tl)} {statistics.median(tl) / statistics.median(ts):13.3f}"
            lines.append(line)
            print(line, flush=True)
        del m, past
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
