"""Encoder forward of the fused frozen pair, to_device_layout(..., conv3x3="hip", down3x3="stock") against down3x3="hip", in ONE process,
and each distinct stride-2 3 x 3 convolution of the two encoders alone: ops.conv3x3s2_packed (one f16x3 implicit-GEMM launch, the
STRIDE = 2 form of csrc/conv3x3.hip) against F.conv2d(stride=2) (MIOpen, fp32) + ops.bias_act, the stock route's two passes.  B's input
carries no amax slot, as in the encoder (the stem's and the attention's epilogue pass attach none): every B call includes its npvp_amax pass.
Sizes: c1 = 640 frames of 64 x 64 x 1 (ngf 64, 3 downsamplings, 2 res blocks), c4 = 160 frames of 128 x 128 x 3 (ngf 32, 4 downsamplings,
3 res blocks).  Both encoders run conv3x3="hip": that is the configuration a user of these routes runs.  Method: both routes on the same
weights, warmed up at the timed shape; then the routes alternate A, B, A, B (A = stock, B = hip), every timing `iters` forwards between
two device events.  A shape counts as FASTER only where both B timings beat both A timings.  The outputs of the two routes are compared
on the timed inputs (rel-L2).  No time is a pass condition.  The result is what the eligibility rule `_down3x3_takes_hip` of
npvp_amd/models/ResNetAutoEncoder.py cites (profiles/frozen_down3x3_bench.txt).
Usage: python tools/frozen_down3x3_bench.py [--iters 20] [--conv-iters 200] [--out FILE]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import npvp_amd
from npvp_amd import ops
from oracle import ops as O

DEV = "cuda:0"
SIZES = {
    "c1": (dict(ngf=64, n_downsampling=3, num_res_blocks=2, out_layer="Tanh", learn_3d=False), 1, (32, 20, 1, 64, 64)),
    "c4": (dict(ngf=32, n_downsampling=4, num_res_blocks=3, out_layer="Tanh", learn_3d=False), 3, (8, 20, 3, 128, 128)),
}
# (size, name, C_in, C_out, input grid side, frames): block1 and every block{i}_conv of the two encoders
CONVS = [("c1", "block1", 64, 128, 64, 640), ("c1", "block2_conv", 128, 256, 32, 640), ("c1", "block3_conv", 256, 512, 16, 640),
         ("c4", "block1", 32, 64, 128, 160), ("c4", "block2_conv", 64, 128, 64, 160), ("c4", "block3_conv", 128, 256, 32, 160),
         ("c4", "block4_conv", 256, 512, 16, 160)]
ROUTES = ("stock", "hip")


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def abab(fa, fb, iters):
    """([A1, A2], [B1, B2], verdict) in ms per call, the routes alternating"""
    a, b = [], []
    for _ in range(2):
        a.append(timed(fa, iters))
        b.append(timed(fb, iters))
    verdict = "FASTER" if max(b) < min(a) else ("slower" if min(b) > max(a) else "within the spread")
    return a, b, verdict


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--conv-iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frozen_down3x3_bench needs an MI355X: a CPU run gives no time")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"frozen_down3x3_bench on {torch.cuda.get_device_name(0)}: A = down3x3=\"stock\" (MIOpen + npvp_bias_act), B = down3x3=\"hip\" "
        f"(npvp_conv3x3s2_f16), both with conv3x3=\"hip\"; order A B A B; FASTER = both B below both A")
    with torch.no_grad():
        for size, name, Ci, Co, S, frames in CONVS:
            x = O.seeded_randn((frames, Ci, S, S), 11).to(DEV).contiguous(memory_format=torch.channels_last)
            w = (O.seeded_randn((Co, Ci, 3, 3), 12) * (9 * Ci) ** -0.5).to(DEV).contiguous(memory_format=torch.channels_last)
            b = O.seeded_randn((Co,), 13).to(DEV)
            planes, w_amax = ops.conv3x3s2_planes(w)
            gmac = frames * (S // 2) * (S // 2) * 9 * Ci * Co / 1e9
            stock = lambda: ops.bias_act(F.conv2d(x, w, None, 2, 1), b, 1)
            hip = lambda: ops.conv3x3s2_packed(x, planes, w_amax, b, 1)
            for _ in range(3):
                ys, yh = stock(), hip()
            torch.cuda.synchronize()
            a, bb, verdict = abab(stock, hip, args.conv_iters)
            say(f"conv {size} {name:11s} {Ci:3d} -> {Co:3d} grid {S:3d}x{S:<3d} frames {frames} ({gmac:5.1f} GMAC): A {a[0]:7.3f} {a[1]:7.3f} ms, "
                f"B {bb[0]:7.3f} {bb[1]:7.3f} ms ({2 * gmac / min(bb):6.1f} TFLOP/s fp32-equivalent at the best B): {verdict}; "
                f"hip vs stock rel-L2 {rel(yh, ys):.2e}")
            del x, w, planes
        for name, (AE, ch, shape) in SIZES.items():
            x = torch.rand(shape, generator=torch.Generator().manual_seed(5)).to(DEV)
            encs = {}
            for r in ROUTES:
                enc, dec = npvp_amd.build_frozen_autoencoder(AE, ch)
                O.key_hashed_fill(enc, 121)
                encs[r] = npvp_amd.to_device_layout(enc, dec, DEV, conv3x3="hip", down3x3=r)[0]
            out = {}
            for r in ROUTES:
                for _ in range(2):                                   # warm-up at the timed shape (solver search, code objects, workspaces)
                    out[r] = encs[r](x)
            torch.cuda.synchronize()
            a, b, verdict = abab(lambda: encs["stock"](x), lambda: encs["hip"](x), args.iters)
            say(f"encoder {name}: AE {AE['ngf']}/{AE['n_downsampling']}/{AE['num_res_blocks']}, {shape[0] * shape[1]} frames of "
                f"{shape[3]}x{shape[4]}x{shape[2]}, conv3x3=\"hip\": A {a[0]:7.2f} {a[1]:7.2f} ms, B {b[0]:7.2f} {b[1]:7.2f} ms: {verdict}; "
                f"hip vs stock features rel-L2 {rel(out['hip'], out['stock']):.2e}")
            del encs, out, x
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
