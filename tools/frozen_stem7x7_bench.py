"""The 7 x 7 stem of the fused frozen encoder, to_device_layout(..., stem7x7="stock") against stem7x7="hip", in ONE process: what the
stock stem's time is made of, the stem alone, and the whole encoder.
  parts    the stock stem's forward on the planar frames the data path hands over, piece by piece: the padded copy (ReflectionPad2d(3)),
           MIOpen's convolution with C_in = 1 or 3 (channels-last weights, as to_device_layout leaves them), npvp_bias_act; and the
           npvp_amax pass over the stem's output that a routed block1 behind a STOCK stem then needs.
  stem     A = the stock FoldedConvAct (pad, MIOpen, npvp_bias_act), B = ops.stem7x7_packed on the same planar frames (one npvp_amax pass
           over the untagged input, one launch: padding as index math, bias and ReLU in the epilogue, channels-last out with its slot).
           "+amax" = the same with what a routed block1 needs behind it: A pays the npvp_amax pass over its output, B hands its slot on.
  encoder  frames (N, T, ch, S, S) -> features under no_grad, attn2d, conv3x3 and down3x3 "hip" on both sides.
Sizes: c1 = 640 frames of 64 x 64 x 1 (ngf 64, 3 downsamplings), c2 = 1920 frames of 64 x 64 x 3 (ngf 64; the stem only), c4 = 160
frames of 128 x 128 x 3 (ngf 32, 4).  Method: both routes on the same weights, warmed up at the timed shape; then the routes alternate
A, B, A, B, every timing `iters` calls between two device events.  A shape counts as FASTER only where both B timings beat both A
timings.  No time is a pass condition.  The result is what `_stem7x7_takes_hip` of npvp_amd/models/ResNetAutoEncoder.py cites
(profiles/frozen_stem7x7_bench.txt).
Usage: python tools/frozen_stem7x7_bench.py [--iters 20] [--sizes c1,c2,c4] [--out FILE]"""
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
# AE section, image channels, (N, T), frame side, whether the whole encoder is timed
SIZES = {
    "c1": (dict(ngf=64, n_downsampling=3, num_res_blocks=2, out_layer="Tanh", learn_3d=False), 1, (32, 20), 64, True),
    "c2": (dict(ngf=64, n_downsampling=3, num_res_blocks=2, out_layer="Tanh", learn_3d=False), 3, (64, 30), 64, False),
    "c4": (dict(ngf=32, n_downsampling=4, num_res_blocks=3, out_layer="Tanh", learn_3d=False), 3, (8, 20), 128, True),
}
OTHERS = dict(attn2d="hip", conv3x3="hip", down3x3="hip")


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


def encoder(AE, ch, stem7x7):
    enc, dec = npvp_amd.build_frozen_autoencoder(AE, ch)
    O.key_hashed_fill(enc, 121)
    return npvp_amd.to_device_layout(enc, dec, DEV, stem7x7=stem7x7, **OTHERS)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", default="c1,c2,c4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frozen_stem7x7_bench needs an MI355X: a CPU run gives no time")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"frozen_stem7x7_bench on {torch.cuda.get_device_name(0)}: A = stem7x7=\"stock\" (padded copy, MIOpen, npvp_bias_act), "
        f"B = stem7x7=\"hip\" (npvp_amax over the frames, npvp_stem7x7_f16); order A B A B; FASTER = both B below both A")
    with torch.no_grad():
        for name in args.sizes.split(","):
            AE, ch, (N, T), side, whole = SIZES[name]
            frames, C = N * T, AE["ngf"]
            encs = {r: encoder(AE, ch, r) for r in ("stock", "hip")}
            ms, mh = encs["stock"].block0[0], encs["hip"].block0[0]
            assert mh.stem7x7 and not ms.stem7x7
            x5 = torch.rand((N, T, ch, side, side), generator=torch.Generator().manual_seed(5)).to(DEV)
            x = x5.flatten(0, 1)
            gb = frames * side * side * C * 4 / 1e9
            # ---- what the stock forward is made of
            xp = ms.pad(x)
            yc = F.conv2d(xp, ms.weight)
            ys = ops.bias_act(yc, ms.bias, ms.act)
            parts = [("padded copy", lambda: ms.pad(x)), ("MIOpen convolution", lambda: F.conv2d(xp, ms.weight)),
                     ("npvp_bias_act", lambda: ops.bias_act(yc, ms.bias, ms.act)),
                     ("npvp_amax over the output", lambda: ops.amax_of(ys.detach().permute(0, 2, 3, 1).reshape(-1, C)))]
            for _, fn in parts:
                fn(); fn()
            torch.cuda.synchronize()
            say(f"parts {name}: {frames} frames of {side}x{side}, C_in {ch} -> {C} (output {gb:.2f} GB), stock forward: " +
                ", ".join(f"{what} {timed(fn, args.iters):.3f} ms" for what, fn in parts))
            del xp, yc, ys, parts
            # ---- the stem alone
            stock = lambda: ms(x)
            hip = lambda: mh(x)
            stock_amax = lambda: ops.amax_of(ms(x).permute(0, 2, 3, 1).reshape(-1, C))
            for _ in range(2):
                ya, yb = stock(), hip()
                stock_amax()
            torch.cuda.synchronize()
            assert yb.permute(0, 2, 3, 1).is_contiguous() and getattr(yb, "_npvp_amax", None) is not None
            gmac = frames * side * side * 49 * ch * C / 1e9
            head = f"stem {name}: C_in {ch} -> {C}, {frames} frames of {side}x{side} ({gmac:.1f} GMAC, output {gb:.2f} GB)"
            a, b, verdict = abab(stock, hip, args.iters)
            say(f"{head} fwd      : A {a[0]:7.3f} {a[1]:7.3f} ms, B {b[0]:7.3f} {b[1]:7.3f} ms ({gb / min(b):5.2f} TB/s of output at the best B): "
                f"{verdict}; hip vs stock rel-L2 {rel(yb, ya):.2e}")
            a, b, verdict = abab(stock_amax, hip, args.iters)
            say(f"{head} fwd +amax: A {a[0]:7.3f} {a[1]:7.3f} ms, B {b[0]:7.3f} {b[1]:7.3f} ms: {verdict}")
            del ya, yb
            torch.cuda.empty_cache()
            # ---- the whole encoder
            if whole:
                ea, eb = encs["stock"], encs["hip"]
                for _ in range(2):                                   # warm-up at the timed shape (solver search, code objects, workspaces)
                    oa, ob = ea(x5), eb(x5)
                torch.cuda.synchronize()
                a, b, verdict = abab(lambda: ea(x5), lambda: eb(x5), args.iters)
                say(f"encoder {name}: AE {AE['ngf']}/{AE['n_downsampling']}, {frames} frames of {side}x{side}x{ch}, attn2d, conv3x3, down3x3 hip "
                    f"on both sides, fwd: A {a[0]:7.2f} {a[1]:7.2f} ms, B {b[0]:7.2f} {b[1]:7.2f} ms: {verdict}; features hip vs stock rel-L2 "
                    f"{rel(ob, oa):.2e}")
                del oa, ob
            del encs, x, x5
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
