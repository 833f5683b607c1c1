"""The 7 x 7 tail of the fused frozen decoder, to_device_layout(..., tail7x7="stock") against tail7x7="hip", in ONE process: what the
stock tail's time is made of, the tail alone, and the whole decoder.
  parts    the stock tail's forward on the channels-last tensor the routed upsamplings hand over, piece by piece: the layout copy back
           to NCHW, the padded copy (ReflectionPad2d(3)), MIOpen's convolution with C_out = 1 or 3, npvp_bias_act; and one npvp_amax pass
           over the tail's input (what the routed tail pays when its producer hands over no slot).
  tail     A = the stock FoldedConvAct behind the copy back to NCHW (copy, pad, MIOpen, npvp_bias_act), B = ops.tail7x7_packed on the
           channels-last tensor (one launch: padding as index math, bias and activation in the epilogue, NCHW out).  B's input carries
           its producer's amax slot, as in the routed decoder.  "fwd" under no_grad; "fwd+dgrad" = forward with an input that requires
           grad, then autograd.grad to the input (B: act_bwd, amax, npvp_tail7x7_dgrad_f16; dx channels-last).
  decoder  features (N, T, C, h, w) NCHW as the predictor hands them out -> frames, up3x3="hip" on both sides; "fwd" under no_grad,
           "fwd+dgrad" with the gradient to the features.  One more line per size with up3x3="stock" on both sides (B then makes one copy
           to channels-last in front of the tail).
Sizes: c1 = 320 frames of 64 x 64 x 1 (ngf 64, 3 upsamplings), c2 = 1792 frames of 64 x 64 x 3 (ngf 64, 3), c4 = 128 frames of
128 x 128 x 3 (ngf 32, 4).  Method: both routes on the same weights, warmed up at the timed shape; then the routes alternate A, B, A, B,
every timing `iters` calls between two device events.  A shape counts as FASTER only where both B timings beat both A timings.  No time
is a pass condition.  The result is what `_tail7x7_takes_hip` of npvp_amd/models/ResNetAutoEncoder.py cites
(profiles/frozen_tail7x7_bench.txt).
Usage: python tools/frozen_tail7x7_bench.py [--iters 20] [--sizes c1,c2,c4] [--out FILE]"""
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
    "c1": (dict(ngf=64, n_downsampling=3, num_res_blocks=2, out_layer="Tanh", learn_3d=False), 1, (32, 10), 64),
    "c2": (dict(ngf=64, n_downsampling=3, num_res_blocks=2, out_layer="Tanh", learn_3d=False), 3, (64, 28), 64),
    "c4": (dict(ngf=32, n_downsampling=4, num_res_blocks=3, out_layer="Tanh", learn_3d=False), 3, (8, 16), 128),
}


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


def fwd_bwd(fn, x, g, slot=None):
    """forward with an input that requires grad (carrying its producer's amax slot where one is given), then the gradient to it"""
    def run():
        xg = ops.tag_amax(x.detach().requires_grad_(), slot)
        (dx,) = torch.autograd.grad(fn(xg), xg, g)
        return dx
    return run


def decoder(AE, ch, up3x3, tail7x7):
    enc, dec = npvp_amd.build_frozen_autoencoder(AE, ch)
    O.key_hashed_fill(dec, 121)
    return npvp_amd.to_device_layout(enc, dec, DEV, up3x3=up3x3, tail7x7=tail7x7)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", default="c1,c2,c4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frozen_tail7x7_bench needs an MI355X: a CPU run gives no time")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"frozen_tail7x7_bench on {torch.cuda.get_device_name(0)}: A = tail7x7=\"stock\" (copy to NCHW, padded copy, MIOpen, npvp_bias_act), "
        f"B = tail7x7=\"hip\" (npvp_tail7x7_f16, backward npvp_tail7x7_dgrad_f16); order A B A B; FASTER = both B below both A")
    for name in args.sizes.split(","):
        AE, ch, (N, T), side = SIZES[name]
        frames, n_up, C = N * T, AE["n_downsampling"], AE["ngf"]
        decs = {(up, tail): decoder(AE, ch, up, tail) for up in ("hip", "stock") for tail in ("stock", "hip")}
        ms, mh = decs[("hip", "stock")].model[-1], decs[("hip", "hip")].model[-1]
        assert mh.tail7x7 and not ms.tail7x7 and ms.weight.is_contiguous()
        xcl = O.seeded_randn((frames, C, side, side), 21).clamp_min(0).to(DEV).contiguous(memory_format=torch.channels_last)
        g = O.seeded_randn((frames, ch, side, side), 22).to(DEV)
        slot = ops.amax_of(xcl.permute(0, 2, 3, 1).reshape(-1, C))
        ops.tag_amax(xcl, slot)
        gb = xcl.numel() * 4 / 1e9
        # ---- what the stock forward is made of
        with torch.no_grad():
            xn = xcl.contiguous()
            xp = ms.pad(xn)
            yc = F.conv2d(xp, ms.weight)
            parts = [("copy to NCHW", lambda: xcl.contiguous()), ("padded copy", lambda: ms.pad(xn)),
                     ("MIOpen convolution", lambda: F.conv2d(xp, ms.weight)), ("npvp_bias_act", lambda: ops.bias_act(yc, ms.bias, ms.act)),
                     ("npvp_amax over the input", lambda: ops.amax_of(xcl.detach().permute(0, 2, 3, 1).reshape(-1, C)))]
            for _, fn in parts:
                fn(); fn()
            torch.cuda.synchronize()
            say(f"parts {name}: {frames} frames of {side}x{side}, C_in {C} -> {ch} (input {gb:.2f} GB), stock forward: " +
                ", ".join(f"{what} {timed(fn, args.iters):.3f} ms" for what, fn in parts))
        del xn, xp, yc, parts
        # ---- the tail alone
        stock = lambda t: ms(t.contiguous())
        hip = lambda t: mh(t)
        sb, hb = fwd_bwd(stock, xcl, g), fwd_bwd(hip, xcl, g, slot)
        for _ in range(2):
            with torch.no_grad():
                ys, yh = stock(xcl), hip(xcl)
            ds, dh = sb(), hb()
        torch.cuda.synchronize()
        assert yh.is_contiguous() and dh.permute(0, 2, 3, 1).is_contiguous()
        gmac = frames * side * side * 49 * C * ch / 1e9
        head = f"tail {name}: C_in {C} -> {ch}, {frames} frames of {side}x{side} ({gmac:.1f} GMAC, input {gb:.2f} GB)"
        with torch.no_grad():
            a, b, verdict = abab(lambda: stock(xcl), lambda: hip(xcl), args.iters)
        say(f"{head} fwd      : A {a[0]:7.3f} {a[1]:7.3f} ms, B {b[0]:7.3f} {b[1]:7.3f} ms ({gb / min(b):5.2f} TB/s of input at the best B): {verdict}; "
            f"hip vs stock rel-L2 {rel(yh, ys):.2e}")
        a, b, verdict = abab(sb, hb, args.iters)
        say(f"{head} fwd+dgrad: A {a[0]:7.3f} {a[1]:7.3f} ms, B {b[0]:7.3f} {b[1]:7.3f} ms: {verdict}; dx hip vs stock rel-L2 {rel(dh, ds):.2e}")
        del xcl, g, ys, yh, ds, dh, sb, hb
        torch.cuda.empty_cache()
        # ---- the whole decoder
        feats = O.seeded_randn((N, T, C << n_up, side >> n_up, side >> n_up), 5).clamp_min(0).to(DEV)
        gy = O.seeded_randn((N, T, ch, side, side), 6).to(DEV)
        for up in ("hip", "stock"):
            da, db = decs[(up, "stock")], decs[(up, "hip")]
            fa, fb = fwd_bwd(da, feats, gy), fwd_bwd(db, feats, gy)
            for _ in range(2):                                   # warm-up at the timed shape (solver search, code objects, workspaces)
                with torch.no_grad():
                    oa, ob = da(feats), db(feats)
                ga, gb_ = fa(), fb()
            torch.cuda.synchronize()
            head = f"decoder {name}: AE {AE['ngf']}/{n_up}, {frames} frames of {side}x{side}x{ch}, up3x3={up}"
            if up == "hip":
                with torch.no_grad():
                    a, b, verdict = abab(lambda: da(feats), lambda: db(feats), args.iters)
                say(f"{head} fwd      : A {a[0]:7.2f} {a[1]:7.2f} ms, B {b[0]:7.2f} {b[1]:7.2f} ms: {verdict}; hip vs stock frames rel-L2 "
                    f"{rel(ob, oa):.2e}")
            a, b, verdict = abab(fa, fb, args.iters)
            say(f"{head} fwd+dgrad: A {a[0]:7.2f} {a[1]:7.2f} ms, B {b[0]:7.2f} {b[1]:7.2f} ms: {verdict}; frames rel-L2 {rel(ob, oa):.2e}, "
                f"feature gradient hip vs stock rel-L2 {rel(gb_, ga):.2e}")
            del oa, ob, ga, gb_, fa, fb
        del decs, feats, gy
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
