"""Decoder of the fused frozen pair, to_device_layout(..., up3x3="stock") against up3x3="hip", in ONE process: each distinct
transposed 3 x 3 convolution alone, the whole decoder, and the routed decoder's 7 x 7 tail in both layouts.
  conv     A = F.conv_transpose2d (MIOpen, fp32, NCHW as the stock decoder runs it) + ops.bias_act; B = ops.convt3x3s2_packed on
           channels-last frames (one f16x3 launch, the transposed form of csrc/conv3x3.hip).  B's input carries no amax slot: every B
           call includes its npvp_amax pass (in the decoder only the first routed convolution pays it).  "fwd" under no_grad; "fwd+dgrad"
           = forward with an input that requires grad, then autograd.grad to the input (B: act_bwd, amax, npvp_conv3x3s2_f16).
  decoder  features (N, T, C, h, w) NCHW as the predictor hands them out -> frames; "fwd" under no_grad, "fwd+dgrad" with the
           gradient to the features.  B includes its copy to channels-last at the entry and the reshape of the result.
  tail     the routed decoder with its stock remainder (the 7 x 7 tail; ngf = 32: the 64 -> 32 transposed convolution in front of it) on
           the channels-last tensor (A = UP3X3_TAIL "nhwc") against NCHW weights behind one copy back to NCHW (B = "nchw"), forward +
           input gradient of the whole decoder.
Sizes: c1 = 320 frames of 64 x 64 x 1 (ngf 64, 3 upsamplings; N Tp of KTH B = 32), c2 = 1792 frames of 64 x 64 x 3 (ngf 64, 3; BAIR
B = 64, Tp = 28), c4 = 128 frames of 128 x 128 x 3 (ngf 32, 4: the last upsampling, 64 -> 32, stays stock; the KITTI shard).  Method:
both routes on the same weights, warmed up at the timed shape; then the routes alternate A, B, A, B, every timing `iters` calls between
two device events.  A shape counts as FASTER only where both B timings beat both A timings.  No time is a pass condition.  The result is
what the eligibility rule `_up3x3_takes_hip` and UP3X3_TAIL of npvp_amd/models/ResNetAutoEncoder.py cite
(profiles/frozen_up3x3_bench.txt).
Usage: python tools/frozen_up3x3_bench.py [--iters 20] [--conv-iters 200] [--sizes c1,c2,c4] [--out FILE]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import npvp_amd
from npvp_amd import ops
from npvp_amd.models import ResNetAutoEncoder as RAE
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


def fwd_bwd(fn, x, g):
    """forward with an input that requires grad, then the gradient to it"""
    def run():
        xg = x.detach().requires_grad_()
        (dx,) = torch.autograd.grad(fn(xg), xg, g)
        return dx
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--conv-iters", type=int, default=200)
    ap.add_argument("--sizes", default="c1,c2,c4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frozen_up3x3_bench needs an MI355X: a CPU run gives no time")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"frozen_up3x3_bench on {torch.cuda.get_device_name(0)}: A = up3x3=\"stock\" (MIOpen NCHW + npvp_bias_act), B = up3x3=\"hip\" "
        f"(npvp_convt3x3s2_f16, backward npvp_conv3x3s2_f16); order A B A B; FASTER = both B below both A")
    for name in args.sizes.split(","):
        AE, ch, (N, T), side = SIZES[name]
        frames, n_up = N * T, AE["n_downsampling"]
        grid0 = side >> n_up
        for i in range(n_up):
            Ci, Co, S = AE["ngf"] << (n_up - i), AE["ngf"] << (n_up - i - 1), grid0 << i
            if not ops.convt3x3s2_takes(Ci, Co):
                say(f"conv {name} {Ci:3d} -> {Co:3d} grid {S}x{S}: outside the channel rule, stays stock")
                continue
            x = O.seeded_randn((frames, Ci, S, S), 11).to(DEV)
            xcl = x.contiguous(memory_format=torch.channels_last)
            w = (O.seeded_randn((Ci, Co, 3, 3), 12) * (9 * Ci / 4) ** -0.5).to(DEV)
            b = O.seeded_randn((Co,), 13).to(DEV)
            g = O.seeded_randn((frames, Co, 2 * S, 2 * S), 14).to(DEV)
            gcl = g.contiguous(memory_format=torch.channels_last)
            planes = ops.convt3x3s2_planes(w)
            gmac = frames * S * S * 9 * Ci * Co / 1e9
            stock = lambda t: ops.bias_act(F.conv_transpose2d(t, w, None, 2, 1, 1), b, 1)
            hip = lambda t: ops.convt3x3s2_packed(t, planes, b, 1)
            sb, hb = fwd_bwd(stock, x, g), fwd_bwd(hip, xcl, gcl)
            for _ in range(3):
                with torch.no_grad():
                    ys, yh = stock(x), hip(xcl)
                ds, dh = sb(), hb()
            torch.cuda.synchronize()
            with torch.no_grad():
                a, bb, verdict = abab(lambda: stock(x), lambda: hip(xcl), args.conv_iters)
            say(f"conv {name} {Ci:3d} -> {Co:3d} grid {S:2d}x{S:<2d} frames {frames} ({gmac:5.1f} GMAC) fwd      : A {a[0]:7.3f} {a[1]:7.3f} ms, "
                f"B {bb[0]:7.3f} {bb[1]:7.3f} ms ({2 * gmac / min(bb):6.1f} TFLOP/s fp32-equivalent at the best B): {verdict}; "
                f"hip vs stock rel-L2 {rel(yh, ys):.2e}")
            a, bb, verdict = abab(sb, hb, args.conv_iters)
            say(f"conv {name} {Ci:3d} -> {Co:3d} grid {S:2d}x{S:<2d} frames {frames} ({2 * gmac:5.1f} GMAC) fwd+dgrad: A {a[0]:7.3f} {a[1]:7.3f} ms, "
                f"B {bb[0]:7.3f} {bb[1]:7.3f} ms: {verdict}; dx hip vs stock rel-L2 {rel(dh, ds):.2e}")
            del x, xcl, w, g, gcl, planes, ys, yh, ds, dh
            torch.cuda.empty_cache()
        C = AE["ngf"] << n_up
        feats = O.seeded_randn((N, T, C, grid0, grid0), 5).clamp_min(0).to(DEV)
        gy = O.seeded_randn((N, T, ch, side, side), 6).to(DEV)
        decs = {}
        for r in RAE.UP3X3_ROUTES:
            enc, dec = npvp_amd.build_frozen_autoencoder(AE, ch)
            O.key_hashed_fill(dec, 121)
            decs[r] = npvp_amd.to_device_layout(enc, dec, DEV, up3x3=r)[1]
            del enc
        fb = {r: fwd_bwd(decs[r], feats, gy) for r in decs}
        out, dout = {}, {}
        for r in decs:
            for _ in range(2):                                   # warm-up at the timed shape (solver search, code objects, workspaces)
                with torch.no_grad():
                    out[r] = decs[r](feats)
                dout[r] = fb[r]()
        torch.cuda.synchronize()
        head = (f"decoder {name}: AE {AE['ngf']}/{n_up}, {frames} frames of {side}x{side}x{ch}, tail {RAE.UP3X3_TAIL}")
        with torch.no_grad():
            a, b, verdict = abab(lambda: decs["stock"](feats), lambda: decs["hip"](feats), args.iters)
        say(f"{head} fwd      : A {a[0]:7.2f} {a[1]:7.2f} ms, B {b[0]:7.2f} {b[1]:7.2f} ms: {verdict}; hip vs stock frames rel-L2 "
            f"{rel(out['hip'], out['stock']):.2e}")
        a, b, verdict = abab(fb["stock"], fb["hip"], args.iters)
        say(f"{head} fwd+dgrad: A {a[0]:7.2f} {a[1]:7.2f} ms, B {b[0]:7.2f} {b[1]:7.2f} ms: {verdict}; feature gradient hip vs stock rel-L2 "
            f"{rel(dout['hip'], dout['stock']):.2e}")
        # the layout of the stock remainder (the 7 x 7 tail; ngf = 32: the 64 -> 32 transposed convolution too), two routed decoders
        keep, tails = RAE.UP3X3_TAIL, {}
        try:
            for layout in ("nhwc", "nchw"):
                RAE.UP3X3_TAIL = layout
                enc, dec = npvp_amd.build_frozen_autoencoder(AE, ch)
                O.key_hashed_fill(dec, 121)
                tails[layout] = fwd_bwd(npvp_amd.to_device_layout(enc, dec, DEV, up3x3="hip")[1], feats, gy)
                del enc
        finally:
            RAE.UP3X3_TAIL = keep
        for layout in tails:
            for _ in range(2):
                tails[layout]()
        torch.cuda.synchronize()
        a, b, verdict = abab(tails["nhwc"], tails["nchw"], args.iters)
        say(f"tail {name}: routed decoder fwd+dgrad, stock remainder on the channels-last tensor A {a[0]:7.2f} {a[1]:7.2f} ms, behind one copy "
            f"to NCHW B {b[0]:7.2f} {b[1]:7.2f} ms: nchw is {verdict}")
        del decs, out, dout, feats, gy, fb, tails
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
