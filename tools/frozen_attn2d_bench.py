"""Encoder forward of the fused frozen pair, to_device_layout(..., attn2d="stock") against attn2d="hip", in ONE process at the sizes users
run: the BAIR autoencoder on 640 frames of 64 x 64 (32 clips of 10 + 10 frames, the c1 full-step size) and the KITTI autoencoder on 72
frames of 128 x 128 (one 8-clip shard of 4 + 5 frames).  Method: both routes are built on the same weights and warmed up at the timed
shape; then rounds alternate the routes, every round timing `iters` forwards of each between two device events; reported are the median
over the rounds, the spread (min .. max) and torch.cuda.max_memory_allocated of one forward of each route (peak over the level before
the call, and the absolute peak).  The outputs of the two routes are compared on the timed frames (rel-L2).  No time is a pass condition.
Usage: python tools/frozen_attn2d_bench.py [--rounds 7] [--iters 3] [--only bair|kitti]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import npvp_amd
from oracle import ops as O

DEV = "cuda:0"
SIZES = {
    "bair": (dict(ngf=64, n_downsampling=3, num_res_blocks=2, out_layer="Tanh", learn_3d=False), 3, (32, 20, 3, 64, 64)),
    "kitti": (dict(ngf=32, n_downsampling=4, num_res_blocks=3, out_layer="Tanh", learn_3d=False), 3, (8, 9, 3, 128, 128)),
}
ROUTES = ("stock", "hip")


def pair(AE, ch, route):
    enc, dec = npvp_amd.build_frozen_autoencoder(AE, ch)
    O.key_hashed_fill(enc, 121); O.key_hashed_fill(dec, 122)          # (seeded weights, a non-zero gamma: the branch is live)
    return npvp_amd.to_device_layout(enc, dec, DEV, attn2d=route)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--only", choices=sorted(SIZES), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frozen_attn2d_bench needs an MI355X: a CPU run gives no time")
    count = npvp_amd._lib.lib().npvp_launch_count
    for name, (AE, ch, shape) in SIZES.items():
        if args.only and name != args.only:
            continue
        x = torch.rand(shape, generator=torch.Generator().manual_seed(5)).to(DEV)
        encs = {r: pair(AE, ch, r) for r in ROUTES}
        out, peak, launches = {}, {}, {}
        with torch.no_grad():
            for r in ROUTES:
                for _ in range(2):                                   # warm-up at the timed shape (solver search, code objects, workspaces)
                    encs[r](x)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base, n0 = torch.cuda.memory_allocated(), count()
                out[r] = encs[r](x)
                torch.cuda.synchronize()
                peak[r] = (torch.cuda.max_memory_allocated() - base, torch.cuda.max_memory_allocated())
                launches[r] = count() - n0
            ms = {r: [] for r in ROUTES}
            for _ in range(args.rounds):
                for r in ROUTES:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.iters):
                        encs[r](x)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[r].append(e0.elapsed_time(e1) / args.iters)
        err = float((out["hip"].double() - out["stock"].double()).norm() / out["stock"].double().norm())
        frames = shape[0] * shape[1]
        print(f"{name}: AE {AE['ngf']}/{AE['n_downsampling']}/{AE['num_res_blocks']}, {frames} frames of {shape[3]}x{shape[4]}, "
              f"{args.rounds} alternating rounds of {args.iters} forwards; hip vs stock features rel-L2 {err:.2e}")
        for r in ROUTES:
            print(f"  attn2d={r:5s}: encoder forward median {statistics.median(ms[r]):8.2f} ms (min {min(ms[r]):.2f} .. max {max(ms[r]):.2f}), "
                  f"peak memory over the call's start {peak[r][0] / 2 ** 20:8.1f} MiB (absolute {peak[r][1] / 2 ** 20:.1f} MiB), "
                  f"library launches {launches[r]}")
        m = {r: statistics.median(ms[r]) for r in ROUTES}
        print(f"  hip / stock median time {m['hip'] / m['stock']:.3f} ({'hip is SLOWER here' if m['hip'] > m['stock'] else 'hip is faster here'}); "
              f"peak memory hip / stock {peak['hip'][0] / max(peak['stock'][0], 1):.3f}", flush=True)
        del encs, out, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
