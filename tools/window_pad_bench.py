"""What the centre-pad route of spatial window attention costs (ref/models/VidHRFormer.py:488-511).  Needs an MI355X.  JSON lines.

  kernels  npvp_grid_center_pad / npvp_grid_center_cut alone through the C ABI at one shape (default: KTH's native 120 x 160 frames,
           a 15 x 20 grid padded to 16 x 20, 64 clips x 30 frames, C = 512): microseconds per call between device events and the
           bytes each call must move (pad: reads F*H*W rows, writes rows_out; cut: reads F*H*W rows (+ the addend), writes F*H*W)
           over that time, beside the float4-copy rate measured on this part (6.29 TB/s, MI355X_MICROARCH).
  step     the KTH NPVP-S predictor training step (batch 8, 10 + 10 frames, 4 + 8 layers, window 4) at a grid the window does not
           tile beside the same step at the next tiling grid (default 15 x 20 and 16 x 20), alternating A, B, A, B in one process:
           milliseconds per eager step between device events.

Usage: python tools/window_pad_bench.py kernels [--frames 1920 --H 15 --W 20 --ws 4 --C 512 --iters 200]
       python tools/window_pad_bench.py step [--H 15 --W 20 --ws 4 --batch 8 --steps 10 --rounds 2]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                      # noqa: E402

COPY_PEAK = 6.29e12               # bytes / s, float4 copy measured on the MI355X


def timed(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters          # ms


def kernels(a):
    import npvp_amd
    from npvp_amd._lib import lib, check
    L = lib()
    Fr, H, W, C = a.frames, a.H, a.W, a.C
    Hp, Wp, top, left = npvp_amd.ops.window_pad_geometry(H, W, a.ws)
    rows, rows_out = Fr * H * W, -(-Fr * Hp * Wp // 32) * 32
    x, add = torch.randn(rows, C, device="cuda"), torch.randn(rows, C, device="cuda")
    xp, y = torch.empty(rows_out, C, device="cuda"), torch.empty(rows, C, device="cuda")
    slot = torch.zeros(512, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    geom = (Fr, H, W, Hp, Wp, top, left, C)

    def pad(s=None):
        check(L.npvp_grid_center_pad(x.data_ptr(), C, xp.data_ptr(), C, *geom, rows_out, s, st), "npvp_grid_center_pad")

    def cut(ad=None, s=None):
        check(L.npvp_grid_center_cut(xp.data_ptr(), C, ad, C, y.data_ptr(), C, *geom, s, st), "npvp_grid_center_cut")
    for name, fn, nbytes in (("pad", pad, 4 * C * (rows + rows_out)), ("pad+amax", lambda: pad(slot.data_ptr()), 4 * C * (rows + rows_out)),
                             ("cut", cut, 4 * C * 2 * rows), ("cut+amax", lambda: cut(None, slot.data_ptr()), 4 * C * 2 * rows),
                             ("cut+addend", lambda: cut(add.data_ptr()), 4 * C * 3 * rows)):
        ms = timed(fn, a.iters)
        rate = nbytes / (ms * 1e-3)
        print(json.dumps({"kernel": name, "frames": Fr, "grid": [H, W], "padded": [Hp, Wp], "C": C, "rows_out": rows_out,
                          "us": round(ms * 1e3, 2), "bytes": nbytes, "TB_per_s": round(rate / 1e12, 3),
                          "share_of_float4_copy_rate": round(rate / COPY_PEAK, 3)}))


def step(a):
    import npvp_amd
    from oracle import ops as O
    Hp, Wp, _, _ = npvp_amd.ops.window_pad_geometry(a.H, a.W, a.ws)
    B, To, Tp = a.batch, 10, 10
    runs = {}
    for H, W in ((a.H, a.W), (Hp, Wp)):
        to, tp = torch.linspace(0, To - 1, To), torch.linspace(To, To + Tp - 1, Tp)
        m = npvp_amd.Predictor(H, W, To + Tp, torch.linspace(0, H - 1, H), torch.linspace(0, W - 1, W), to, tp, 512, 'Add', 'layer', 256,
                               1, True, 8, window_size=a.ws, evt_former=True, learn_evt_token=False, evt_former_num_layers=4)
        O.key_hashed_fill(m, 7)
        m = m.cuda().train()
        opt = npvp_amd.FlatAdamW(m, lr=1e-4, clip_module=m.transformer, max_grad_norm=1.0)
        past, fut = O.synth_features((B, To, 512, H, W), 1).cuda(), O.synth_features((B, Tp, 512, H, W), 2).cuda()
        runs[(H, W)] = lambda m=m, opt=opt, past=past, fut=fut: npvp_amd.predictor_train_step(m, opt, past, fut, 0.01, 1e-8, 1.0, sync=False)
    n0 = {}
    for r in range(a.rounds):
        for grid, fn in runs.items():
            ms = timed(fn, a.steps, warm=3 if r == 0 else 1)
            c0 = npvp_amd._lib.lib().npvp_launch_count()
            fn()
            torch.cuda.synchronize()
            n0[grid] = npvp_amd._lib.lib().npvp_launch_count() - c0
            print(json.dumps({"round": r, "grid": list(grid), "token_rows_per_side": B * To * grid[0] * grid[1], "step_ms": round(ms, 3),
                              "launches_per_step": n0[grid]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "step"])
    ap.add_argument("--frames", type=int, default=64 * 30)
    ap.add_argument("--H", type=int, default=15)
    ap.add_argument("--W", type=int, default=20)
    ap.add_argument("--ws", type=int, default=4)
    ap.add_argument("--C", type=int, default=512)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_pad_bench needs an MI355X")
    kernels(a) if a.what == "kernels" else step(a)


if __name__ == "__main__":
    main()
