"""Stage-1 autoencoder training step (LitAE, ref/models/ResNetAutoEncoder.py:27-49): the HIP path (prepare_trainable_autoencoder +
ae_train_step + FlatAdamW) against the stock path (the same modules in train mode on PyTorch-ROCm + torch.optim.Adam) at a config's
real batch, on the same seeded weights and frames.  One JSON line: ms per step, peak allocated memory, loss of each path and their
relative difference, and the algorithmic bytes of the new BatchNorm / attention kernels per step (for a share of the HBM peak from a
separate `rocprofv3 --kernel-trace --stats` run).
--dp adds two paths on a forced group of ONE rank over RCCL, where every collective is a real RCCL call that leaves the values
unchanged - what the data-parallel machinery costs a step beyond its transfers: "hip_gs" = GradSync's bucket all-reduces alone
(plain BatchNorm), "hip_dp" = ae_data_parallel (GradSync + synchronised BatchNorm's two small all-reduces per layer).  With --repeats R the paths are timed R times in
alternation and every window is reported.
--size H W trains at H x W frames (each a multiple of 2**n_downsampling) instead of the config's own: off the configs' sizes the
HIP path's attention runs the any-grid kernels (ops.nonlocal_attn_grid_packed), the stock path materialises its H W x H W / 4 scores.
--learn-3d flips learn_3d in the chosen config (the shipped dicts stay as they are): every Factorized3DConvAttn block gains its temporal
Conv1d and NonLocalAttenion1D (csrc/ae_temporal.hip on the HIP path, permute copies + batched matmuls on the stock path); the record
then also holds the temporal attention kernels' own time per step (forward + backward at every block's shape, timed alone) next to
the reference's route for the same core (permute copies to (N H W, T, d) sequences, batched matmuls and softmax, permute back).
--frames T overrides the config's clip length (like --size its frame size): above ops.TEMPORAL_ATTN_MAX_T = 32 frames the HIP path's
temporal attention runs the key-tiled kernels (ops.temporal_attn_long_packed), e.g. KTH's evaluation clips of 40 and 50 frames.
Usage: python tools/ae_train_bench.py --config {BAIR,KTH,KITTI} [--steps 10] [--warmup 3] [--batch B] [--size H W] [--dp] [--repeats R]
                                      [--paths hip,hip_gs,hip_dp] [--learn-3d] [--frames T]"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                      # noqa: E402
import torch.nn as nn             # noqa: E402

# the AE: sections and Dataset batch / clip lengths of ref/configs/config_{BAIR,KTH,KITTI}_Autoencoder.yaml
CONFIGS = {
    "BAIR": dict(AE=dict(ngf=64, n_downsampling=3, num_res_blocks=2, out_layer='Tanh', learn_3d=False), ch=3, S=64, B=8, T=12),
    "KTH": dict(AE=dict(ngf=64, n_downsampling=3, num_res_blocks=2, out_layer='Tanh', learn_3d=False), ch=1, S=64, B=8, T=20),
    "KITTI": dict(AE=dict(ngf=32, n_downsampling=4, num_res_blocks=3, out_layer='Tanh', learn_3d=False), ch=3, S=128, B=16, T=9),
}


def algorithmic_bytes(enc, dec, frames, H, W):
    """HBM bytes the new kernels must move per step at minimum (fp32): BatchNorm forward = stats read + apply read / write
    (+ residual read), backward = sum pass (x, g) + dx pass (x, g, dx); attention = q, k, v read + o written forward, q, k, v, o,
    dO read + dq, dk, dv written backward (the score matrix stays on chip).  The shapes come from a one-frame probe of COPIES in
    eval mode: the modules passed in are left as they are (running statistics included)."""
    enc, dec = copy.deepcopy(enc).eval(), copy.deepcopy(dec).eval()
    from npvp_amd.models.ResNetAutoEncoder import NonLocalAttenion2D, NonLocalAttenion1D
    # BatchNorm element counts from the conv outputs of a one-frame probe
    counts = []

    def bn_hook(m, inp, out):
        counts.append(inp[0].numel())
    hs = [m.register_forward_hook(bn_hook) for m in list(enc.modules()) + list(dec.modules()) if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d))]
    att = []

    def at_hook(m, inp, out):
        N, C, h, w = inp[0].shape
        att.append(h * w * (2 * (C // 8) + C // 2 + C // 2))
    hs += [m.register_forward_hook(at_hook) for m in enc.modules() if isinstance(m, NonLocalAttenion2D)]

    def at1_hook(m, inp, out):
        M, C, T = inp[0].shape                                  # (pixels of the one-frame probe, C, 1)
        att.append(M * T * (2 * (C // 8) + C // 2 + C // 2))
    hs += [m.register_forward_hook(at1_hook) for m in enc.modules() if isinstance(m, NonLocalAttenion1D)]
    with torch.no_grad():
        dec(enc(torch.zeros(1, 1, enc.block0[1].in_channels, H, W)))
    for h in hs:
        h.remove()
    bn = 4 * frames * sum(n * (1 + 2) + n * 2 + n * 3 for n in counts)           # fwd 3 passes-worth, bwd 5 (residual not counted)
    attn = 4 * frames * sum(e + 2 * e + e for e in att)                            # fwd q,k,v,o ; bwd q,k,v,o,dO + dq,dk,dv
    return bn, attn


def temporal_kernel_ms(enc, B, T, H, W, iters=20):
    """ms per training step spent in the temporal attention kernels alone: forward + backward of ops.temporal_attn_packed (above 32
    frames ops.temporal_attn_long_packed) at every learn_3d block's (C, grid), timed with device events over `iters` calls each (after
    3 warm-up calls), summed over the blocks; per block also the reference's route for the same core on the same rows (permute copies
    to (N*HW, T, d), softmax(q k^T) v as batched matmuls, permute back; forward + backward), which the stock path runs"""
    import npvp_amd
    from npvp_amd.models.ResNetAutoEncoder import Factorized3DConvAttn
    shapes = []

    def hook(m, inp, out):
        shapes.append((inp[0].shape[1], inp[0].shape[2] * inp[0].shape[3]))
    probe = copy.deepcopy(enc).eval()
    hs = [m.register_forward_hook(hook) for m in probe.modules() if isinstance(m, Factorized3DConvAttn) and m.learn_3d]
    with torch.no_grad():
        probe(torch.zeros(1, 1, probe.block0[1].in_channels, H, W))
    for h in hs:
        h.remove()
    total, per = 0.0, []
    for C, HW in shapes:
        A, V = C // 8, C // 2
        ld = 2 * A + V + (-(2 * A + V) % 32)
        qkv = (0.3 * torch.randn(B * T * HW, ld, device="cuda:0")).requires_grad_()
        go = torch.randn(B * T * HW, V, device="cuda:0")
        run = lambda: npvp_amd.ops.temporal_attn_any_packed(qkv, B, T, HW, A, V).backward(go)

        def stock():
            seq = lambda t: t.reshape(B, T, HW, -1).permute(0, 2, 1, 3).reshape(B * HW, T, -1).contiguous()
            q, k, v = seq(qkv[:, :A]), seq(qkv[:, A:2 * A]), seq(qkv[:, 2 * A:2 * A + V])
            o = torch.softmax(q @ k.transpose(1, 2), -1) @ v
            o.reshape(B, HW, T, V).permute(0, 2, 1, 3).reshape(B * T * HW, V).contiguous().backward(go)

        def timed(fn):
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters
        ms = timed(run)
        per.append({"C": C, "HW": HW, "T": T, "fwd_bwd_ms": round(ms, 4), "stock_route_fwd_bwd_ms": round(timed(stock), 4)})
        total += ms
    return round(total, 4), per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="BAIR")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--size", type=int, nargs=2, default=None, metavar=("H", "W"),
                    help="frame height and width, each a multiple of 2**n_downsampling (default: the config's own square size)")
    ap.add_argument("--paths", default=None, help="comma list of stock, hip, hip_gs, hip_dp (default: stock,hip; with --dp also hip_gs,hip_dp)")
    ap.add_argument("--one-context", action="store_true",
                    help="build every trainer on the process's default scheduling context instead of one context per path")
    ap.add_argument("--dp", action="store_true", help="also time the HIP step on a forced one-rank RCCL group (paths hip_gs, hip_dp)")
    ap.add_argument("--repeats", type=int, default=1, help="timed windows per path, the paths alternating")
    ap.add_argument("--learn-3d", action="store_true", help="flip learn_3d in the chosen config: the spatio-temporal autoencoder")
    ap.add_argument("--frames", type=int, default=None, metavar="T", help="frames per clip (default: the config's own clip length)")
    a = ap.parse_args()
    paths = a.paths.split(",") if a.paths else ["stock", "hip"] + (["hip_gs", "hip_dp"] if a.dp else [])
    if not a.dp and any(p in ("hip_gs", "hip_dp") for p in paths):
        raise SystemExit("paths hip_gs / hip_dp need --dp")
    if a.dp:        # (read when npvp_amd.dp is imported / the process group is made)
        os.environ.setdefault("NPVP_DP_FORCE", "1")
        os.environ.setdefault("NPVP_DIST_BACKEND", "nccl")
        os.environ.setdefault("MASTER_PORT", "29541")
    import npvp_amd
    from oracle import ops as O
    if not torch.cuda.is_available():
        raise SystemExit("ae_train_bench needs an MI355X")
    cfg = CONFIGS[a.config]
    if a.learn_3d:
        cfg = dict(cfg, AE=dict(cfg["AE"], learn_3d=True))
    B, T, ch = a.batch or cfg["B"], a.frames or cfg["T"], cfg["ch"]
    if T < 2:
        raise SystemExit("--frames: a clip has at least 2 frames (past and future)")
    H, W = a.size or (cfg["S"], cfg["S"])
    down = 2 ** cfg["AE"]["n_downsampling"]
    if H < down or W < down or H % down or W % down:
        raise SystemExit(f"--size: H and W must be multiples of 2**n_downsampling = {down}")
    dev = "cuda:0"
    enc0, dec0 = npvp_amd.build_autoencoder(cfg["AE"], ch)
    O.key_hashed_fill(npvp_amd.AEPair(enc0, dec0), 1)
    x = torch.tanh(O.seeded_randn((B, T, ch, H, W), 2)).to(dev)
    past, fut = x[:, : T // 2].contiguous(), x[:, T // 2:].contiguous()
    out = {"config": a.config, "batch": B, "frames_per_step": B * T, "frames_per_clip": T, "res": H if H == W else [H, W]}
    out["bn_bytes_per_step"], out["attn_bytes_per_step"] = algorithmic_bytes(enc0, dec0, B * T, H, W)
    if a.learn_3d:
        out["learn_3d"] = True
        out["temporal_attn_kernels_ms_per_step"], out["temporal_attn_kernels"] = temporal_kernel_ms(enc0, B, T, H, W)
    losses, steps = {}, {}
    for path in paths:
        enc, dec = copy.deepcopy(enc0), copy.deepcopy(dec0)
        if path == "stock":
            enc, dec = enc.to(dev), dec.to(dev)
            opt = torch.optim.Adam(list(enc.parameters()) + list(dec.parameters()), lr=1e-4, betas=(0.5, 0.999))

            def step(enc=enc, dec=dec, opt=opt):        # (bound now: with --repeats the step outlives this iteration's names)
                opt.zero_grad()
                xx = torch.cat([past, fut], 1)
                loss = (dec(enc(xx)) - xx).abs().mean()
                loss.backward()
                opt.step()
                return loss.detach()
        else:
            enc, dec = enc.to(dev).to(memory_format=torch.channels_last), dec.to(dev)
            npvp_amd.prepare_trainable_autoencoder(enc, dec)
            # (a scheduling context per path: each GradSync listens on its own trainer's gradient sink)
            with npvp_amd.ops.use(None if a.one_context else npvp_amd.ops.StepContext(path)):
                opt = npvp_amd.ae_optimizer(enc, dec, lr=1e-4)
            gs = None
            if path in ("hip_gs", "hip_dp"):
                from npvp_amd import dp
                dp.init_distributed()
                if path == "hip_dp":
                    gs = npvp_amd.ae_data_parallel(enc, dec, opt)
                else:
                    dp.broadcast_module(opt.ae_pair)
                    gs = dp.GradSync(opt)
                assert gs is not None and gs.on, "--dp: the one-rank process group did not come up"
                out["dp"] = {"backend": torch.distributed.get_backend(), "world_size": gs.world, "buckets": len(gs.buckets),
                             "sync_batchnorm_layers": sum(isinstance(m, dp.SyncBatchNorm2d) for m in opt.ae_pair.modules())}
            step = lambda enc=enc, dec=dec, opt=opt, gs=gs: npvp_amd.ae_train_step(enc, dec, opt, past, fut, grad_sync=gs)
        first = float(step())
        losses[path] = first
        for _ in range(max(a.warmup - 1, 0)):
            step()
        torch.cuda.synchronize()
        out[f"{path}_loss_step1"] = first
        steps[path] = step
        if a.repeats > 1:
            continue
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        out[f"{path}_ms_per_step"] = round((time.perf_counter() - t0) * 1e3 / a.steps, 3)
        out[f"{path}_peak_alloc_MiB"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
        del enc, dec, opt, step, steps[path]
        torch.cuda.empty_cache()
    if a.repeats > 1:       # every path stays resident and warm; the windows alternate so that drift of the host hits all alike
        windows = {path: [] for path in steps}
        for _ in range(a.repeats):
            for path, step in steps.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step()
                torch.cuda.synchronize()
                windows[path].append(round((time.perf_counter() - t0) * 1e3 / a.steps, 3))
        for path, w in windows.items():
            out[f"{path}_ms_per_step"] = sorted(w)[len(w) // 2]
            out[f"{path}_ms_per_step_windows"] = w
    if "stock" in losses and "hip" in losses:
        out["loss_rel_diff"] = abs(losses["hip"] - losses["stock"]) / abs(losses["stock"])
    print(json.dumps(out))
    if a.dp and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
