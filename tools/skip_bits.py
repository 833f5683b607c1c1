"""A fingerprint of the DropPath-skip plumbing of npvp_amd/ops.py and sched.py: one encoder block (spatial self-attention sub-layer +
MlpDWBN, drop_path 0.25, 8 clips x T frames x 8 x 8 x 512 - the block of tests/test_hip_wgrad_rowskip.py) forward + backward on flat
gradient buffers, at T = 4 and T = 2, under the four settings of ops.DROP_PATH_SKIP / ops.WGRAD_ROW_SKIP and four schedules:

    stream    the gradient stream (weight gradients chained inside its flush)
    fused     single stream, the fused dgrad + weight-gradient launch on
    chained   single stream, the fused launch off (chained weight gradients on the current stream)
    unchained the gradient stream with the chain off (every weight gradient through ops.gemm, a reduction launch each)

Per case one line: a SHA-256 over y, dx and every parameter gradient, and the library launches of the step (npvp_launch_count).  The
seed is the first below 400 in which one of the block's two DropPath sites drops some but not all of its samples.  Two checkouts that
print the same 32 lines hand the same skip words to the same launches: run it before and after a change of that host code that is
meant to move no bit and no launch.  It uses only names both sides of such a change have.  Needs a GPU.

    python tools/skip_bits.py [--tree path/to/another/checkout]      (built: its npvp_amd/libnpvp_hip.so is loaded)"""
import argparse
import hashlib
import os
import sys

import torch

SCHEDULES = {"stream": (True, False, True), "fused": (False, True, True), "chained": (False, False, True),
             "unchained": (True, False, False)}           # WgradStream.enabled, FusedLinearBwd.enabled, WgradChain.enabled
DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to import npvp_amd and oracle from")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import npvp_amd as impl
    from npvp_amd.trainer import FlatBuffers
    from oracle import ops as O
    K = impl.ops
    assert os.path.abspath(impl.__file__).startswith(os.path.abspath(a.tree)), impl.__file__
    K.set_gemm_precision("f16x3")
    dev = torch.device(DEV)
    count = impl._lib.lib().npvp_launch_count
    N = 8
    m = impl.VidHRFormerBlockEnc(8, 8, 512, 8, 4, 0.0, 0.25, 4, 1024)
    O.key_hashed_fill(m, 751)
    m = m.to(DEV).train()
    fb = FlatBuffers(m)
    fuser = impl.PosFeatFuser(512, 'layer')
    print(f"# {torch.cuda.get_device_name(0)}, ROCm {torch.version.hip}")
    for T in (4, 2):
        x = O.synth_features((N, T, 8, 8, 512), 752).to(DEV).requires_grad_()
        beta = (0.5 * O.seeded_randn((T * 64, 512), 753)).to(DEV)
        cot = O.seeded_randn((N, T, 8, 8, 512), 754).to(DEV)
        K.DropRecorder.sites = []
        try:
            with torch.no_grad():
                K.rng.manual_seed(0, dev)
                K.rng.begin_step(dev)
                m(x, (beta, None), fuser)
            sites = [s for s in K.DropRecorder.sites if s[1] == "group"]
        finally:
            K.DropRecorder.sites = None
        assert len(sites) == 2
        for seed in range(400):
            K.rng.manual_seed(seed, dev)
            K.rng.begin_step(dev)
            kept = [int((K.DropRecorder.mask(s, dev) != 0).sum()) for s in sites]
            if any(0 < k < N for k in kept):
                break
        else:
            raise SystemExit("no seed below 400 in which a site drops some but not all samples")
        keep = (K.DROP_PATH_SKIP, K.WGRAD_ROW_SKIP, K.WgradStream.enabled, K.FusedLinearBwd.enabled, K.WgradChain.enabled)
        try:
            for name, (stream, fused, chain) in SCHEDULES.items():
                for dp_skip in (False, True):
                    for wg_skip in (False, True):
                        K.WgradStream.join()
                        K.DROP_PATH_SKIP, K.WGRAD_ROW_SKIP = dp_skip, wg_skip
                        K.WgradStream.enabled, K.FusedLinearBwd.enabled, K.WgradChain.enabled = stream, fused, chain
                        fb.flat_g.zero_()
                        x.grad = None
                        K.rng.manual_seed(seed, dev)
                        K.rng.begin_step(dev)
                        torch.cuda.synchronize()
                        n0 = count()
                        y = m(x, (beta, None), fuser)
                        (y * cot).sum().backward()
                        K.ReduceQueue.finish()
                        K.WgradStream.join()
                        torch.cuda.synchronize()
                        n = count() - n0
                        h = hashlib.sha256()
                        for t in [y.detach(), x.grad] + [p.grad for _, p in sorted(m.named_parameters())]:
                            h.update(b"none" if t is None else t.detach().contiguous().cpu().numpy().tobytes())
                        print(f"T {T} seed {seed:3d} kept {kept[0]}/{N} {kept[1]}/{N}  {name:9s} DROP_PATH_SKIP {int(dp_skip)} WGRAD_ROW_SKIP {int(wg_skip)}  "
                              f"launches {n:4d}  {h.hexdigest()}", flush=True)
        finally:
            K.WgradStream.join()
            K.DROP_PATH_SKIP, K.WGRAD_ROW_SKIP, K.WgradStream.enabled, K.FusedLinearBwd.enabled, K.WgradChain.enabled = keep


if __name__ == "__main__":
    main()
