"""Non-local attention core alone (ops.nonlocal_attn_grid: forward, and forward + backward) at one (C, H, W, frames): ms per call and
the worst rel-L2 of o / dq / dk / dv against float64 when --check is given.  A config shape runs the exact-tile kernels;
NPVP_NL_GRID_GENERAL=1 in the environment sends it to the masked general kernels instead, which is how the cost of the masks is
measured at a shape both forms can run.  One JSON line.
Usage: [NPVP_NL_GRID_GENERAL=1] python tools/nl_grid_bench.py --C 64 --H 64 --W 64 [--frames 8] [--iters 20] [--check]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--C", type=int, default=64)
    ap.add_argument("--H", type=int, default=64)
    ap.add_argument("--W", type=int, default=64)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    import npvp_amd
    from oracle import ops as O
    if not torch.cuda.is_available():
        raise SystemExit("nl_grid_bench needs an MI355X")
    C, H, W, Fr = a.C, a.H, a.W, a.frames
    A, V = C // 8, C // 2
    q = (O.seeded_randn((Fr, H * W, A), 1) * (1.5 / A ** 0.5)).cuda().requires_grad_()
    k, v = O.seeded_randn((Fr, H * W, A), 2).cuda().requires_grad_(), O.seeded_randn((Fr, H * W, V), 3).cuda().requires_grad_()
    go = O.seeded_randn((Fr, H * W, V), 4).cuda()

    def timed(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / a.iters, 4)

    def fwd():
        with torch.no_grad():
            return npvp_amd.ops.nonlocal_attn_grid(q, k, v, H, W)

    def both():
        q.grad = k.grad = v.grad = None
        npvp_amd.ops.nonlocal_attn_grid(q, k, v, H, W).backward(go)
    general = os.environ.get("NPVP_NL_GRID_GENERAL", "") == "1" or not npvp_amd.ops.nonlocal_attn_config_shape(A, V, H, W)
    out = {"C": C, "H": H, "W": W, "frames": Fr, "kernels": "general" if general else "exact-tile",
           "fwd_ms": timed(fwd), "fwd_bwd_ms": timed(both)}
    if a.check:
        import torch.nn.functional as F
        qd, kd, vd = (t.detach().double().cpu().requires_grad_() for t in (q, k, v))
        pool = lambda t: F.max_pool2d(t.transpose(1, 2).reshape(Fr, t.shape[-1], H, W), 2, 2).flatten(2)
        od = torch.softmax(qd @ pool(kd), dim=-1) @ pool(vd).transpose(1, 2)
        od.backward(go.double().cpu())
        both()
        o = fwd()
        rel = lambda x, y: float((x.double().cpu() - y).norm() / y.norm())
        out["rel_l2"] = {n: float(f"{rel(x, y):.3e}") for n, x, y in (("o", o, od.detach()), ("dq", q.grad, qd.grad), ("dk", k.grad, kd.grad),
                                                                      ("dv", v.grad, vd.grad))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
