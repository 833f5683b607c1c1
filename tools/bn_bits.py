"""A fingerprint of the Stage-1 BatchNorm entry points (csrc/ae_train.hip): the six calls through the C ABI only, on seeded inputs, one
SHA-256 per case over every output (y, mean, rstd, running statistics of the fused and of the synchronised forward; dx, dw, db of
the fused backward; sums, dw, db, dx of the split one).  Two builds of the library that print the same lines compute the same bits:
run it before and after a change of these entry points or their kernels that is meant to move none.  Needs a GPU.

Training mode: the shards of tests/test_hip_ae_dp.py's SHAPES x act 0 / 1 x with / without residual, each shard fed its own sums and
count.  Eval mode (forward from the running statistics, fused backward with train = 0) at (3, 64, 4, 4) in both layouts.

    python tools/bn_bits.py [--lib path/to/libnpvp_hip.so]
"""
import argparse
import ctypes
import hashlib
import os
import sys

import torch                      # (before the library: both must use the HIP runtime that torch loads)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from npvp_amd import _lib  # noqa: E402  (the argument types of include/npvp_hip.h; the library is the one --lib names)
EPS, MOM = 1e-5, 0.1
# (layout, C, H, W, frames of shard a, frames of shard b): SHAPES of tests/test_hip_ae_dp.py
SHAPES = [(0, 4, 2, 2, 1, 2), (0, 64, 3, 3, 2, 3), (0, 32, 12, 12, 2, 3), (0, 512, 8, 8, 1, 2), (1, 64, 3, 4, 2, 3), (1, 512, 8, 8, 1, 2)]
ENTRY_POINTS = ("npvp_bn_workspace_bytes", "npvp_bn_stats", "npvp_bn_act_apply", "npvp_bn_act_bwd", "npvp_bn_act_apply_sync",
                "npvp_bn_bwd_sums", "npvp_bn_act_bwd_apply", "npvp_last_error")


def load(path):
    return _lib.bind(ctypes.CDLL(path), ENTRY_POINTS)


def case(L, layout, C, H, W, n, act, with_res, train, seed):
    """every output of the six calls (training) or of the eval forward and backward on one [n, C, H, W] problem"""
    gen = torch.Generator().manual_seed(seed)
    shape = (n, H, W, C) if layout == 0 else (n, C, H, W)                 # the memory the kernels read: rows or planes
    rnd = lambda *s: torch.randn(*s, generator=gen)
    x, g, res = (rnd(shape) * 1.7 + 0.6).cuda(), rnd(shape).cuda(), rnd(shape).cuda()
    w, b = (1 + 0.1 * rnd(C)).cuda(), (0.1 * rnd(C)).cuda()
    rm0, rv0 = (0.1 * rnd(C)).cuda(), (0.5 + rnd(C).abs()).cuda()
    outer, inner, count = (n * H * W, C, n * H * W) if layout == 0 else (n * C, H * W, n * H * W)
    wsn = L.npvp_bn_workspace_bytes(C)
    ws = torch.empty(wsn // 4, dtype=torch.float32, device="cuda")
    f32 = lambda: torch.empty(C, dtype=torch.float32, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()
    r = p(res) if with_res else None

    def ok(rc):
        assert rc == 0, L.npvp_last_error()

    outs = []
    if train:
        st = torch.empty(2 * C + 1, dtype=torch.float64, device="cuda")
        ok(L.npvp_bn_stats(p(x), outer, inner, C, layout, p(st), p(ws), wsn, None))
        st[2 * C:].fill_(float(count))
        outs.append(st)
    for form in (("fused", "sync") if train else ("fused",)):
        y, mean, rstd, rm, rv = torch.empty_like(x), f32(), f32(), rm0.clone(), rv0.clone()
        if form == "fused":
            ok(L.npvp_bn_act_apply(p(x), p(w), p(b), r, p(st) if train else None, count if train else 0, EPS, MOM, p(rm), p(rv), outer,
                                   inner, C, layout, act, p(y), p(mean), p(rstd), None))
        else:
            ok(L.npvp_bn_act_apply_sync(p(x), p(w), p(b), r, p(st), EPS, MOM, p(rm), p(rv), outer, inner, C, layout, act, p(y), p(mean),
                                        p(rstd), None))
        outs += [y, mean, rstd, rm, rv]
    mean, rstd = outs[-4], outs[-3]
    dx, dw, db = torch.empty_like(x), f32(), f32()
    ok(L.npvp_bn_act_bwd(p(g), p(x), p(mean), p(rstd), p(w), p(b), outer, inner, C, layout, act, int(train), p(dx), p(dw), p(db), p(ws),
                         wsn, None))
    outs += [dx, dw, db]
    if train:
        sums, dx2, dw2, db2 = torch.empty(2 * C, dtype=torch.float64, device="cuda"), torch.empty_like(x), f32(), f32()
        ok(L.npvp_bn_bwd_sums(p(g), p(x), p(mean), p(rstd), p(w), p(b), outer, inner, C, layout, act, p(sums), p(dw2), p(db2), p(ws), wsn,
                              None))
        ok(L.npvp_bn_act_bwd_apply(p(g), p(x), p(mean), p(rstd), p(w), p(b), p(sums), st.data_ptr() + 2 * C * 8, outer, inner, C, layout,
                                   act, p(dx2), None))
        outs += [sums, dw2, db2, dx2]
    torch.cuda.synchronize()
    return hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in outs)).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", default=os.path.join(ROOT, "npvp_amd", "libnpvp_hip.so"))
    L = load(ap.parse_args().lib)
    seed = 20250
    for layout, C, H, W, na, nb in SHAPES:
        for n in (na, nb):
            for act in (0, 1):
                for with_res in (0, 1):
                    seed += 1
                    print(f"train layout {layout} C {C} {H}x{W} n {n} act {act} res {with_res}  {case(L, layout, C, H, W, n, act, with_res, True, seed)}")
    for layout in (0, 1):
        for act in (0, 1):
            seed += 1
            print(f"eval  layout {layout} C 64 4x4 n 3 act {act} res 1  {case(L, layout, 64, 4, 4, 3, act, 1, False, seed)}")


if __name__ == "__main__":
    main()
