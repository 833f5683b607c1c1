"""A fingerprint of the non-local attention entry points (csrc/ae_train.hip): npvp_nonlocal_attn_fwd / _bwd and
npvp_nonlocal_attn_grid_fwd / _bwd through the C ABI only, on seeded inputs, one SHA-256 per case over every output (o, lse, D, dq,
dk, dv).  Two builds of the library that print the same lines compute the same bits: run it before and after a change of these entry
points or their kernels that is meant to move none.  Needs a GPU.

The config entry points run at the four (C, grid) pairs of the AE configs; the any-grid ones at the same four and at every entry of
GRID_SHAPES of tests/test_hip_nl_grid.py (read from that file), two frames each.  As it stands the config shapes run the exact-tile
kernels under both names and the other shapes the general kernels; with NPVP_NL_GRID_GENERAL=1 in the environment the "grid" lines of
the config shapes come from the general kernels instead.

    [NPVP_NL_GRID_GENERAL=1] python tools/nl_bits.py [--lib path/to/libnpvp_hip.so]
"""
import argparse
import ast
import ctypes
import hashlib
import os
import sys

import torch                      # (before the library: both must use the HIP runtime that torch loads)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from npvp_amd import _lib  # noqa: E402  (the argument types of include/npvp_hip.h; the library is the one --lib names)
FRAMES = 2
CONFIG_SHAPES = [(64, 64, 64), (128, 32, 32), (256, 16, 16), (512, 8, 8)]          # (C, H, W)


def grid_shapes():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_hip_nl_grid.py")).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "GRID_SHAPES" for t in node.targets):
            return [tuple(s) for s in ast.literal_eval(node.value)]
    raise SystemExit("GRID_SHAPES not found in tests/test_hip_nl_grid.py")


def load(path):
    return _lib.bind(ctypes.CDLL(path), ("npvp_nonlocal_attn_fwd", "npvp_nonlocal_attn_bwd", "npvp_nonlocal_attn_grid_fwd",
                                         "npvp_nonlocal_attn_grid_bwd", "npvp_last_error"))


def case(L, stem, C, H, W, seed):
    """every output of <stem>_fwd and <stem>_bwd on FRAMES frames of an H x W grid, q | k | v packed in one [F*H*W, 2A+V] tensor"""
    A, V, rows = C // 8, C // 2, FRAMES * H * W
    gen = torch.Generator().manual_seed(seed)
    ld = 2 * A + V
    qkv = torch.randn(rows, ld, generator=gen)
    qkv[:, :A] *= 1.5 / A ** 0.5
    qkv, go = qkv.cuda(), torch.randn(rows, V, generator=gen).cuda()
    new = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device="cuda")       # (an element no kernel writes is hashed as this)
    o, lse, D, dqkv = new(rows, V), new(rows), new(2 * rows), new(rows, ld)
    p, d = qkv.data_ptr(), dqkv.data_ptr()

    def ok(rc):
        assert rc == 0, L.npvp_last_error()

    ok(getattr(L, stem + "_fwd")(p, ld, p + 4 * A, ld, p + 8 * A, ld, o.data_ptr(), V, lse.data_ptr(), FRAMES, H, W, A, V, None))
    ok(getattr(L, stem + "_bwd")(p, ld, p + 4 * A, ld, p + 8 * A, ld, go.data_ptr(), V, lse.data_ptr(), D.data_ptr(),
                                 d, ld, d + 4 * A, ld, d + 8 * A, ld, FRAMES, H, W, A, V, None))
    torch.cuda.synchronize()
    return hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in (o, lse, D, dqkv))).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", default=os.path.join(ROOT, "npvp_amd", "libnpvp_hip.so"))
    L = load(ap.parse_args().lib)
    seed = 31400
    for name, stem, shapes in (("config", "npvp_nonlocal_attn", CONFIG_SHAPES),
                               ("grid  ", "npvp_nonlocal_attn_grid", CONFIG_SHAPES + grid_shapes())):
        for C, H, W in shapes:
            seed += 1
            print(f"{name} C {C} {H}x{W} frames {FRAMES}  {case(L, stem, C, H, W, seed)}")


if __name__ == "__main__":
    main()
