#!/usr/bin/env python3
"""Fixture of the learn_3d=True block on a clip of more than 32 frames, from the REFERENCE (ref/models/submodules.py
Factorized3DConvAttn / NonLocalAttenion1D; CPU, fp32): Factorized3DConvAttn(64, learn_3d=True) at (N, T, H, W) = (1, 50, 2, 2), both
orders, seed 310, with the entries of ae3d_block.npz - and in the same run the measured agreement of this package's stock module and
of the float64 restatement of tests/ae3d_cases.py with it (AE3D_LONG_VS_REFERENCE.txt).

Development only: needs the reference checkout that make_golden.py imports; nothing in tests/, smoke() or bench.py runs this - they
read the committed files.  Only DATA is written (outputs, gradients, statistics).

    python tests/golden/make_ae3d_long_golden.py        # rewrites tests/golden/ae3d_long_block_*.npz and AE3D_LONG_VS_REFERENCE.txt
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (puts the repository root on sys.path)
import make_ae3d_golden as M3  # noqa: E402  (run_block, note and its REPORT / ZEROS)
import ae3d_cases as AC  # noqa: E402
import ae3d_long_cases as LC  # noqa: E402
from oracle import ops as O  # noqa: E402


def main():
    _, _, ref_sub = MG.import_reference()
    import npvp_amd.models.ResNetAutoEncoder as mine

    N, T, H, W = LC.LONG_BLOCK
    note = M3.note
    for cf in (True, False):
        tag = LC.long_block_tag(cf)
        x, cot = LC.long_block_input()
        rb = O.key_hashed_fill(ref_sub.Factorized3DConvAttn(AC.BLOCK_C, conv_first=cf, learn_3d=True), LC.BLOCK_SEED)
        mb = mine.Factorized3DConvAttn(AC.BLOCK_C, conv_first=cf, learn_3d=True)
        mb.load_state_dict(rb.state_dict(), strict=True)
        p64 = AC.block_params(rb)
        r64, m64 = copy.deepcopy(rb).double(), copy.deepcopy(mb).double()
        gold = M3.run_block(rb, x, cot, T)
        got = M3.run_block(mb, x, cot, T)
        g64r, g64m = M3.run_block(r64, x.double(), cot.double(), T), M3.run_block(m64, x.double(), cot.double(), T)
        for k in gold:
            note(f"block {tag} {k}: stock fp32 vs reference fp32", got[k], gold[k])
            note(f"block {tag} {k}: stock float64 vs reference float64", g64m[k], g64r[k])
            note(f"block {tag} {k}: reference fp32 vs reference float64", gold[k], g64r[k])
        # the float64 restatement of tests/ae3d_cases.py against the fp32 fixture
        xd = x.double().requires_grad_()
        yd, stats = AC.block_ref(p64, xd, T, cf, True)
        pn = [n for n, _ in rb.named_parameters()]
        gd = torch.autograd.grad((yd * cot.double()).sum(), [xd] + [p64[n] for n in pn])
        note(f"block {tag} y: float64 restatement vs reference fp32", yd, gold["y"])
        note(f"block {tag} dx: float64 restatement vs reference fp32", gd[0], gold["dx"])
        for n, g in zip(pn, gd[1:]):
            note(f"block {tag} grad.{n}: float64 restatement vs reference fp32", g, gold["grad." + n])
        for k, v in stats.items():
            note(f"block {tag} stat.{k}: float64 restatement vs reference fp32", v, gold["stat." + k])
        with torch.no_grad():
            note(f"block {tag} eval: float64 restatement vs reference fp32", AC.block_ref(p64, x.double(), T, cf, False)[0], gold["eval"])
        arrays = {f"{tag}.{k}": v.detach().numpy().astype(np.float32) for k, v in gold.items()}
        arrays["seed"] = np.array(LC.BLOCK_SEED)
        MG.save(LC.long_block_file(cf), **arrays)          # one file per order: both do not fit the size limit of a committed file

    out = os.path.join(HERE, "AE3D_LONG_VS_REFERENCE.txt")
    with open(out, "w") as f:
        f.write(f"learn_3d=True block on a clip of T = {T} frames ((N, T, H, W) = {LC.LONG_BLOCK}): rel-L2 of this package against the\n"
                "reference module (CPU), per fixture entry.  Written by tests/golden/make_ae3d_long_golden.py; the bar of\n"
                "tests/test_ae3d_long_host.py is 1e-5.\n\n")
        for kind in ("stock fp32 vs reference fp32", "stock float64 vs reference float64", "reference fp32 vs reference float64",
                     "float64 restatement vs reference fp32"):
            rows = [(n, e) for n, e in M3.REPORT if n.endswith(kind)]
            worst = max(rows, key=lambda r: r[1])
            f.write(f"== {kind}: {len(rows)} entries, worst {worst[1]:.3e} ({worst[0].rsplit(':', 1)[0]})\n")
        f.write("\n")
        for n, e in M3.REPORT:
            f.write(f"{n:110s} {e:.3e}\n")
        f.write("\nexact gradient 0 (a constant before a training BatchNorm, or removed by the softmax): max |g| here, in the reference\n")
        for n, a, b in M3.ZEROS:
            f.write(f"{n:110s} {a:.1e} {b:.1e}\n")
    print(open(out).read()[:1200])


if __name__ == "__main__":
    main()
