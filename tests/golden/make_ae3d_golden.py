#!/usr/bin/env python3
"""Fixtures of the learn_3d=True autoencoder from the REFERENCE (ref/models/submodules.py Factorized3DConvAttn / NonLocalAttenion1D,
ref/models/ResNetAutoEncoder.py ResnetEncoder / ResnetDecoder; CPU, fp32), and in the same run the measured agreement of this
package's stock modules and of the float64 restatements of tests/ae3d_cases.py with it (AE3D_VS_REFERENCE.txt).

Development only: needs the reference checkout that make_golden.py imports; nothing in tests/, smoke() or bench.py runs this - they
read the committed files.  Only DATA is written (names, shapes, outputs, gradients, statistics).

    python tests/golden/make_ae3d_golden.py        # rewrites tests/golden/ae3d_*.{json,npz} and AE3D_VS_REFERENCE.txt
"""
import copy
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (puts the repository root on sys.path)
import ae3d_cases as AC  # noqa: E402
from oracle import ops as O  # noqa: E402

BLOCK_SEED, PAIR_SEED = 310, 410
REPORT, ZEROS = [], []


def note(name, mine, ref):
    """rel-L2; a tensor whose exact gradient is 0 (AC.ZERO_GRAD: rounding noise on both sides) is reported by its largest |value|"""
    if name.split(":")[0].endswith(AC.ZERO_GRAD):
        ZEROS.append((name, float(torch.as_tensor(mine).abs().max()), float(torch.as_tensor(ref).abs().max())))
        return 0.0
    e = AC.rel(mine, ref)
    REPORT.append((name, e))
    return e


class Pair(nn.Module):
    """LitAE's two children under LitAE's names"""

    def __init__(self, enc, dec):
        super().__init__()
        self.VPTR_Enc, self.VPTR_Dec = enc, dec


def shapes(module):
    return {k: list(v.shape) for k, v in module.state_dict().items()}


def run_block(block, x, cot, T):
    """-> arrays of one block case: eval output first (state untouched), then one train-mode forward / backward"""
    out = {}
    block.eval()
    with torch.no_grad():
        out["eval"] = block(x, T)
    block.train()
    xi = x.clone().requires_grad_()
    y = block(xi, T)
    names = [n for n, _ in block.named_parameters()]
    gs = torch.autograd.grad((y * cot).sum(), [xi] + [p for _, p in block.named_parameters()])
    out["y"], out["dx"] = y.detach(), gs[0]
    for n, g in zip(names, gs[1:]):
        out["grad." + n] = g
    for k, v in block.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            out["stat." + k] = v.clone()
    return out


def run_pair(enc, dec, frames):
    out = {}
    enc.eval()
    with torch.no_grad():
        out["enc_eval"] = enc(frames)
    enc.train(); dec.train()
    feat = enc(frames)
    rec = dec(feat)
    loss = (rec - frames).abs().mean()
    pair = Pair(enc, dec)
    names = [n for n, _ in pair.named_parameters()]
    gs = torch.autograd.grad(loss, [p for _, p in pair.named_parameters()])
    out["enc"], out["rec"], out["loss"] = feat.detach(), rec.detach(), loss.detach()
    for n, g in zip(names, gs):
        out["grad." + n] = g
    return out


def main():
    ref_models, _, ref_sub = MG.import_reference()
    import models.ResNetAutoEncoder as ref_ae
    import npvp_amd.models.ResNetAutoEncoder as mine

    # ---- keys
    small = dict(ngf=AC.AE_SMALL['ngf'], n_downsampling=AC.AE_SMALL['n_downsampling'], num_res_blocks=AC.AE_SMALL['num_res_blocks'])
    big = dict(ngf=AC.AE64_3D['ngf'], n_downsampling=AC.AE64_3D['n_downsampling'], num_res_blocks=AC.AE64_3D['num_res_blocks'])
    keys = {"small": shapes(ref_ae.ResnetEncoder(1, learn_3d=True, **small)), "ae64": shapes(ref_ae.ResnetEncoder(1, learn_3d=True, **big))}
    with open(os.path.join(HERE, "ae3d_keys.json"), "w") as f:
        json.dump(keys, f, indent=0, sort_keys=False)

    # ---- block
    arrays = {}
    for (N, T, H, W) in AC.BLOCK_CASES:
        for cf in (True, False):
            tag = AC.block_tag(N, T, H, W, cf)
            x, cot = AC.block_input(N, T, H, W)
            rb = O.key_hashed_fill(ref_sub.Factorized3DConvAttn(AC.BLOCK_C, conv_first=cf, learn_3d=True), BLOCK_SEED)
            mb = mine.Factorized3DConvAttn(AC.BLOCK_C, conv_first=cf, learn_3d=True)
            mb.load_state_dict(rb.state_dict(), strict=True)
            p64 = AC.block_params(rb)
            r64, m64 = copy.deepcopy(rb).double(), copy.deepcopy(mb).double()
            gold = run_block(rb, x, cot, T)
            got = run_block(mb, x, cot, T)
            g64r, g64m = run_block(r64, x.double(), cot.double(), T), run_block(m64, x.double(), cot.double(), T)
            for k in gold:
                note(f"block {tag} {k}: stock fp32 vs reference fp32", got[k], gold[k])
                note(f"block {tag} {k}: stock float64 vs reference float64", g64m[k], g64r[k])
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
            for k, v in gold.items():
                arrays[f"{tag}.{k}"] = v.detach().numpy().astype(np.float32)
        # one file per grid: every parameter gradient of four cases does not fit the size limit of a committed file
        arrays["seed"] = np.array(BLOCK_SEED)
        MG.save(AC.block_file(N, T, H, W), **arrays)
        arrays = {}

    # ---- pair
    frames = AC.pair_frames()
    renc = ref_ae.ResnetEncoder(1, learn_3d=True, **small)
    rdec = ref_ae.ResnetDecoder(1, ngf=small['ngf'], n_downsampling=small['n_downsampling'], out_layer='Tanh')
    O.key_hashed_fill(Pair(renc, rdec), PAIR_SEED)
    menc = mine.ResnetEncoder(1, learn_3d=True, **small)
    mdec = mine.ResnetDecoder(1, ngf=small['ngf'], n_downsampling=small['n_downsampling'], out_layer='Tanh')
    menc.load_state_dict(renc.state_dict(), strict=True)
    mdec.load_state_dict(rdec.state_dict(), strict=True)
    r64 = (copy.deepcopy(renc).double(), copy.deepcopy(rdec).double())
    m64 = (copy.deepcopy(menc).double(), copy.deepcopy(mdec).double())
    gold, got = run_pair(renc, rdec, frames), run_pair(menc, mdec, frames)
    g64r, g64m = run_pair(*r64, frames.double()), run_pair(*m64, frames.double())
    for k in gold:
        note(f"pair {k}: stock fp32 vs reference fp32", got[k], gold[k])
        note(f"pair {k}: stock float64 vs reference float64", g64m[k], g64r[k])
    arrays = {k: v.detach().numpy().astype(np.float32) for k, v in gold.items()}
    arrays["seed"] = np.array(PAIR_SEED)
    MG.save("ae3d_pair", **arrays)

    with open(os.path.join(HERE, "AE3D_VS_REFERENCE.txt"), "w") as f:
        f.write("learn_3d=True autoencoder: rel-L2 of this package against the reference modules (CPU), per fixture entry.\n"
                "Written by tests/golden/make_ae3d_golden.py; the bar of tests/test_ae3d_host.py is 1e-5.\n\n")
        for kind in ("stock fp32 vs reference fp32", "stock float64 vs reference float64", "float64 restatement vs reference fp32"):
            rows = [(n, e) for n, e in REPORT if n.endswith(kind)]
            worst = max(rows, key=lambda r: r[1])
            f.write(f"== {kind}: {len(rows)} entries, worst {worst[1]:.3e} ({worst[0].rsplit(':', 1)[0]})\n")
        f.write("\n")
        for n, e in REPORT:
            f.write(f"{n:110s} {e:.3e}\n")
        f.write("\nexact gradient 0 (a constant before a training BatchNorm, or removed by the softmax): max |g| here, in the reference\n")
        for n, a, b in ZEROS:
            f.write(f"{n:110s} {a:.1e} {b:.1e}\n")
    print(open(os.path.join(HERE, "AE3D_VS_REFERENCE.txt")).read()[:900])


if __name__ == "__main__":
    main()
