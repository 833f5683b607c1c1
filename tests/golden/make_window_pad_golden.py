#!/usr/bin/env python3
"""Generate tests/golden/window_pad.npz and tests/golden/predictor_window_pad.npz by importing the REFERENCE (see make_golden.py,
whose import_reference / save this script uses): spatial window attention and the whole predictor on feature grids the
window does not tile, where the reference centre-pads (ref/models/VidHRFormer.py:488-511).

Dev-container only, like make_golden.py: only DATA is written (inputs are re-generated from seeds by tests/window_pad_cases.py).
In the same run the CPU restatement of tests/window_pad_cases.py ("pad with zero rows -> project -> attend over the padded
windows without a key mask -> cut") is compared with the reference in float64 and in float32; the figures are appended to
tests/golden/WINDOW_PAD_VS_REFERENCE.txt.

    python tests/golden/make_window_pad_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import import_reference, save, rel_err, O  # noqa: E402
import window_pad_cases as WC  # noqa: E402


def npy(t):
    return WC.view(t).detach().cpu().numpy().astype(np.float32)


REPORT = []


def note(name, e, bound):
    REPORT.append(f"{name:64s} {e:.3e}")
    print(f"  {name:64s} restatement-vs-reference rel-L2 = {e:.3e}")
    assert e < bound, f"the restatement deviates from the reference on {name}: {e}"


def nrmlp_margin(mod, coor):
    """smallest |pre-activation| of the NRMLP's ReLU layers (make_golden.py: a unit at the kink makes d/dB discontinuous)"""
    x = mod.gaussian_mapping(coor)
    worst = 1e9
    for l in mod.MLP:
        x = l(x)
        if isinstance(l, nn.Linear):
            worst = min(worst, float(x.abs().min()))
    return worst


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    R, RV, RS = import_reference()

    # ------------------------------------------------------------------ the module: reference's own SLMHSA with value= given
    arrays = {}
    for i in range(len(WC.SLMHSA_CASES)):
        case, seed = WC.fixture_case(i)
        Fr, H, W, ws = case
        for dtype, bound in ((torch.float64, 1e-12), (torch.float32, 1e-5)):
            ref = RV.SpatialLocalMultiheadAttention(512, 8, ws, 0.0)
            O.key_hashed_fill(ref, seed)
            ref = ref.to(dtype)
            x, v, cot = WC.slmhsa_inputs(case, seed, "cpu", dtype)
            want = WC.slmhsa_results(ref(x, value=v), x, v, cot, ref.attn.in_proj_weight, ref.attn.in_proj_bias)
            got = WC.case_slmhsa_restated(case, seed, dtype)
            tag = f"slmhsa {Fr}x{H}x{W} ws{ws} {str(dtype).split('.')[-1]}"
            for k in WC.SLMHSA_KEYS:
                note(f"{tag}.{k}", rel_err(got[k], want[k]), bound)
            C = 512
            gb = want["gb"].detach()
            REPORT.append(f"{tag}: |gb_q| {float(gb[:C].norm()):.3e} |gb_k| {float(gb[C:2 * C].norm()):.3e} |gb_v| {float(gb[2 * C:].norm()):.3e}")
        for k in WC.SLMHSA_KEYS:          # (the float32 run of the reference is what is stored)
            arrays[f"c{i}_{k}"] = npy(want[k])
    save("window_pad", meta=np.array([WC.SEED0] + [d for c in WC.SLMHSA_CASES for d in c]), **arrays)

    # ------------------------------------------------------------------ the whole predictor at 6 x 10, window 4
    p = WC.PRED
    kw = dict(norm=nn.LayerNorm(512))
    ref = WC.small_predictor(R, 0, "cpu", **kw)
    holder = nn.Module(); holder.nrmlp = ref.nrmlp
    best = (-1.0, 241)
    for seed in range(241, 400241, 1000):          # the ReLU-margin search of make_golden.py's random-context case
        O.key_hashed_fill(holder, seed)
        with torch.no_grad():
            mg = min(nrmlp_margin(ref.nrmlp, ref.observed_coor), nrmlp_margin(ref.nrmlp, ref.predict_coor))
        best = max(best, (mg, seed))
        if mg > 7e-6:
            break
    mg, seed = best
    print(f"  predictor 6x10: fill seed {seed}, smallest NRMLP |pre-activation| {mg:.2e}")
    REPORT.append(f"predictor {p['H']}x{p['W']} ws4: fill seed {seed}, smallest NRMLP |pre-activation| {mg:.2e}")
    O.key_hashed_fill(ref, seed)
    past, cot = WC.predictor_inputs("cpu")
    res = WC.run_predictor(ref, past, cot)
    save("predictor_window_pad", meta=np.array([p["N"], p["To"], p["Tp"], p["H"], p["W"], seed, p["past"], p["cot"]]),
         **{k: npy(t) for k, t in res.items()})

    with open(os.path.join(HERE, "WINDOW_PAD_VS_REFERENCE.txt"), "a") as f:
        f.write("restatement (tests/window_pad_cases.py) vs the reference, rel-L2 per tensor; bias-gradient norms of the reference\n")
        f.write("\n".join(REPORT) + "\n")


if __name__ == "__main__":
    main()
