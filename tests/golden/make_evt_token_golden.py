#!/usr/bin/env python3
"""Generate tests/golden/evt_token_encoder.npz, predictor_evt_token_{D,S}.npz and predictor_evt_token_keys.json by importing the
REFERENCE (see make_golden.py, whose import_reference / save this script uses): the encoder with its learned event token
(ref/models/VidHRFormer.py:22-23, 35-42) alone, and the whole predictor with learn_evt_token=True (ref/models/Predictor.py:343-344).

Dev-container only, like make_golden.py: only DATA is written (inputs are re-generated from seeds by tests/evt_token_cases.py).
In the same run the CPU restatement of tests/evt_token_cases.py ("append the token -> tables with a zero frame -> the oracle's
layers on T+1 frames -> shared norm -> split") is compared with the reference in float64 (on float64 modules) and in float32; the
figures are appended to tests/golden/EVT_TOKEN_VS_REFERENCE.txt.

    python tests/golden/make_evt_token_golden.py
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import import_reference, save, rel_err, O  # noqa: E402
from make_window_pad_golden import nrmlp_margin  # noqa: E402
import evt_token_cases as EC  # noqa: E402
import oracle  # noqa: E402

REPORT = []


def npy(t):
    return EC.view(t).detach().cpu().numpy().astype(np.float32)


def note(name, e, bound):
    REPORT.append(f"{name:64s} {e:.3e}")
    print(f"  {name:64s} restatement-vs-reference rel-L2 = {e:.3e}")
    assert e < bound, f"the restatement deviates from the reference on {name}: {e}"


def reference_encoder(RV, RS, dtype):
    """the reference's VidHRFormerEncoder(evt_token=True) on the encoder case, split as ref/models/Predictor.py:344 does"""
    e = EC.ENC
    m = RV.VidHRFormerEncoder(e["layers"], EC.H, EC.W, EC.C, 8, 4, 0.0, 0.0, 4, 1024, nn.LayerNorm(EC.C), True)
    EC.fill(m, e["fill"], e["token"])
    m = m.to(dtype)
    x, beta, gamma, cot_m, cot_e = EC.encoder_inputs("cpu", dtype)
    y = m(x, (beta, gamma), RS.PosFeatFuser(EC.C, 'layer').to(dtype))
    mem, evt = y[:, 0:-1, ...], y[:, -1, ...]
    return EC.encoder_results(mem, evt, x, beta, gamma, m.EVT, dict(m.named_parameters())[EC.ENC_BIAS], cot_m, cot_e)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    R, RV, RS = import_reference()

    # ------------------------------------------------------------------ EVT_Former alone
    for dtype, bound in ((torch.float64, 1e-12), (torch.float32, 1e-5)):
        want = reference_encoder(RV, RS, dtype)
        got = EC.case_encoder_restated(dtype)
        for k in EC.ENC_KEYS:
            note(f"encoder {str(dtype).split('.')[-1]}.{k}", rel_err(got[k], want[k]), bound)
    e = EC.ENC          # (the float32 run of the reference is what is stored)
    assert float(want["g_EVT"].norm()) > 0
    save("evt_token_encoder", meta=np.array([e["N"], e["T"], e["layers"], e["fill"], e["token"], e["x"], e["tables"]]),
         **{k: npy(want[k]) for k in EC.ENC_KEYS})

    # ------------------------------------------------------------------ the whole predictor, D and S
    p = EC.PRED
    kw = dict(norm=nn.LayerNorm(EC.C))
    probe = EC.small_predictor(R, False, 0, "cpu", **kw)
    holder = nn.Module(); holder.nrmlp = probe.nrmlp
    best = (-1.0, 631)
    for seed in range(631, 400631, 1000):          # the ReLU-margin search of make_window_pad_golden.py
        O.key_hashed_fill(holder, seed)
        with torch.no_grad():
            mg = min(nrmlp_margin(probe.nrmlp, probe.observed_coor), nrmlp_margin(probe.nrmlp, probe.predict_coor))
        best = max(best, (mg, seed))
        if mg > 7e-6:
            break
    mg, seed = best
    print(f"  predictor: fill seed {seed}, smallest NRMLP |pre-activation| {mg:.2e}")
    REPORT.append(f"predictor 8x8 SPADE: fill seed {seed}, smallest NRMLP |pre-activation| {mg:.2e}")
    for variant, stochastic in (("D", False), ("S", True)):
        for dtype, bound in ((torch.float64, 1e-12), (torch.float32, 1e-5)):
            ref = EC.small_predictor(R, stochastic, seed, "cpu", **kw).to(dtype)
            plain = EC.small_predictor(R, stochastic, seed, "cpu", learn_evt_token=False, **kw)
            new = sorted(set(ref.state_dict()) - set(plain.state_dict()))
            assert new == ["EVT_Former.EVT"] and len(ref.state_dict()) == len(plain.state_dict()) + 1, new
            mine = EC.restated_predictor(stochastic, seed, dtype)
            assert list(ref.state_dict().keys()) == list(mine.state_dict().keys()), "state-dict keys differ"
            assert [n for n, _ in ref.named_parameters()] == [n for n, _ in mine.named_parameters()], "parameter order differs"
            past, fut, eps, cot = EC.predictor_inputs("cpu", dtype)
            want = EC.run_predictor(ref, stochastic, past, fut, eps, cot, R.Div_KL(1e-2), patch_randn=True)
            got = EC.run_predictor(mine, stochastic, past, fut, eps, cot, oracle.Div_KL(1e-2))
            for k in EC.PRED_KEYS + (EC.PRED_KEYS_S if stochastic else ()):
                note(f"predictor[{variant}] {str(dtype).split('.')[-1]}.{k}", rel_err(got[k], want[k]), bound)
        assert float(want["g_EVT"].norm()) > 0
        save(f"predictor_evt_token_{variant}",
             meta=np.array([p["N"], p["To"], p["Tp"], seed, p["token"], p["past"], p["fut"], p["eps"], p["cot"]]),
             **{k: npy(t) for k, t in want.items()})

    # ------------------------------------------------------------------ the reference module's sorted state-dict keys, config depth
    full, plain = EC.full_predictor(R, True, **kw), EC.full_predictor(R, False, **kw)
    keys = sorted(full.state_dict().keys())
    assert len(keys) == 604 and sorted(set(keys) - set(plain.state_dict())) == ["EVT_Former.EVT"] and len(plain.state_dict()) == 603
    with open(os.path.join(HERE, "predictor_evt_token_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
        f.write("\n")
    print(f"  {len(keys)} state-dict keys with the token")
    with open(os.path.join(HERE, "EVT_TOKEN_VS_REFERENCE.txt"), "a") as f:
        f.write("restatement (tests/evt_token_cases.py) vs the reference, rel-L2 per tensor\n")
        f.write("\n".join(REPORT) + "\n")


if __name__ == "__main__":
    main()
