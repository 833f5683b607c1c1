"""What the learned event token costs (ref/models/VidHRFormer.py:35-42): the NPVP-S training step (4 + 8 layers, 8 x 8 grid, window 4)
at BAIR's clip (To 2, Tp 28) and KTH's (To 10, Tp 20), batch 8, with learn_evt_token=True beside the same step without it.  Needs an
MI355X.  JSON lines, then one summary line per dataset.

The two models of a dataset alternate A, B, A, B ... in one process (--rounds rounds of --steps eager steps each, timed between device
events after warm-up steps); the figure reported is the MEDIAN of a model's rounds.  Expectation: the two encoder passes run on T + 1
instead of T frames (context: (To + 1) / To, target: (Tp + 1) / Tp of their token rows), the decoder is unchanged.

Usage: python tools/evt_token_bench.py [--batch 8 --steps 10 --rounds 5 --datasets BAIR KTH]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                      # noqa: E402

CLIPS = {"BAIR": (2, 28), "KTH": (10, 20)}


def timed(fn, iters, warm):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters          # ms


def build(npvp_amd, O, B, To, Tp, token):
    h = torch.linspace(0, 7, 8)
    to, tp = torch.linspace(0, To - 1, To), torch.linspace(To, To + Tp - 1, Tp)
    m = npvp_amd.Predictor(8, 8, To + Tp, h, h, to, tp, 512, 'Add', 'layer', 256, 1, True, 8, window_size=4, evt_former=True,
                           learn_evt_token=token, evt_former_num_layers=4)
    O.key_hashed_fill(m, 7)
    m = m.cuda().train()
    opt = npvp_amd.FlatAdamW(m, lr=1e-4, clip_module=m.transformer, max_grad_norm=1.0)
    past, fut = O.synth_features((B, To, 512, 8, 8), 1).cuda(), O.synth_features((B, Tp, 512, 8, 8), 2).cuda()
    return lambda: npvp_amd.predictor_train_step(m, opt, past, fut, 0.01, 1e-8, 1.0, sync=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--datasets", nargs="+", default=list(CLIPS), choices=list(CLIPS))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evt_token_bench needs an MI355X")
    import npvp_amd
    from oracle import ops as O
    L = npvp_amd._lib.lib()
    for name in a.datasets:
        To, Tp = CLIPS[name]
        runs = {token: build(npvp_amd, O, a.batch, To, Tp, token) for token in (False, True)}
        ms, launches = {False: [], True: []}, {}
        for r in range(a.rounds):
            for token, fn in runs.items():
                t = timed(fn, a.steps, warm=3 if r == 0 else 1)
                c0 = L.npvp_launch_count()
                fn()
                torch.cuda.synchronize()
                launches[token] = L.npvp_launch_count() - c0
                ms[token].append(t)
                print(json.dumps({"dataset": name, "round": r, "learn_evt_token": token, "step_ms": round(t, 3),
                                  "launches_per_step": launches[token]}), flush=True)
        med = {k: statistics.median(v) for k, v in ms.items()}
        enc_rows = lambda extra: a.batch * 64 * ((To + extra) + (Tp + extra))
        print(json.dumps({"dataset": name, "To": To, "Tp": Tp, "batch": a.batch, "rounds": a.rounds, "steps_per_round": a.steps,
                          "median_step_ms_without": round(med[False], 3), "median_step_ms_with": round(med[True], 3),
                          "ratio": round(med[True] / med[False], 4), "spread_without": [round(min(ms[False]), 3), round(max(ms[False]), 3)],
                          "spread_with": [round(min(ms[True]), 3), round(max(ms[True]), 3)],
                          "encoder_token_rows_ratio": round(enc_rows(1) / enc_rows(0), 4), "launches_without": launches[False],
                          "launches_with": launches[True]}), flush=True)
        del runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
