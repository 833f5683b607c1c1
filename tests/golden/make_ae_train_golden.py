#!/usr/bin/env python3
"""Generate tests/golden/ae_train_{64,128}.npz: two Stage-1 training steps of the REFERENCE's LitAE (ref/models/ResNetAutoEncoder.py:
13-49) on CPU - its shared_step and its configure_optimizers (Adam, betas=(0.5, 0.999)) called as they are - for the KTH pair (1
channel, ngf 64, 3 down-samplings, 2 res blocks; B=2, T=4, 64x64) and the KITTI pair (3 channels, ngf 32, 4, 3; B=1, T=2, 128x128).

Dev-container only, like make_golden.py (same two stubs: timm's to_2tuple, pytorch_lightning.LightningModule = nn.Module, under
which LitAE builds from a plain namespace config).  Only DATA is written: losses, per-parameter gradient norms, the first 64
elements of every gradient and parameter, the BatchNorm running statistics after step 1, LitAE's state-dict keys and parameter
names.  Sizes, seeds and layout: tests/ae_train_cases.py.

    python tests/golden/make_ae_train_golden.py
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import ae_train_cases as AC  # noqa: E402
from make_golden import import_reference  # noqa: E402


def reference_case(tag):
    ref_models = import_reference()[0]
    from models.ResNetAutoEncoder import LitAE
    ci, AE, B, T, S = AC.CASES[tag]
    cfg = SimpleNamespace(Dataset=SimpleNamespace(img_channels=ci), AE=SimpleNamespace(AE_lr=AC.LR, **AE))
    torch.manual_seed(0)
    lit = LitAE(cfg)
    AC.fill(lit)
    lit.train()
    opt = lit.configure_optimizers()

    def step(past, fut):
        opt.zero_grad()
        loss = lit.shared_step((past, fut), 0)
        loss.backward()
        opt.step()
        return loss.detach()
    out = AC.record(lit, step, tag)
    arrays = {k: v.numpy() for k, v in out.items()}
    arrays["param_names"] = AC.param_names(lit)
    arrays["state_keys"] = AC.state_keys(lit)
    return arrays


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for tag in ("64", "128"):
        a = reference_case(tag)
        path = os.path.join(HERE, f"ae_train_{tag}.npz")
        np.savez_compressed(path, **a)
        print(f"wrote {path}: {os.path.getsize(path)} bytes, loss {float(a['loss_0']):.6f} / {float(a['loss_1']):.6f}, "
              f"{len(a['param_names'])} parameters, {len(a['state_keys'])} keys")


if __name__ == "__main__":
    main()
