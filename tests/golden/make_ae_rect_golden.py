#!/usr/bin/env python3
"""Generate tests/golden/ae_train_rect.npz: two Stage-1 training steps of the REFERENCE's LitAE (ref/models/ResNetAutoEncoder.py:
13-49) on CPU - its shared_step and its configure_optimizers called as they are - for the KITTI pair (3 channels, ngf 32, 4
down-samplings, 3 res blocks) at B=2, T=2 and 48x80 frames: a size no shipped config has, whose attention grids (24x40, 12x20, 6x10,
3x5) are rectangular, not powers of two and, at the last one, odd.

Dev-container only, like make_ae_train_golden.py (same stubs).  Only DATA is written, in that fixture's layout: losses,
per-parameter gradient norms, the first 64 elements of every gradient and parameter, the BatchNorm running statistics after step 1,
LitAE's state-dict keys and parameter names.  Sizes and seeds: tests/ae_rect_cases.py.

    python tests/golden/make_ae_rect_golden.py
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

import ae_rect_cases as RC  # noqa: E402
from make_golden import import_reference  # noqa: E402


def reference_case():
    import_reference()
    from models.ResNetAutoEncoder import LitAE
    cfg = SimpleNamespace(Dataset=SimpleNamespace(img_channels=RC.CI), AE=SimpleNamespace(AE_lr=RC.LR, **RC.AE))
    torch.manual_seed(0)
    lit = LitAE(cfg)
    RC.fill(lit)
    lit.train()
    opt = lit.configure_optimizers()

    def step(past, fut):
        opt.zero_grad()
        loss = lit.shared_step((past, fut), 0)
        loss.backward()
        opt.step()
        return loss.detach()
    arrays = {k: v.numpy() for k, v in RC.record(lit, step).items()}
    arrays["param_names"] = RC.param_names(lit)
    arrays["state_keys"] = RC.state_keys(lit)
    return arrays


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    a = reference_case()
    path = os.path.join(HERE, RC.NAME + ".npz")
    np.savez_compressed(path, **a)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, loss {float(a['loss_0']):.6f} / {float(a['loss_1']):.6f}, "
          f"{len(a['param_names'])} parameters, {len(a['state_keys'])} keys, smallest gradient norm "
          f"{min(float(g) for g, n in zip(a['grad_norm'], a['param_names']) if not str(n).endswith(('spatial_conv.0.bias', 'attn2d.Wk.bias', 'attn2d.Wv.bias', 'attn2d.out_proj.bias'))):.3e}")


if __name__ == "__main__":
    main()
