"""The Stage-1 step cases behind tests/golden/ae_train_{64,128}.npz (written by tests/golden/make_ae_train_golden.py from the
reference's LitAE).  Sizes, seeds and the fixture layout live here so that the generator, the CPU regeneration test and the GPU test
agree on them."""
import numpy as np
import torch

from oracle import ops as O

# tag -> (img channels, AE: section of ref/configs/config_{KTH,KITTI}_Autoencoder.yaml, B, T, S)
CASES = {
    "64": (1, dict(ngf=64, n_downsampling=3, num_res_blocks=2, out_layer='Tanh', learn_3d=False), 2, 4, 64),      # KTH
    "128": (3, dict(ngf=32, n_downsampling=4, num_res_blocks=3, out_layer='Tanh', learn_3d=False), 1, 2, 128),    # KITTI
}
FILL_SEED, FRAME_SEED, LR = 141, 142, 1e-4
HEAD = 64          # first elements stored of every gradient / parameter


def frames(tag, step):
    """(past, future) of step `step` (0, 1): tanh of seeded normals, T/2 + T/2 frames"""
    ci, _, B, T, S = CASES[tag]
    x = torch.tanh(O.seeded_randn((B, T, ci, S, S), FRAME_SEED + 10 * int(tag) + step))
    return x[:, : T // 2].contiguous(), x[:, T // 2:].contiguous()


def fill(pair):
    """key_hashed_fill over LitAE's keys (VPTR_Enc. / VPTR_Dec.): gamma = 0.1 randn, so the attention weights and their BatchNorm
    get gradients (at the reference's initial gamma = 0 they get none)"""
    O.key_hashed_fill(pair, FILL_SEED)


def record(pair, step_fn, tag, dev="cpu"):
    """Two optimisation steps of `pair` (a module whose state_dict keys are LitAE's) through step_fn(past, future) -> loss, which runs
    forward, backward and the optimiser step and leaves the gradients in .grad.  Returns the fixture's arrays."""
    out = {}
    for step in range(2):
        past, fut = (t.to(dev) for t in frames(tag, step))
        loss = step_fn(past, fut)
        out[f"loss_{step}"] = torch.as_tensor(float(loss))
        named = list(pair.named_parameters())
        if step == 0:
            out["grad_norm"] = torch.stack([p.grad.detach().double().norm().float().cpu() for _, p in named])
            out["grad_head"] = torch.stack([_head(p.grad) for _, p in named])
            sd = pair.state_dict()
            out["running"] = torch.cat([sd[k].detach().float().cpu().reshape(-1) for k in sd if k.endswith(("running_mean", "running_var"))])
        out[f"param_head_{step}"] = torch.stack([_head(p.detach()) for _, p in named])
    return out


def _head(t):
    h = t.detach().float().cpu().reshape(-1)[:HEAD]
    return torch.cat([h, h.new_zeros(HEAD - h.numel())])


def param_names(pair):
    return np.array([n for n, _ in pair.named_parameters()])


def state_keys(pair):
    return np.array(list(pair.state_dict()))
