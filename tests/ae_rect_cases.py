"""The Stage-1 step case behind tests/golden/ae_train_rect.npz (written by tests/golden/make_ae_rect_golden.py from the reference's
LitAE): the KITTI pair at a frame size that is no config's - 48 x 80, so the non-local attentions see 24x40 @ C=64, 12x20 @ 128,
6x10 @ 256 and 3x5 @ 512 (odd: 2 pooled keys).  Sizes, seeds and the fixture layout live here so that the generator, the CPU
regeneration test and the GPU test agree on them; the layout is ae_train_cases.record's."""
import torch

from oracle import ops as O

from ae_train_cases import _head, fill, param_names, state_keys  # noqa: F401  (re-exported: one import for the users of this case)

NAME = "ae_train_rect"
CI = 3
AE = dict(ngf=32, n_downsampling=4, num_res_blocks=3, out_layer='Tanh', learn_3d=False)      # KITTI
# B = 2: every parameter outside the GPU test's ZERO_GRAD list has a gradient norm >= 1.9e-5 in the fixture (at B = 1 one fell to
# ~3e-7, below what a per-tensor norm comparison can resolve)
B, T, H, W = 2, 2, 48, 80
# The frames are chosen by the reference's own conditioning, on the CPU: of the seeds 1540 .. 1551 this one gives the smallest
# worst-case change of a per-parameter gradient norm between the stock modules in float32 and in float64 (8.3e-5; 1542 gave 10.5 %
# on a gamma whose gradient is one cancelling sum - a ReLU on its edge - and six others a parameter with a norm below 1e-5), so
# the per-tensor bounds of the GPU test are not spent on the fixture's own rounding.
FRAME_SEED, LR = 1547, 1e-4


def frames(step):
    """(past, future) of step `step` (0, 1): tanh of seeded normals, T/2 + T/2 frames"""
    x = torch.tanh(O.seeded_randn((B, T, CI, H, W), FRAME_SEED + step))
    return x[:, : T // 2].contiguous(), x[:, T // 2:].contiguous()


def record(pair, step_fn, dev="cpu"):
    """ae_train_cases.record on this case's frames: two optimisation steps of `pair` through step_fn(past, future) -> loss"""
    out = {}
    for step in range(2):
        past, fut = (t.to(dev) for t in frames(step))
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
