"""Case table and float64 reference of the frozen encoder's opt-in 7 x 7 stem route (to_device_layout(..., stem7x7="hip"),
csrc/conv7x7.hip), shared by tests/test_frozen_stem7x7_host.py (CPU: the table, the reference against wrong restatements, the K index
and the planner) and tests/test_hip_frozen_stem7x7.py (GPU).

The reference is the module stack in float64:
    y = act(F.conv2d(F.pad(x, (3, 3, 3, 3), 'reflect'), w) + bias[co])                     (F, C_out, H, W)
Inputs: oracle.ops.seeded_randn; w [C_out][C_in][7][7] carries the fan-in scale (49 C_in)^-1/2, so the pre-activation has unit spread
and bias and activation move the result by O(1).  SCALED_CASE has x times 2^12 and w times 2^-10, as the sibling tables have."""
import torch
import torch.nn.functional as F

from oracle import ops as O
from frozen_conv3x3_cases import (ACT, AE_CONFIGS, BAR, F16X3_TOL, W_SCALE, X_SCALE, act64, log_line, rel)      # noqa: F401 (shared bars)

# (C_in, C_out, H, W, frames, act): the smallest shapes that still reach each way to go wrong
KERNEL_CASES = [
    (1, 64, 64, 64, 1, "relu"),                  # the KTH / SM-MNIST frame
    (3, 64, 4, 4, 9, "relu"),                    # the minimum extent: both mirrors meet; M = 144: a tile spans 8 frames, the last is ragged; K 147 -> 160
    (3, 32, 5, 9, 3, "relu"),                    # the 32-column variant on an odd rectangular grid, M = 135
    (1, 32, 7, 130, 1, "none"),                  # a tile boundary inside an image row; signed outputs
    (2, 64, 4, 7, 5, "none"),                    # K 98 -> 128
    (4, 128, 8, 8, 2, "relu"),                   # the most K-steps (K 196 -> 224: seven); two column tiles
    (3, 64, 8, 16, 2, "none"),                   # the scaled case
]
SCALED_CASE = KERNEL_CASES[6]
PLAN_WIDTHS = (129, 300)                         # further widths of the planner tests (C_in 3, C_out 64, H 5, one frame)

MUTANTS = ("zero_padding", "replicate_padding", "symmetric_padding", "khkw_swapped", "kernel_flipped", "frames_stacked", "bias_dropped",
           "act_before_bias", "planar_read_as_channels_last")


def case_id(case):
    Ci, Co, H, W, Fr, act = case
    return f"{Ci}to{Co}_{H}x{W}x{Fr}_{act}"


def inputs(case):
    """x (F, C_in, H, W), w [C_out][C_in][7][7], bias [C_out]: fp32, seeded"""
    Ci, Co, H, W, Fr, act = case
    s = 3300 + 10 * KERNEL_CASES.index(case) if case in KERNEL_CASES else 3390
    x = O.seeded_randn((Fr, Ci, H, W), s)
    w = O.seeded_randn((Co, Ci, 7, 7), s + 1) * (49 * Ci) ** -0.5
    if case is SCALED_CASE:
        x, w = x * X_SCALE, w * W_SCALE
    return dict(x=x, w=w, bias=O.seeded_randn((Co,), s + 2))


def _pad64(x, mode):
    if mode == "zero":
        return F.pad(x, (3, 3, 3, 3))
    if mode == "symmetric":                              # the edge pixel repeated: -1 -> 0, -2 -> 1, -3 -> 2
        x = torch.cat([x[..., :3].flip(-1), x, x[..., -3:].flip(-1)], -1)
        return torch.cat([x[..., :3, :].flip(-2), x, x[..., -3:, :].flip(-2)], -2)
    return F.pad(x, (3, 3, 3, 3), mode)


def ref64(case, mutant=None, ins=None):
    """the float64 reference (F, C_out, H, W); mutant: one of MUTANTS, a WRONG restatement (the host test shows the bar rejects each)"""
    assert mutant is None or mutant in MUTANTS
    Ci, Co, H, W, Fr, act = case
    i = ins if ins is not None else inputs(case)
    x, w, b = i["x"].double(), i["w"].double(), i["bias"].double().view(1, Co, 1, 1)
    if mutant == "planar_read_as_channels_last":         # the planar memory [F][C][H][W] taken for [F][H][W][C]
        x = x.contiguous().view(Fr, H, W, Ci).permute(0, 3, 1, 2)
    if mutant == "frames_stacked":                       # one tall image: taps bleed across the frame borders, only the ends reflect
        x = x.permute(1, 0, 2, 3).reshape(1, Ci, Fr * H, W)
    if mutant == "khkw_swapped":
        w = w.transpose(2, 3)
    if mutant == "kernel_flipped":
        w = w.flip(2, 3)
    pad = {"zero_padding": "zero", "replicate_padding": "replicate", "symmetric_padding": "symmetric"}.get(mutant, "reflect")
    y = F.conv2d(_pad64(x, pad), w)
    if mutant == "frames_stacked":
        y = y[0].reshape(Co, Fr, H, W).permute(1, 0, 2, 3)
    if mutant == "act_before_bias":
        return act64(y, act) + b
    if mutant == "bias_dropped":
        return act64(y, act)
    return act64(y + b, act)


def expected_k(C_in):
    """the (kh, kw, ci) of the dense K order, k = (kh * 7 + kw) * C_in + ci, written out as nested loops"""
    return [(kh, kw, ci) for kh in range(7) for kw in range(7) for ci in range(C_in)]
