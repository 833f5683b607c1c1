"""Case table and float64 reference of the frozen decoder's opt-in 7 x 7 tail route (to_device_layout(..., tail7x7="hip"),
csrc/conv7x7.hip), shared by tests/test_frozen_tail7x7_host.py (CPU: the table, the reference against wrong restatements of the forward
and of the input gradient, the index functions and the planners) and tests/test_hip_frozen_tail7x7.py (GPU).

The reference is the module stack in float64:
    y = act(F.conv2d(F.pad(x, (3, 3, 3, 3), 'reflect'), w) + bias[co])                     (F, C_out, H, W)
Inputs: oracle.ops.seeded_randn; w [C_out][C_in][7][7] carries the fan-in scale (49 C_in)^-1/2, so the pre-activation has unit spread
and bias and activation move the result by O(1).  SCALED_CASE has x times 2^12 and w times 2^-10, as the 3 x 3 tables have."""
import torch
import torch.nn.functional as F

from oracle import ops as O
from frozen_conv3x3_cases import (ACT, AE_CONFIGS, BAR, F16X3_TOL, W_SCALE, X_SCALE, act64, log_line, rel)      # noqa: F401 (shared bars)

# (C_in, C_out, H, W, frames, act): the smallest shapes that still reach each way to go wrong
KERNEL_CASES = [
    (64, 3, 64, 64, 1, "tanh"),                  # the configs' frame: two image rows per tile
    (64, 1, 4, 4, 9, "sigmoid"),                 # the minimum extent: both mirrors reach the same pixels; a tile spans 8 frames, the last is ragged
    (32, 3, 5, 9, 2, "tanh"),                    # C_in = 32, an odd rectangular grid
    (64, 3, 6, 150, 1, "none"),                  # W > 128: column segments with halo windows
    (64, 4, 7, 128, 2, "tanh"),                  # W = 128 exactly, no padded output column
    (64, 3, 8, 16, 2, "none"),                   # the scaled case
]
SCALED_CASE = KERNEL_CASES[5]
PLAN_WIDTHS = (129, 300)                         # further widths of the planner tests (C_in 64, C_out 3, H 5, one frame)

MUTANTS = ("zero_padding", "replicate_padding", "symmetric_padding", "khkw_swapped", "kernel_flipped", "frames_stacked", "bias_dropped",
           "act_before_bias")
GRAD_MUTANTS = ("mirrors_dropped", "replicate_adjoint", "kernel_unflipped", "act_derivative_dropped")
GRAD_BAR = 5e-3                  # the project's bound for gradients through ReLU chains (tests/test_hip_golden.py)


def case_id(case):
    Ci, Co, H, W, Fr, act = case
    return f"{Ci}to{Co}_{H}x{W}x{Fr}_{act}"


def inputs(case):
    """x (F, C_in, H, W), w [C_out][C_in][7][7], bias [C_out], g (F, C_out, H, W): fp32, seeded"""
    Ci, Co, H, W, Fr, act = case
    s = 3100 + 10 * KERNEL_CASES.index(case) if case in KERNEL_CASES else 3190
    x = O.seeded_randn((Fr, Ci, H, W), s)
    w = O.seeded_randn((Co, Ci, 7, 7), s + 1) * (49 * Ci) ** -0.5
    if case is SCALED_CASE:
        x, w = x * X_SCALE, w * W_SCALE
    return dict(x=x, w=w, bias=O.seeded_randn((Co,), s + 2), g=O.seeded_randn((Fr, Co, H, W), s + 3))


def _pad64(x, mode):
    if mode == "zero":
        return F.pad(x, (3, 3, 3, 3))
    if mode == "symmetric":                              # the edge pixel repeated: -1 -> 0, -2 -> 1, -3 -> 2
        x = torch.cat([x[..., :3].flip(-1), x, x[..., -3:].flip(-1)], -1)
        return torch.cat([x[..., :3, :].flip(-2), x, x[..., -3:, :].flip(-2)], -2)
    return F.pad(x, (3, 3, 3, 3), mode)


def pre64(case, ins, x=None, pad="reflect"):
    """the pre-activation in float64 (x: a float64 leaf to differentiate through)"""
    Co = case[1]
    x = ins["x"].double() if x is None else x
    return F.conv2d(_pad64(x, pad), ins["w"].double()) + ins["bias"].double().view(1, Co, 1, 1)


def ref64(case, mutant=None, ins=None):
    """the float64 reference (F, C_out, H, W); mutant: one of MUTANTS, a WRONG restatement (the host test shows the bar rejects each)"""
    assert mutant is None or mutant in MUTANTS
    Ci, Co, H, W, Fr, act = case
    i = ins if ins is not None else inputs(case)
    x, w, b = i["x"].double(), i["w"].double(), i["bias"].double().view(1, Co, 1, 1)
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


def act_grad64(y, act):
    """d act / d pre-activation in float64, through the OUTPUT y"""
    y = y.detach().double().cpu()
    return {"none": torch.ones_like(y), "tanh": 1 - y * y, "sigmoid": y * (1 - y)}[act]


def dgrad64(case, ins=None, y=None, mutant=None):
    """the float64 input gradient (F, C_in, H, W) of sum(g * y) by autograd through pad + conv; y: the output whose activation derivative
    is used (default: the reference's own); mutant: one of GRAD_MUTANTS, a WRONG restatement"""
    assert mutant is None or mutant in GRAD_MUTANTS
    Ci, Co, H, W, Fr, act = case
    i = ins if ins is not None else inputs(case)
    y = ref64(case, ins=i) if y is None else y
    dz = i["g"].double() * (1.0 if mutant == "act_derivative_dropped" else act_grad64(y, act))
    w = i["w"].double()
    if mutant == "mirrors_dropped":                      # the adjoint of zero padding: what reflection folds back is lost
        return F.conv_transpose2d(dz, w, padding=3)
    if mutant == "kernel_unflipped":                     # a correlation of the padded dz with w instead of the transposed convolution
        x = i["x"].double().requires_grad_()
        (dx,) = torch.autograd.grad(F.conv2d(_pad64(x, "reflect"), w.flip(2, 3)), x, dz)
        return dx
    x = i["x"].double().requires_grad_()
    (dx,) = torch.autograd.grad(F.conv2d(_pad64(x, "replicate" if mutant == "replicate_adjoint" else "reflect"), w), x, dz)
    return dx


def expected_src(extent):
    """[coordinate][tap] -> source coordinate: the indices F.pad(..., 'reflect') moves, read off a padded arange"""
    idx = torch.arange(extent, dtype=torch.float64).view(1, 1, extent)
    p = F.pad(idx, (3, 3), "reflect").view(-1).long().tolist()
    return [[p[c + tap] for tap in range(7)] for c in range(extent)]


def expected_adj(extent):
    """[source coordinate][tap] -> the sorted output coordinates whose tap reads it, from autograd of one-hot gradients through the pad"""
    want = [[[] for _ in range(7)] for _ in range(extent)]
    for o in range(extent):
        for tap in range(7):
            x = torch.zeros(1, 1, extent, dtype=torch.float64, requires_grad=True)
            F.pad(x, (3, 3), "reflect")[0, 0, o + tap].backward()
            (s,) = torch.nonzero(x.grad.view(-1)).view(-1).tolist()
            want[s][tap].append(o)
    return want
