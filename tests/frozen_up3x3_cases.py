"""Case table and float64 reference of the frozen decoder's opt-in transposed 3 x 3 convolution route (to_device_layout(...,
up3x3="hip"), the transposed form of csrc/conv3x3.hip), shared by tests/test_frozen_up3x3_host.py (CPU: the table, the reference
against seven wrong restatements, the index functions and the planner) and tests/test_hip_frozen_up3x3.py (GPU).

The reference is F.conv_transpose2d in float64 with stride 2, padding 1 and output_padding 1, then bias and activation:
    y = act(conv_transpose2d(x, w, None, 2, 1, 1) + bias[co])                     (F, C_out, 2H, 2W)
Inputs: oracle.ops.seeded_randn; w is in the ConvTranspose2d layout [C_in][C_out][3][3] and carries the fan-in scale (9 C_in / 4)^-1/2
(an output pixel sums 9 / 4 taps on average), so the pre-activation has unit spread and bias and activation move the result by O(1).
SCALED_CASE has x times 2^12 and w times 2^-10, as the stride-1 and stride-2 tables have."""
import torch
import torch.nn.functional as F

from oracle import ops as O
from frozen_conv3x3_cases import (ACT, AE_CONFIGS, BAR, F16X3_TOL, W_SCALE, X_SCALE, act64, log_line, rel)      # noqa: F401 (shared bars)

# (C_in, C_out, H, W, frames, act): the smallest shapes that still reach each way to go wrong
KERNEL_CASES = [
    (512, 256, 8, 8, 5, "relu"),                 # 320 rows per class: full and ragged tiles, long K
    (64, 64, 1, 1, 3, "relu"),                   # extent 1: every kernel-index-0 tap is dead; variant 2
    (128, 64, 3, 5, 2, "relu"),                  # an odd rectangular grid
    (256, 128, 2, 3, 70, "relu"),                # a tile across 20+ frames
    (32, 64, 4, 6, 3, "none"),                   # C_in = 32: one K-step per tap (kernel level only: the op needs C_in % 64 for its backward)
    (256, 128, 15, 20, 1, "sigmoid"),            # KTH's native chain, odd H
    (128, 128, 16, 16, 1, "relu"),               # the scaled case
]
SCALED_CASE = KERNEL_CASES[6]
# (case, act) of the op's input-gradient test: the table's shapes and inputs, one of them with the activation taken off (the table's
# own act = none case has C_in = 32, which the op's backward - the stride-2 kernel with out = C_in - does not take)
GRAD_CASES = ((KERNEL_CASES[2], "relu"), (KERNEL_CASES[5], "sigmoid"), (KERNEL_CASES[3], "none"))

MUTANTS = ("parities_swapped", "k02_swapped", "weight_as_cout_cin", "output_padding_zero", "frames_stacked", "bias_dropped",
           "act_before_bias")


def case_id(case):
    Ci, Co, H, W, Fr, act = case
    return f"{Ci}to{Co}_{H}x{W}x{Fr}_{act}"


def rows(case):
    """input-grid rows: the M of one pixel class"""
    return case[4] * case[2] * case[3]


def inputs(case):
    """x (F, C_in, H, W), w [C_in][C_out][3][3], bias [C_out]: fp32, seeded"""
    Ci, Co, H, W, Fr, act = case
    s = 2900 + 10 * KERNEL_CASES.index(case)
    x = O.seeded_randn((Fr, Ci, H, W), s)
    w = O.seeded_randn((Ci, Co, 3, 3), s + 1) * (9 * Ci / 4) ** -0.5
    if case is SCALED_CASE:
        x, w = x * X_SCALE, w * W_SCALE
    return dict(x=x, w=w, bias=O.seeded_randn((Co,), s + 2))


def convt64(x, w):
    return F.conv_transpose2d(x.double(), w.double(), None, 2, 1, 1)


def ref64(case, mutant=None, ins=None):
    """the float64 reference (F, C_out, 2H, 2W); mutant: one of MUTANTS, a WRONG restatement (the host test shows the bar rejects each)"""
    assert mutant is None or mutant in MUTANTS
    Ci, Co, H, W, Fr, act = case
    i = ins if ins is not None else inputs(case)
    x, w, b = i["x"].double(), i["w"].double(), i["bias"].double().view(1, Co, 1, 1)
    if mutant == "frames_stacked":                       # one tall image: taps bleed across the frame borders
        x = x.permute(1, 0, 2, 3).reshape(1, Ci, Fr * H, W)
    if mutant == "k02_swapped":                          # the kernel flipped, as a forward convolution's would be
        w = w.flip(2, 3)
    if mutant == "weight_as_cout_cin":                   # the same memory read in Conv2d's channel order
        w = w.reshape(Co, Ci, 3, 3).transpose(0, 1)
    if mutant == "output_padding_zero":                  # the last output row and column never written
        y = F.pad(F.conv_transpose2d(x, w, None, 2, 1, 0), (0, 1, 0, 1))
    else:
        y = F.conv_transpose2d(x, w, None, 2, 1, 1)
    if mutant == "parities_swapped":                     # class (a, b) stored where class (1 - a, 1 - b) belongs
        z = torch.empty_like(y)
        for a in (0, 1):
            for bb in (0, 1):
                z[:, :, a::2, bb::2] = y[:, :, 1 - a::2, 1 - bb::2]
        y = z
    if mutant == "frames_stacked":
        y = y[0].reshape(Co, Fr, 2 * H, 2 * W).permute(1, 0, 2, 3)
    if mutant == "act_before_bias":
        return act64(y, act) + b
    if mutant == "bias_dropped":
        return act64(y, act)
    return act64(y + b, act)


def expected_taps(extent):
    """[output coordinate] -> the set of (kernel index, source coordinate) pairs that reach it, read off one-hot conv_transpose1d calls
    (stride 2, padding 1, output_padding 1): the index map F.conv_transpose2d applies per axis"""
    want = [set() for _ in range(2 * extent)]
    for s in range(extent):
        for k in range(3):
            x = torch.zeros(1, 1, extent, dtype=torch.float64); x[0, 0, s] = 1.0
            w = torch.zeros(1, 1, 3, dtype=torch.float64); w[0, 0, k] = 1.0
            y = F.conv_transpose1d(x, w, None, 2, 1, 1).view(-1)
            assert y.numel() == 2 * extent and float(y.sum()) in (0.0, 1.0)
            for o in torch.nonzero(y).view(-1).tolist():
                want[o].add((k, s))
    return want


# ----------------------------------------------------------------------------------------------------------------- the modules
MODULE_CIN, MODULE_COUT, MODULE_GRID, MODULE_FRAMES = 256, 128, 16, 2          # the second upsampling of the ngf = 64 decoders at 64 x 64 frames
GRAD_BAR = 5e-3                  # the project's bound for gradients through ReLU chains (tests/test_hip_golden.py)
