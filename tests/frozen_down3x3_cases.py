"""Case table and float64 reference of the frozen encoder's opt-in stride-2 3 x 3 convolution route (to_device_layout(...,
down3x3="hip"), the STRIDE = 2 form of csrc/conv3x3.hip), shared by tests/test_frozen_down3x3_host.py (CPU: the table, the reference
against seven wrong restatements, the index function and the planner) and tests/test_hip_frozen_down3x3.py (GPU).

The reference is F.conv2d in float64 with stride 2 and zero padding 1, then bias, activation and residual:
    y = act(conv2d(x, w, stride=2, padding=1) + bias[co]) (+ residual)            (F, C_out, (H + 1) // 2, (W + 1) // 2)
Inputs: oracle.ops.seeded_randn; the weights carry the fan-in scale (9 C_in)^-1/2, so the pre-activation has unit spread and bias,
activation and residual all move the result by O(1).  SCALED_CASE has x times 2^12 and w times 2^-10, as the stride-1 table's has."""
import torch
import torch.nn.functional as F

from oracle import ops as O
from frozen_conv3x3_cases import (ACT, AE_CONFIGS, BAR, F16X3_TOL, W_SCALE, X_SCALE, act64, log_line, rel)      # noqa: F401 (shared bars)

# (C_in, C_out, H, W, frames, act, residual): the smallest shapes that still reach each way to go wrong
KERNEL_CASES = [
    (256, 512, 8, 8, 5, "relu", False),          # M = 80: one ragged tile holding five frames
    (64, 128, 16, 16, 3, "relu", False),         # M = 192: a full and a ragged tile, variant 1
    (32, 64, 12, 10, 2, "relu", False),          # C_in = 32 (one K-step per tap), variant 2, a rectangular grid
    (64, 64, 7, 9, 3, "relu", False),            # odd extents: the last output's tap 2 is outside
    (128, 256, 1, 1, 3, "relu", False),          # extent 1: only the centre tap
    (64, 128, 2, 3, 70, "relu", False),          # 1 x 2 outputs per frame: a tile across 64+ frames
    (256, 512, 30, 40, 1, "none", True),         # KTH's native 120 x 160 chain; no activation, a residual
    (128, 256, 32, 32, 1, "relu", False),        # the scaled case
]
SCALED_CASE = KERNEL_CASES[7]

# ("src_unpadded_near" and "odd_pixels" are two routes to the same wrong tensor - windows starting at 2 o instead of 2 o - 1 - written
# independently: once as a shifted strided convolution, once as the stride-1 result sampled at the odd pixels)
MUTANTS = ("src_unpadded_near", "odd_pixels", "floor_size_padded_back", "khkw_swapped", "frames_stacked", "bias_dropped",
           "act_before_bias")


def out_extent(extent):
    return (extent + 1) // 2


def case_id(case):
    Ci, Co, H, W, Fr, act, res = case
    return f"{Ci}to{Co}_{H}x{W}x{Fr}_{act}" + ("_res" if res else "")


def rows(case):
    return case[4] * out_extent(case[2]) * out_extent(case[3])


def inputs(case):
    """x (F, C_in, H, W), w [C_out][C_in][3][3], bias [C_out], res (F, C_out, Ho, Wo) or None: fp32, seeded"""
    Ci, Co, H, W, Fr, act, res = case
    s = 1900 + 10 * KERNEL_CASES.index(case)
    x = O.seeded_randn((Fr, Ci, H, W), s)
    w = O.seeded_randn((Co, Ci, 3, 3), s + 1) * (9 * Ci) ** -0.5
    if case is SCALED_CASE:
        x, w = x * X_SCALE, w * W_SCALE
    return dict(x=x, w=w, bias=O.seeded_randn((Co,), s + 2),
                res=O.seeded_randn((Fr, Co, out_extent(H), out_extent(W)), s + 3) if res else None)


def ref64(case, mutant=None, ins=None):
    """the float64 reference (F, C_out, Ho, Wo); mutant: one of MUTANTS, a WRONG restatement (the host test shows the bar rejects each)"""
    assert mutant is None or mutant in MUTANTS
    Ci, Co, H, W, Fr, act, res = case
    Ho, Wo = out_extent(H), out_extent(W)
    i = ins if ins is not None else inputs(case)
    x, w, b = i["x"].double(), i["w"].double(), i["bias"].double().view(1, Co, 1, 1)
    if mutant == "frames_stacked":                       # one tall image: taps bleed across the frame borders
        x = x.permute(1, 0, 2, 3).reshape(1, Ci, Fr * H, W)
    if mutant == "khkw_swapped":
        w = w.transpose(2, 3)
    if mutant == "src_unpadded_near":                    # source 2 o + tap: padding on the far side only
        y = F.conv2d(F.pad(x, (0, 2, 0, 2)), w, stride=2)[:, :, :Ho, :Wo]
    elif mutant == "odd_pixels":                         # the stride-1 result sampled at the odd pixels instead of the even ones
        y = F.pad(F.conv2d(x, w, padding=1), (0, 1, 0, 1))[:, :, 1::2, 1::2]
    elif mutant == "floor_size_padded_back":             # floor(extent / 2) outputs computed, the missing last row / column left zero
        y = F.pad(F.conv2d(x, w, stride=2, padding=1)[:, :, :H // 2, :W // 2], (0, Wo - W // 2, 0, Ho - H // 2))
    else:
        y = F.conv2d(x, w, stride=2, padding=1)
    if mutant == "frames_stacked":
        tall = y[0]                                      # (Co, ceil(Fr H / 2), Wo): cut back into Fr frames of Ho rows (zero rows appended
        tall = F.pad(tall, (0, 0, 0, Fr * Ho - tall.shape[1]))          # where an odd H leaves the tall image short of Fr Ho)
        y = tall.reshape(Co, Fr, Ho, Wo).permute(1, 0, 2, 3)
    if mutant == "act_before_bias":
        y = act64(y, act) + b
    elif mutant == "bias_dropped":
        y = act64(y, act)
    else:
        y = act64(y + b, act)
    if i["res"] is not None:
        y = y + i["res"].double()
    return y


def expected_src(extent):
    """[output coordinate][tap] -> source coordinate, or -1 for a tap that contributes 0: the indices F.pad(..., value=-1) plus stride-2
    slicing give"""
    idx = torch.arange(extent, dtype=torch.float64).view(1, 1, extent)
    padded = F.pad(idx, (1, 1), mode="constant", value=-1.0).view(-1)
    windows = padded.unfold(0, 3, 2)                     # window o = padded[2 o : 2 o + 3]
    return [[int(v) for v in win] for win in windows]


# ----------------------------------------------------------------------------------------------------------------- the modules
MODULE_CIN, MODULE_COUT, MODULE_GRID, MODULE_FRAMES = 128, 256, 32, 2          # block2_conv of the ngf = 64 encoders at 64 x 64 frames
