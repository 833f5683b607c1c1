"""Case table and float64 reference of the frozen encoder's opt-in 3 x 3 convolution route (to_device_layout(..., conv3x3="hip"),
csrc/conv3x3.hip), shared by tests/test_frozen_conv3x3_host.py (CPU: the table, the reference against seven wrong restatements, the index
functions and the planner) and tests/test_hip_frozen_conv3x3.py (GPU).

The reference pads explicitly (torch.nn.functional.pad), convolves with F.conv2d in float64, then applies bias, activation and residual:
    y = act(conv2d(pad(x), w) + bias[co]) (+ residual)
Inputs: oracle.ops.seeded_randn; the weights carry the fan-in scale (9 C_in)^-1/2, so the pre-activation has unit spread and bias,
activation and residual all move the result by O(1).  SCALED_CASE has x times 2^12 and w times 2^-10: the amax scaling of both operands
is exercised far from 1."""
import os

import torch
import torch.nn.functional as F

from oracle import ops as O

F16X3_TOL = 1e-5                 # the whole-tensor bar tests/test_hip_ops.py passes to close() for the f16x3 GEMMs; rows: its ROW_TOL
BAR = 1e-4                       # the project's forward bar for the frozen pair (tests/test_hip_golden.py::test_frozen_autoencoder)
ERR_LOG = os.environ.get("NPVP_ERR_LOG")
PAD_MODE = {"zero": 0, "reflect": 1}
ACT = {"none": 0, "relu": 1, "tanh": 2, "sigmoid": 3}

# (C_in, C_out, H, W, frames, pad, act, residual): the smallest shapes that still reach each way to go wrong
KERNEL_CASES = [
    (512, 512, 8, 8, 3, "reflect", "relu", True),        # M = 192: a ragged last tile
    (512, 512, 8, 8, 3, "zero", "relu", True),
    (256, 256, 16, 16, 2, "zero", "relu", True),
    (128, 128, 32, 32, 1, "zero", "none", False),
    (64, 64, 64, 64, 1, "zero", "relu", True),
    (64, 128, 3, 5, 2, "reflect", "tanh", False),        # an odd grid, a tile across the frame border, C_in != C_out
    (128, 128, 2, 2, 5, "reflect", "relu", True),        # reflection at extent 2
    (64, 64, 1, 7, 3, "zero", "none", True),
    (64, 64, 15, 20, 1, "reflect", "relu", True),        # KTH's native grid
]
SCALED_CASE = KERNEL_CASES[2]
X_SCALE, W_SCALE = 2.0 ** 12, 2.0 ** -10

MUTANTS = ("zero_for_reflect", "replicate_for_reflect", "khkw_swapped", "frames_stacked", "no_residual", "act_before_bias", "bias_dropped")
PADDING_MUTANTS = ("zero_for_reflect", "replicate_for_reflect")


def case_id(case):
    Ci, Co, H, W, Fr, pad, act, res = case
    return f"{Ci}to{Co}_{H}x{W}x{Fr}_{pad}_{act}" + ("_res" if res else "")


def rows(case):
    return case[4] * case[2] * case[3]


def inputs(case):
    """x (F, C_in, H, W), w [C_out][C_in][3][3], bias [C_out], res (F, C_out, H, W) or None: fp32, seeded"""
    Ci, Co, H, W, Fr, pad, act, res = case
    s = 900 + 10 * KERNEL_CASES.index(case)
    x = O.seeded_randn((Fr, Ci, H, W), s)
    w = O.seeded_randn((Co, Ci, 3, 3), s + 1) * (9 * Ci) ** -0.5
    if case is SCALED_CASE:
        x, w = x * X_SCALE, w * W_SCALE
    return dict(x=x, w=w, bias=O.seeded_randn((Co,), s + 2), res=O.seeded_randn((Fr, Co, H, W), s + 3) if res else None)


def act64(v, act):
    return (v, v.clamp_min(0), torch.tanh(v), torch.sigmoid(v))[ACT[act]]


def ref64(case, mutant=None, ins=None):
    """the float64 reference (F, C_out, H, W); mutant: one of MUTANTS, a WRONG restatement (the host test shows the bar rejects each)"""
    assert mutant is None or mutant in MUTANTS
    Ci, Co, H, W, Fr, pad, act, res = case
    i = ins if ins is not None else inputs(case)
    x, w, b = i["x"].double(), i["w"].double(), i["bias"].double().view(1, Co, 1, 1)
    mode = {"zero": "constant", "reflect": "reflect"}[pad]
    if pad == "reflect" and mutant == "zero_for_reflect":
        mode = "constant"
    if pad == "reflect" and mutant == "replicate_for_reflect":
        mode = "replicate"
    if mutant == "frames_stacked":                       # one tall image: taps bleed across the frame borders
        x = x.permute(1, 0, 2, 3).reshape(1, Ci, Fr * H, W)
    if mutant == "khkw_swapped":
        w = w.transpose(2, 3)
    y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode=mode), w)
    if mutant == "frames_stacked":
        y = y.reshape(Co, Fr, H, W).permute(1, 0, 2, 3)
    if mutant == "act_before_bias":
        y = act64(y, act) + b
    elif mutant == "bias_dropped":
        y = act64(y, act)
    else:
        y = act64(y + b, act)
    if i["res"] is not None and mutant != "no_residual":
        y = y + i["res"].double()
    return y


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu().flatten(), torch.as_tensor(b).detach().double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def expected_src(extent, pad_mode):
    """[coordinate][tap] -> source coordinate, or -1 for a tap that contributes 0: the indices torch.nn.functional.pad moves"""
    idx = torch.arange(extent, dtype=torch.float64).view(1, 1, extent)
    if pad_mode == 1:
        padded = F.pad(idx, (1, 1), mode="reflect").view(-1)
    else:
        padded = F.pad(idx, (1, 1), mode="constant", value=-1.0).view(-1)
    return [[int(padded[c + tap]) for tap in range(3)] for c in range(extent)]


# ----------------------------------------------------------------------------------------------------------------- the modules
AE_CONFIGS = ("BAIR_VFP_NPVP-D", "Cityscapes_VFP_NPVP-S", "KITTI_VFP_NPVP-D", "KTH_VFP_NPVP-S", "SMMNIST_VFP_NPVP-S")
MODULE_C, MODULE_GRID, MODULE_FRAMES = 512, 8, 2


def block64(blk, x):
    """Factorized3DConvAttn(learn_3d=False).forward of the UNFUSED eval module restated in float64 on a deep copy"""
    import copy
    return copy.deepcopy(blk).double()(x.double(), 1)


def log_line(text):
    print(text)
    if ERR_LOG:
        with open(ERR_LOG, "a") as f:
            f.write(text + "\n")
