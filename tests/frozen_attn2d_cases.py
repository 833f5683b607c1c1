"""Case tables and float64 references of the frozen encoder's opt-in NonLocalAttenion2D route (to_device_layout(..., attn2d="hip")) and of
its epilogue kernel npvp_bias_act_scaled (csrc/ae.hip), shared by tests/test_frozen_attn2d_host.py (CPU: the tables and the reference
are checked there, the reference against seven wrong restatements) and tests/test_hip_frozen_attn2d.py (GPU).

Inputs of the module cases: key_hashed_fill, then gamma planted at -0.75 (the reference initialises it to 0: a zero gamma would hide the
whole branch), every bias of the attention times 10 (0.2 randn: an omitted bias moves the branch by far more than the bar), Wq and Wk
times A^-1/4 (unit-variance frames then give scores of spread about 1: a softmax that is neither uniform nor one-hot, so pooling and
the score scale both show)."""
import copy
import math
import os

import torch
import torch.nn as nn

from oracle import ops as O

BAR = 1e-4                       # the project's forward bar for the frozen pair (tests/test_hip_golden.py::test_frozen_autoencoder)
GAMMA = -0.75
BLOCK_SEED = 720
ERR_LOG = os.environ.get("NPVP_ERR_LOG")

# (C, H, W, frames): the configs' own (C, grid) pairs (exact-tile kernels), and grids only the general kernels take
CONFIG_SHAPES = [(64, 64, 64, 1), (128, 32, 32, 2), (256, 16, 16, 2), (512, 8, 8, 3)]
GRID_SHAPES = [(512, 3, 5, 2), (256, 7, 9, 1), (64, 6, 10, 2), (512, 15, 20, 1)]
MODULE_SHAPES = CONFIG_SHAPES + GRID_SHAPES

MUTANTS = ("no_gamma", "gamma_inside_act", "no_bias", "no_residual", "no_relu", "unpooled", "scaled_scores")

# npvp_bias_act_scaled: (name, layout, outer, inner, C, offset of x in floats).  vector = inner % 4 == 0 and x, out, residual 16-byte
# aligned; min(16384, ceil(work / 256)) blocks of 256 threads, work = n / 4 (vector) or n (scalar)
SMALL_KERNEL_CASES = [
    ("rows_c64_vector", 0, 3, 64, 64, 0),
    ("rows_c6_scalar_by_shape", 0, 5, 6, 6, 0),
    ("rows_c64_scalar_by_alignment", 0, 3, 64, 64, 1),
    ("planes_c3_inner15", 1, 6, 15, 3, 0),
]
GRID_CAP = 16384 * 256           # threads of the capped grid: above this much work the grid-stride loop runs more than once
LOOP_KERNEL_CASES = [
    ("rows_c64_vector_two_strides", 0, 262144 + 3, 64, 64, 0),           # n / 4 = 4194352 > GRID_CAP
    ("rows_c6_scalar_two_strides", 0, 699051 + 4, 6, 6, 0),              # n = 4194330 > GRID_CAP
]
KERNEL_CASES = SMALL_KERNEL_CASES + LOOP_KERNEL_CASES
SCALE = -0.75


def kernel_is_vector(case):
    _, layout, outer, inner, C, off = case
    return inner % 4 == 0 and off % 4 == 0


def kernel_work(case):
    _, layout, outer, inner, C, off = case
    return outer * inner // 4 if kernel_is_vector(case) else outer * inner


def kernel_inputs(case):
    """x [outer][inner], bias [C], residual [outer][inner] (fp32, seeded)"""
    name, layout, outer, inner, C, off = case
    s = 800 + 10 * KERNEL_CASES.index(case)
    return dict(x=O.seeded_randn((outer, inner), s), bias=O.seeded_randn((C,), s + 1), res=O.seeded_randn((outer, inner), s + 2))


def kernel_channel(case):
    """the channel of every element, as the two layouts define it"""
    name, layout, outer, inner, C, off = case
    if layout == 0:
        return torch.arange(inner).expand(outer, inner)
    return (torch.arange(outer) % C).view(outer, 1).expand(outer, inner)


def act64(v, act):
    return (v, v.clamp_min(0), torch.tanh(v), torch.sigmoid(v))[act]


def kernel_ref64(case, act, scale, residual):
    """(ref64, x + b in float64) of out = s * act(x + bias[c]) + residual"""
    i = kernel_inputs(case)
    pre = i["x"].double() + i["bias"].double()[kernel_channel(case)]
    out = (1.0 if scale is None else float(scale)) * act64(pre, act)
    return (out + i["res"].double() if residual else out), pre


def two_rounding_bound(s, pre_act, ref):
    """|got - ref64| <= 2^-23 (|s| |a| + |ref64|): the fp32 sum x + b and the one rounding of the fused multiply-add, each half an ulp,
    with a factor two in hand (a = x + b for act 0 / 1, the act-only fp32 output for tanh / sigmoid)"""
    return 2.0 ** -23 * (abs(float(s)) * pre_act.abs() + ref.abs())


# ----------------------------------------------------------------------------------------------------------------- the module
def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu().flatten(), torch.as_tensor(b).detach().double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def make_block(C, conv_first=True):
    """one eval-mode Factorized3DConvAttn(C, learn_3d=False) with the planted inputs of the module docstring (CPU, fp32)"""
    from npvp_amd.models import Factorized3DConvAttn
    blk = O.key_hashed_fill(Factorized3DConvAttn(C, activ_func=nn.ReLU(True), conv_first=conv_first, learn_3d=False), BLOCK_SEED + C)
    a = blk.attn2d
    with torch.no_grad():
        a.gamma.fill_(GAMMA)
        for lin in (a.Wq, a.Wk, a.Wv, a.out_proj):
            lin.bias.mul_(10.0)
        a.norm_func.bias.mul_(10.0)
        for lin in (a.Wq, a.Wk):
            lin.weight.mul_(a.attn_dim ** -0.25)
    for q in blk.parameters():
        q.requires_grad_(False)
    return blk.eval()


class Holder(nn.Module):
    """the least module tree fuse_frozen_autoencoder walks: an `encoder` with one block, a `decoder` with an empty Sequential"""

    def __init__(self, blk=None):
        super().__init__()
        if blk is not None:
            self.blk = blk
        else:
            self.model = nn.Sequential()
        self.eval()


def module_input(shape):
    C, H, W, Fr = shape
    return O.seeded_randn((Fr, C, H, W), 730 + MODULE_SHAPES.index(shape))


def params64(a):
    """the float64 parameters of an UNFUSED NonLocalAttenion2D (its BatchNorm2d still behind out_proj)"""
    a = copy.deepcopy(a).double()
    bn = a.norm_func
    assert isinstance(bn, nn.BatchNorm2d), "params64 reads the unfused module"
    return dict(Wq=a.Wq.weight, bq=a.Wq.bias, Wk=a.Wk.weight, bk=a.Wk.bias, Wv=a.Wv.weight, bv=a.Wv.bias, Wo=a.out_proj.weight,
                bo=a.out_proj.bias, bn_w=bn.weight, bn_b=bn.bias, bn_mean=bn.running_mean, bn_var=bn.running_var, bn_eps=bn.eps,
                gamma=a.gamma.detach().clone())


def attn2d_ref64(p, x, mutant=None):
    """NonLocalAttenion2D.forward (ref/models/submodules.py:150-176) restated in float64 with eval-mode BatchNorm2d and ReLU:
    x + gamma * relu(bn(out_proj(softmax(q pool(k)^T) pool(v)))), scores unscaled, keys / values max-pooled 2x2 (floor).
    mutant: one of MUTANTS, a WRONG restatement (the host test shows the bar rejects each)."""
    assert mutant is None or mutant in MUTANTS
    x = x.double()
    Fr, C, H, W = x.shape
    A, V = p["Wq"].shape[0], p["Wv"].shape[0]
    tok = x.flatten(2).transpose(1, 2)                                                   # (F, HW, C)
    q = tok @ p["Wq"].T + p["bq"]
    k = (tok @ p["Wk"].T + p["bk"]).transpose(1, 2).reshape(Fr, A, H, W)
    v = (tok @ p["Wv"].T + p["bv"]).transpose(1, 2).reshape(Fr, V, H, W)
    if mutant != "unpooled":
        k, v = nn.functional.max_pool2d(k, (2, 2), stride=2), nn.functional.max_pool2d(v, (2, 2), stride=2)
    k, v = k.flatten(2), v.flatten(2)                                                    # (F, A, HW/4), (F, V, HW/4)
    s = q @ k
    if mutant == "scaled_scores":
        s = s / math.sqrt(A)
    out = torch.softmax(s, dim=-1) @ v.transpose(1, 2) @ p["Wo"].T                       # (F, HW, C)
    if mutant != "no_bias":
        out = out + p["bo"]
    out = out.transpose(1, 2).reshape(Fr, C, H, W)
    cs = lambda t: t.view(1, C, 1, 1)
    out = (out - cs(p["bn_mean"])) / torch.sqrt(cs(p["bn_var"]) + p["bn_eps"]) * cs(p["bn_w"]) + cs(p["bn_b"])
    g = p["gamma"]
    if mutant == "gamma_inside_act":
        return x + torch.relu(g * out)
    h = out if mutant == "no_relu" else torch.relu(out)
    if mutant == "no_gamma":
        return x + h
    if mutant == "no_residual":
        return g * h
    return x + g * h


def log_line(text):
    print(text)
    if ERR_LOG:
        with open(ERR_LOG, "a") as f:
            f.write(text + "\n")
