"""The cases of tests/test_hip_hot_kernels.py (GPU) and tests/test_hot_kernel_cases_host.py (CPU): the kernels of the shipped
8 x 8 x 512 point - MlpDWBN's fused middle (csrc/mlpdw.hip), the register-window depthwise convolution, the norms at C = 512 and
P = 64, and attention at P = 64 with wide scores - one entry point at a time against float64.

Same construction as tests/grid_kernel_cases.py, whose BOUND (1e-5 on the whole tensor and on the worst row), ROW_FLOOR, errors,
close and NPVP_ERR_LOG line format are used as they are: a case table per family, inputs from oracle.ops.seeded_randn, and the
reference = the UNCHANGED oracle.ops functions in float64 with autograd, composed where a kernel fuses several of them.
reference(family, case, dtype, mutant) -> {output name: tensor}; MUTANTS are deliberately wrong references, and the host test
requires `worst` to put each at >= 10 x BOUND in some case of its family and the fp32 CPU oracle at <= BOUND / 4 in every case.

A frame MEAN is judged in units of the frame's sigma, |mean - ref| * rstd_ref (SIGMA below names the rstd that scales each mean):
the relative error of a mean near 0 says nothing (the fp32 oracle itself is 3.8e-6 "relative" on the `flat` mean2).

The families mid_bwd and mid_n2 (the fused middle's backward, without and with norm2 inside) have their references, mutants and
route checks here; the C-ABI calls their GPU tests make are data (tests/mid_bwd_calls.py), and the host test holds every operand of
every call to the extent the kernels index before a GPU runs one (an amax slot is 2 KB, whatever a block raises in it).

Input kinds: `plain` and `flat` as in grid_kernel_cases, `shift` at 10 sigma (see `field`); `chan`: per-channel offsets of 5 sigma
(on h1, and on the convolution's bias, so that a thread's first output - the shift of the kernels' one-pass sums - is far from the
frame mean); `lead`: the first four token rows of every frame 10 sigma above the rest (the 2048 elements a one-pass frame
statistic would take its shift from); `wide`: attention scores of sigma 2 with one planted score of 100."""
import functools
import math
import os

import torch

import grid_kernel_cases as G
from grid_kernel_cases import BOUND, ROW_FLOOR, close, errors, rel  # noqa: F401  (re-exported: one bar for both suites)
from oracle import ops as O

H8 = W8 = 8
P64 = 64

# ------------------------------------------------------------------------------------------------------------------- case tables
# fused middle, forward: (frames, Ch, kind).  Ch 512: ONE partial per frame; 1536: an odd count; 2048: the shipped width
MID_FWD = ((1, 512, "plain"), (3, 512, "flat"), (3, 512, "shift"), (3, 1536, "chan"), (1, 2048, "chan"), (3, 2048, "plain"),
           (1, 1536, "shift"))
# fused middle, backward: (frames, Ch, kind).  127 | 128 | 129 frames: one chunk per frame, 128 chunks, 65 chunks of 2 with a last of 1
MID_BWD = ((1, 512, "plain"), (3, 512, "flat"), (127, 512, "plain"), (128, 512, "plain"), (129, 512, "plain"), (3, 1536, "shift"))
# the same with norm2 inside: (frames, Ch, drop_p, nparts2).  nparts2 = Ch / 16 as npvp_frameln_act_bwd_pgrad leaves them (4096
# channels: the 256 a block can merge), or 1: the frame's sums already merged
MID_N2 = ((3, 512, 0.0, 32), (3, 512, 0.3, 32), (2, 512, 0.0, 1), (1, 4096, 0.0, 256), (1, 4096, 0.3, 256))
# depthwise 3x3 at 8 x 8: (frames, Ch, kind)
DW_FWD = ((3, 260, "plain"), (3, 512, "plain"), (2, 1536, "plain"))
DW_STATS = ((3, 1024, "shift"), (2, 3072, "chan"), (1, 1024, "chan"), (2, 3072, "shift"), (1, 1024, "flat"))
DW_WGRAD = ((3, 260, "plain"), (3, 512, "plain"), (3, 1536, "plain"), (255, 260, "plain"), (256, 260, "plain"), (257, 260, "plain"))
# LayerNorm at C = 512 (and the NCHW form's 256): (rows, C, relu, kind)
LAYERNORM = ((3, 512, 0, "plain"), (1001, 512, 1, "plain"), (64, 512, 0, "flat"), (64, 512, 0, "shift"))
LAYERNORM_RES = (5, 512)
# (frames, C, relu, kind): 64 token rows per frame
LAYERNORM_NCHW = ((3, 256, 0, "plain"), (3, 256, 1, "plain"), (3, 512, 0, "flat"), (2, 512, 1, "shift"))
# (N, T, add, gamma, kind) at P = 64, C = 512: N = 3 the fused backward, N = 18 with T = 2 the unfused one
POSFUSE = ((3, 4, 1, 1, "plain"), (3, 2, 0, 1, "flat"), (3, 2, 1, 0, "shift"), (3, 2, 1, 1, "lead"), (18, 2, 1, 1, "plain"),
           (18, 2, 0, 1, "lead"))
LN_POSFUSE = ((3, 2, 1, 1, "plain"), (2, 3, 0, 1, "flat"), (2, 2, 1, 0, "shift"), (2, 2, 1, 1, "lead"))
# linear(frame_stats=True): (rows, N, K) with a +30 bias
LINEAR_STATS = ((3 * 64, 2048, 512), (5 * 64, 512, 2048))
LINEAR_STATS_BIAS = 30.0
# temporal attention at P = 64: (N, Tq, Tk, mask, where the winner is planted: key index).  10: MFMA backward; 18: staged <2,2>;
# 28 x 2: staged <2,1>; 40: generic; 129: streaming, the winner in the first and in the last key tile
ATTN_T = ((1, 10, 10, 0, 3), (1, 10, 10, 1, 3), (1, 18, 18, 0, 17), (1, 18, 18, 1, 5), (1, 28, 2, 0, 1), (1, 40, 40, 0, 33),
          (1, 40, 40, 1, 20), (1, 129, 129, 0, 2), (1, 129, 129, 0, 128), (1, 129, 129, 1, 127))
# spatial attention on the 8 x 8 grid: (frames, window, planted key)
ATTN_S = ((2, 4, 15), (1, 8, 0), (1, 8, 63))
# non-local attention (scores NOT scaled in the model; keys and values 2 x 2 max-pooled): (route, A, frames, H, W, planted key
# window).  The smallest (A, V) = (8, 32) on 4 x 4 (4 keys) and on 18 x 16 (72 keys: a full key tile of 64 and a partial one, the
# winner in the first and in the last) through the any-grid kernels; the config kernels at (64, 256) on 8 x 8
ATTN_NL = (("grid", 8, 2, 4, 4, 0), ("grid", 8, 2, 4, 4, 3), ("grid", 8, 1, 18, 16, 1), ("grid", 8, 1, 18, 16, 71),
           ("config", 64, 2, 8, 8, 15))
NL_Q = 1.5                    # q = randn x 1.5 / sqrt(A), as tests/test_hip_nl_grid.py has it (at 2 the fp32 oracle's dq is at 3.0e-6 for A = 64)
HEADS = 8
# q scale: scores of sigma 2.  At 3 the fp32 oracle's worst row leaves BOUND / 4 in five cases (dk of the masked key: 4.9e-6 at T = 18,
# 8.2e-6 at 40, 6.3e-6 at 129; dq at 28 x 2: 4.6e-6); at 2 its worst is 2.1e-6.  The planted 100 is what reaches for the overflow.
WIDE_Q = 2.0
PLANTED = 100.0

CASES = {"mid_fwd": MID_FWD, "mid_bwd": MID_BWD, "mid_n2": MID_N2, "dw_fwd": DW_FWD, "dw_stats": DW_STATS, "dw_wgrad": DW_WGRAD,
         "layernorm": LAYERNORM, "layernorm_nchw": LAYERNORM_NCHW, "posfuse": POSFUSE, "ln_posfuse": LN_POSFUSE,
         "attn_t": ATTN_T, "attn_s": ATTN_S, "attn_nl": ATTN_NL}
SEED = {"mid_fwd": 2100, "mid_bwd": 2300, "mid_n2": 2500, "dw_fwd": 2700, "dw_stats": 2800, "dw_wgrad": 2900, "layernorm": 3100,
        "layernorm_nchw": 3200, "posfuse": 3300, "ln_posfuse": 3500, "attn_t": 3700, "attn_s": 3900, "attn_nl": 4100, "layernorm_res": 3990,
        "linear_stats": 4000}
# (Bessel's n - 1 moves an rstd by 1 / 2n: 1.5e-5 for a frame of 32 768 values - below 10 x BOUND by construction, so `unbiased` is
# a mutant of the per-token-row LayerNorms (n = 512: 1e-3) only)
NORM_MUTANTS = ("eps0", "tail4")
MUTANTS = {"mid_fwd": ("gelu_tanh", "wrong_nb", "eps0"),
           "mid_bwd": ("gelu_tanh", "gelu_grad_at_a1", "dgrad_unflipped", "wgrad_border_pixel", "gw_tap_major", "last_chunk"),
           "mid_n2": ("mask_not_replayed", "gelu_tanh"),
           "dw_fwd": ("taps_transposed", "dgrad_unflipped"), "dw_stats": ("eps0",), "dw_wgrad": ("wgrad_border_pixel", "last_chunk"),
           "layernorm": ("unbiased", "eps0"), "layernorm_nchw": ("unbiased", "eps0"),
           "posfuse": NORM_MUTANTS, "ln_posfuse": NORM_MUTANTS,
           "attn_t": ("no_max", "mask_ignored", "q_unscaled"), "attn_s": ("no_max", "q_unscaled"),
           "attn_nl": ("no_max", "avg_pool")}
# a mean -> the rstd that turns its error into units of sigma
SIGMA = {"mean1": "rstd1", "mean2": "rstd2", "part2_mean": "rstd2", "merged_mean2": "rstd2", "mean": "rstd",
         "psum": "_psum_unit", "psum2": "_psum2_unit"}
# The frame sums (s1, s2) = (sum g, sum g hhat) of a norm's backward are judged by what their consumer does with them,
# dh = rstd (g - s1 / n - hhat s2 / n): an error of s1 moves every dh by it / n, so it is measured against n x rms(g) (s2: n x
# rms(g hhat)), `_psum_unit` = 1 / that.  Against the sum itself a frame whose terms happen to cancel asks for more than fp32
# addition gives (the fp32 oracle: 3e-6 .. 6e-6 "relative" on three of the five mid_n2 cases); against sqrt(sum g^2) a rounding
# error shared by the frame's terms (the c1, c2 of norm2's backward ahead of it) counts sqrt(n) = 512 times (3e-6 at 4096 channels).
# The dh1 that npvp_frameln_act_bwd_apply makes of the kernel's psum is held to BOUND as a tensor.  A reference's entries that start
# with `_` are such units, not outputs.


def case_id(case):
    return "x".join(str(v) for v in case)


def seed_of(family, case):
    return SEED[family] + 10 * CASES[family].index(case)


# ------------------------------------------------------------------------------------------------------------------- comparison
def sigma_err(a, b, rstd):
    """a mean against its reference in units of sigma; rstd [frames] broadcasts over the partials of a frame"""
    a, b, rstd = (t.detach().double().cpu() for t in (a, b, rstd))
    assert a.shape == b.shape, f"shape {tuple(a.shape)} vs {tuple(b.shape)}"
    d = (a - b).reshape(rstd.numel(), -1) * rstd.reshape(-1, 1)          # (rstd.numel() == a.numel(): a unit per element)
    return float(d.abs().max())


def err_of(name, got, ref):
    """the error of one output as the bound sees it: sigma units for a mean, else the larger of rel-L2 and worst-row rel-L2"""
    if name in SIGMA:
        return sigma_err(got[name], ref[name], ref[SIGMA[name]])
    if not bool(torch.isfinite(got[name].detach().double()).all()):
        return float("inf")
    return max(errors(got[name], ref[name]))


def worst(got, ref):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    return max(err_of(k, got, ref) for k in ref if not k.startswith("_"))


def close_dict(label, got, ref, f32=None, bound=BOUND):
    """every output of `got` against ref (float64); with NPVP_ERR_LOG set, one line per output in grid_kernel_cases.close's format
    (`case what err row_err fp32_cpu_err`; a mean's two error columns both hold its error in sigma units)"""
    failures = []
    for k in got:
        try:
            if k in SIGMA:
                e = sigma_err(got[k], ref[k], ref[SIGMA[k]])
                if os.environ.get("NPVP_ERR_LOG"):
                    fe = "-" if f32 is None else f"{err_of(k, f32, ref):.3e}"
                    with open(os.environ["NPVP_ERR_LOG"], "a") as f:
                        f.write(f"{label} {k}[sigma] {e:.3e} {e:.3e} {fe}\n")
                assert e <= bound, f"{label} {k}: {e:.3e} sigma > {bound:.1e}"
            else:
                close(label, k, got[k], ref[k], bound, None if f32 is None else f32[k])
        except AssertionError as e:              # (every output is measured and logged before the case fails)
            failures.append(str(e))
    assert not failures, "; ".join(failures)


def close_all(family, case, got):
    ref, f32 = ref64(family, case), ref32(family, case)
    close_dict(f"{family}[{case_id(case)}]", got, ref, f32)


# ------------------------------------------------------------------------------------------------------------------- helpers
_leaf, _grads, _stats, _tail4 = G._leaf, G._grads, G._stats, G._tail4


def field(shape, seed, kind, flat_at=0.5):
    """an input kind.  `plain` and `flat` are grid_kernel_cases'; `shift` is 10 + randn here - the 10 sigma of csrc/norm.hip's
    claim; at that file's 30 the fp32 oracle is at 2.7e-6 .. 3.8e-6 on rows of 512, outside the BOUND / 4 it has to hold - and the
    per-token-row norms take `flat` about 0.1 (5 sigma) instead of 0.5 for the same reason (same variance 4e-4)"""
    if kind == "plain":
        return G._field(shape, seed, kind)
    r = O.seeded_randn(shape, seed)
    if kind == "flat":
        return flat_at + 0.02 * r
    if kind == "shift":
        return 10.0 + r
    if kind == "chan":
        return r + 5.0 * O.seeded_randn((shape[-1],), seed + 7)
    if kind == "lead":
        r = r.clone()
        r[:, :4] += 10.0
        return r
    raise ValueError(kind)


def frame_stats64(x, eps=1e-5, mutant=None):
    """[frames, ...] -> (mean [frames], rstd [frames]) over everything but axis 0"""
    mu, rs = _stats(x.reshape(x.shape[0], -1), (1,), eps, mutant)
    return mu.reshape(-1), rs.reshape(-1)


def chan_merge(part, nb, eps=1e-5):
    """frame_stats_merge / frame_stats_finalize_kernel in float64: part [frames, J, 2] of (mean_j, M2_j) over nb values each"""
    part = part.double()
    J = part.shape[1]
    m = part[:, :, 0].mean(1)
    m2 = (part[:, :, 1] + nb * (part[:, :, 0] - m[:, None]) ** 2).sum(1)
    return m, torch.rsqrt(m2 / (nb * J) + eps)


def partials64(x, cols):
    """x [frames, 64, C] -> [frames, C / cols, 2]: (mean, M2) of each block of 64 pixels x `cols` channels"""
    Fr, P, C = x.shape
    b = x.reshape(Fr, P, C // cols, cols).permute(0, 2, 1, 3).reshape(Fr, C // cols, -1)
    mu = b.mean(2)
    return torch.stack([mu, ((b - mu[:, :, None]) ** 2).sum(2)], 2)


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


# ------------------------------------------------------------------------------------------------------------------- fused middle
def mid_inputs(family, case, dtype=torch.float32):
    Fr, Ch, kind = case[0], case[1], (case[2] if family != "mid_n2" else "plain")
    s = seed_of(family, case)
    bias = 0.1 * O.seeded_randn((Ch,), s + 4)
    if kind == "chan":
        bias = bias + 3.0 * O.seeded_randn((Ch,), s + 8)          # (h2 has sigma 0.6: channel means 5 sigma apart)
    if kind == "shift":
        bias = bias + 6.0                                         # (h2 itself 10 sigma off 0)
    return dict(h1=_leaf(field((Fr, P64, Ch), s, kind), dtype), w1n=_leaf(1 + 0.1 * O.seeded_randn((P64, Ch), s + 1), dtype),
                b1n=_leaf(0.1 * O.seeded_randn((P64, Ch), s + 2), dtype), w=_leaf(0.3 * O.seeded_randn((Ch, 3, 3), s + 3), dtype),
                bias=_leaf(bias, dtype), w2n=_leaf(1 + 0.1 * O.seeded_randn((P64, Ch), s + 5), dtype),
                b2n=_leaf(0.1 * O.seeded_randn((P64, Ch), s + 6), dtype), res=O.seeded_randn((Fr, P64, Ch), s + 9).to(dtype),
                cot=O.seeded_randn((Fr, P64, Ch), s + 10).to(dtype),
                prior_dwt=O.seeded_randn((10, Ch), s + 11).to(dtype), prior_gw=O.seeded_randn((Ch, 9), s + 12).to(dtype),
                prior_gb=O.seeded_randn((Ch,), s + 13).to(dtype))


def mid_stats_in(i):
    """norm1's statistics as the kernels are given them: float64, rounded once -> (mean1, rstd1) fp32 [frames]"""
    mu, rs = frame_stats64(i["h1"].detach().double())
    return mu.float(), rs.float()


def mid_part1(i):
    """the row statistics the fc1 GEMM's epilogue leaves (csrc/gemm.h epilogue_rowstats_block): per frame of 64 rows and block of 64
    columns the (mean, M2) of those 4096 values: [frames, Ch / 64, 2] fp32, J1 = Ch / 64, nb1 = 4096"""
    return partials64(i["h1"].detach().double(), 64).float()


def mid_fwd_reference(case, dtype=torch.float64, mutant=None):
    """-> h2, mean1 / rstd1 (the _parts form's outputs), part2_mean / part2_m2 [frames, Ch / 512], mean2 / rstd2, merged_mean2 /
    merged_rstd2 (= the frame's statistics: what the Chan merge of ANY correct partials gives), out, out_res"""
    i = mid_inputs("mid_fwd", case, dtype)
    act = gelu_tanh if mutant == "gelu_tanh" else O.gelu
    nm = mutant if mutant in ("unbiased", "eps0") else None
    h1 = i["h1"].detach()
    mu1, rs1 = frame_stats64(h1, mutant=nm)
    a1 = act(O.frame_ln(h1, i["w1n"].detach(), i["b1n"].detach()) if nm is None else G.frame_ln_mutant(h1, i["w1n"].detach(), i["b1n"].detach(), nm))
    h2 = O.dwconv3x3(a1, i["w"].detach(), i["bias"].detach(), H8, W8)
    mu2, rs2 = frame_stats64(h2, mutant=nm)
    part2 = partials64(h2, 512)
    merged = chan_merge(part2, 4096.0 if mutant == "wrong_nb" else 32768.0) if nm is None else (mu2, rs2)
    ln2 = O.frame_ln(h2, i["w2n"].detach(), i["b2n"].detach()) if nm is None else G.frame_ln_mutant(h2, i["w2n"].detach(), i["b2n"].detach(), nm)
    if mutant == "wrong_nb":
        ln2 = (h2 - merged[0].to(dtype).reshape(-1, 1, 1)) * merged[1].to(dtype).reshape(-1, 1, 1) * i["w2n"].detach() + i["b2n"].detach()
    out = O.gelu(ln2)
    return dict(h2=h2, mean1=mu1, rstd1=rs1, part2_mean=part2[:, :, 0], part2_m2=part2[:, :, 1], mean2=mu2, rstd2=rs2,
                merged_mean2=merged[0].to(dtype), merged_rstd2=merged[1].to(dtype), out=out, out_res=out + i["res"])


def _gelu_grad(y):
    y = y.detach().clone().requires_grad_()
    return torch.autograd.grad(O.gelu(y).sum(), y)[0]


def _mid_chain(i, dh2, mutant, dtype):
    """the float64 autograd of h2 = dwconv(gelu(frame_ln(h1))) + bias under the cotangent dh2 -> da1, dwt_db [10, Ch], psum
    [frames, 2] = (sum g, sum g hhat) with g = dL / d hhat, dh1, dw1n, db1n"""
    Fr, Ch = i["h1"].shape[0], i["h1"].shape[2]
    act = gelu_tanh if mutant == "gelu_tanh" else O.gelu
    # per-frame copies of norm1's affine: their gradients are the per-frame, per-element dL/db = da1 gelu'(y1) and dL/dw = that x hhat
    wf = i["w1n"].detach().expand(Fr, P64, Ch).clone().requires_grad_()
    bf = i["b1n"].detach().expand(Fr, P64, Ch).clone().requires_grad_()
    y1 = O.frame_ln(i["h1"], wf, bf)
    a1 = act(y1)
    h2 = O.dwconv3x3(a1, i["w"], i["bias"], H8, W8)
    g = _grads(h2, dh2, dict(da1=a1, dw=i["w"], db=i["bias"], dh1=i["h1"], dwf=wf, dbf=bf))
    if mutant == "dgrad_unflipped":
        g["da1"] = O.dwconv3x3(dh2, i["w"].detach(), torch.zeros_like(i["bias"]), H8, W8)
    if mutant in ("wgrad_border_pixel", "last_chunk"):
        c2 = dh2.clone()
        if mutant == "wgrad_border_pixel":
            c2[:, P64 - 1] = 0
        else:
            c2[(Fr - 1) // 2 * 2 if Fr >= 128 else Fr - 1:] = 0          # (129 frames in chunks of 2: the last chunk is frame 128)
        g2 = _grads(h2, c2, dict(dw=i["w"], db=i["bias"]))
        g["dw"], g["db"] = g2["dw"], g2["db"]
    if mutant == "gelu_grad_at_a1":
        gm = _grads(y1, g["da1"].detach() * _gelu_grad(a1), dict(dh1=i["h1"], dwf=wf, dbf=bf))
        g.update(gm)
    w1 = i["w1n"].detach()
    psum = torch.stack([(g["dbf"] * w1).sum((1, 2)), (g["dwf"] * w1).sum((1, 2))], 1)
    unit = (torch.stack([(g["dbf"] * w1).pow(2).sum((1, 2)), (g["dwf"] * w1).pow(2).sum((1, 2))], 1) * (P64 * Ch)).rsqrt().detach()
    dwt_db = torch.cat([g["dw"].reshape(Ch, 9).t(), g["db"].reshape(1, Ch)], 0).contiguous()
    return dict(da1=g["da1"].detach(), dwt_db=dwt_db, psum=psum, _psum_unit=unit, dh1=g["dh1"], dw1n=g["dwf"].sum(0), db1n=g["dbf"].sum(0))


def mid_bwd_reference(case, dtype=torch.float64, mutant=None):
    """-> da1, dwt_db (accumulate 0), dwt_db_acc (accumulate 1 onto prior_dwt), gw / gb (reduce_into onto prior_gw [Ch, 9] /
    prior_gb), psum [frames, 2], dh1, dw1n, db1n"""
    i = mid_inputs("mid_bwd", case, dtype)
    o = _mid_chain(i, i["cot"], mutant, dtype)
    Ch = case[1]
    gw = o["dwt_db"][:9].reshape(Ch, 9) if mutant == "gw_tap_major" else o["dwt_db"][:9].t()
    o.update(dwt_db_acc=i["prior_dwt"] + o["dwt_db"], gw=i["prior_gw"] + gw, gb=i["prior_gb"] + o["dwt_db"][9])
    return o


def mid_n2_mask(case):
    """a keep-scale of norm2's dropout [frames, 64, Ch] for the host test (0 or 1 / (1 - p)), drawn once per case"""
    Fr, Ch, p, _ = case
    if p == 0.0:
        return None
    if case not in N2_MASKS:
        N2_MASKS[case] = (torch.rand((Fr, P64, Ch), generator=torch.Generator().manual_seed(seed_of("mid_n2", case))) >= p).double() / (1.0 - p)
    return N2_MASKS[case]


N2_MASKS = {}


def mid_n2_reference(case, dtype=torch.float64, mutant=None, mask=None):
    """da2 = the gradient w.r.t. a2 = drop(gelu(frame_ln(h2))): -> psum2 [frames, 2], dw2n, db2n (npvp_frameln_act_bwd_pgrad), then
    da1, dwt_db, psum, dh1, dw1n, db1n of the chain behind it.  mask: the keep-scale [frames, 64, Ch] the kernels drew (the GPU test
    replays it through npvp_drop_apply); without one, a mask of the host's own"""
    Fr, Ch, p, _ = case
    i = mid_inputs("mid_n2", case, dtype)
    act = gelu_tanh if mutant == "gelu_tanh" else O.gelu
    with torch.no_grad():
        h2 = O.dwconv3x3(O.gelu(O.frame_ln(i["h1"], i["w1n"], i["b1n"])), i["w"], i["bias"], H8, W8)
    h2 = h2.requires_grad_()
    wf = i["w2n"].detach().expand(Fr, P64, Ch).clone().requires_grad_()
    bf = i["b2n"].detach().expand(Fr, P64, Ch).clone().requires_grad_()
    a2 = act(O.frame_ln(h2, wf, bf))
    m = mid_n2_mask(case) if mask is None else mask
    if m is not None and mutant != "mask_not_replayed":
        a2 = a2 * m.to(dtype)
    g = _grads(a2, i["cot"], dict(dh2=h2, dwf=wf, dbf=bf))
    w2 = i["w2n"].detach()
    o = _mid_chain(i, g["dh2"].detach(), None, dtype)
    unit2 = (torch.stack([(g["dbf"] * w2).pow(2).sum((1, 2)), (g["dwf"] * w2).pow(2).sum((1, 2))], 1) * (P64 * Ch)).rsqrt().detach()
    o.update(_psum2_unit=unit2, psum2=torch.stack([(g["dbf"] * w2).sum((1, 2)), (g["dwf"] * w2).sum((1, 2))], 1), dw2n=g["dwf"].sum(0), db2n=g["dbf"].sum(0))
    return o


def mid_n2_stats_in(case):
    """h2 and norm2's statistics as the kernels are given them (float64, rounded once) -> h2, mean2, rstd2 in fp32"""
    i = mid_inputs("mid_n2", case, torch.float64)
    with torch.no_grad():
        h2 = O.dwconv3x3(O.gelu(O.frame_ln(i["h1"], i["w1n"], i["b1n"])), i["w"], i["bias"], H8, W8)
    mu, rs = frame_stats64(h2)
    return h2.float(), mu.float(), rs.float()


# ------------------------------------------------------------------------------------------------------------------- depthwise 8 x 8
def dw_inputs(family, case, dtype=torch.float32):
    Fr, Ch, kind = case
    s = seed_of(family, case)
    bias = 0.1 * O.seeded_randn((Ch,), s + 2) + (5.0 if family == "dw_stats" else 0.0)
    if kind == "chan":
        bias = bias + 5.0 * O.seeded_randn((Ch,), s + 8)
    a = O.seeded_randn((Fr, P64, Ch), s) if kind == "chan" else field((Fr, P64, Ch), s, kind)
    if kind == "flat":          # an output of variance 3e-4 (eps = 1e-5 is 3 % of it) 28 sigma off 0: no + 5 here (280 sigma is conditioning alone)
        a, bias = 0.02 * O.seeded_randn((Fr, P64, Ch), s), 0.5 + 0.002 * O.seeded_randn((Ch,), s + 2)
    return dict(a=_leaf(a, dtype), w=_leaf(0.3 * O.seeded_randn((Ch, 3, 3), s + 1), dtype), b=_leaf(bias, dtype),
                cot=O.seeded_randn((Fr, P64, Ch), s + 3).to(dtype))


def dw_reference(family, case, dtype=torch.float64, mutant=None):
    """dw_fwd -> y, da (flip 1 on the cotangent); dw_stats -> y, mean, rstd; dw_wgrad -> dwt_db [10, Ch]"""
    Fr, Ch, kind = case
    i = dw_inputs(family, case, dtype)
    w = i["w"].transpose(1, 2) if mutant == "taps_transposed" else i["w"]
    y = O.dwconv3x3(i["a"], w, i["b"], H8, W8)
    if family == "dw_stats":
        mu, rs = frame_stats64(y.detach(), mutant=mutant)
        return dict(y=y.detach(), mean=mu, rstd=rs)
    if family == "dw_fwd":
        da = _grads(y, i["cot"], dict(da=i["a"]))["da"]
        if mutant == "dgrad_unflipped":
            da = O.dwconv3x3(i["cot"], i["w"].detach(), torch.zeros_like(i["b"]), H8, W8)
        return dict(y=y.detach(), da=da.detach())
    c2 = i["cot"].clone()
    if mutant == "wgrad_border_pixel":
        c2[:, 0] = 0
    if mutant == "last_chunk":
        c2[Fr - 1:] = 0
    g = _grads(y, c2, dict(dw=i["w"], db=i["b"]))
    return dict(dwt_db=torch.cat([g["dw"].reshape(Ch, 9).t(), g["db"].reshape(1, Ch)], 0).contiguous())


# ------------------------------------------------------------------------------------------------------------------- norms
def layernorm_inputs(case, dtype=torch.float32, seed=None):
    rows, C, relu, kind = case
    s = seed_of("layernorm", case) if seed is None else seed
    return dict(x=_leaf(field((rows, C), s, kind, 0.1), dtype), w=_leaf(1 + 0.1 * O.seeded_randn((C,), s + 1), dtype),
                b=_leaf(0.1 * O.seeded_randn((C,), s + 2), dtype), cot=O.seeded_randn((rows, C), s + 3).to(dtype),
                cot_x=O.seeded_randn((rows, C), s + 4).to(dtype))


def _ln(x, w, b, mutant):
    if mutant is None:
        return O.layernorm(x, w, b)
    mu, rs = _stats(x, (x.dim() - 1,), 1e-5, mutant)
    return (x - mu) * rs * w + b


def layernorm_reference(case, dtype=torch.float64, mutant=None):
    i = layernorm_inputs(case, dtype)
    y = _ln(i["x"], i["w"], i["b"], mutant)
    y = torch.relu(y) if case[2] else y
    out = _grads(y, i["cot"], dict(dx=i["x"], dw=i["w"], db=i["b"]))
    out["y"] = y.detach()
    return out


def layernorm_res_case():
    return (LAYERNORM_RES[0], LAYERNORM_RES[1], 0, "plain")


def layernorm_res_reference(dtype=torch.float64):
    i = layernorm_inputs(layernorm_res_case(), dtype, SEED["layernorm_res"])
    y = O.layernorm(i["x"], i["w"], i["b"])
    gx, gw, gb = torch.autograd.grad((y * i["cot"]).sum() + (i["x"] * i["cot_x"]).sum(), [i["x"], i["w"], i["b"]])
    return dict(x_out=i["x"].detach(), y=y.detach(), dx=gx, dw=gw, db=gb)


def layernorm_nchw_inputs(case, dtype=torch.float32):
    Fr, C, relu, kind = case
    s = seed_of("layernorm_nchw", case)
    return dict(x=_leaf(field((Fr, P64, C), s, kind, 0.1), dtype), w=_leaf(1 + 0.1 * O.seeded_randn((C,), s + 1), dtype),
                b=_leaf(0.1 * O.seeded_randn((C,), s + 2), dtype), cot=O.seeded_randn((1, Fr, C, H8, W8), s + 3).to(dtype))


def layernorm_nchw_reference(case, dtype=torch.float64, mutant=None):
    """LayerNorm(C) (+ ReLU) of [frames, 64, C], written as (1, frames, C, 8, 8): -> y, dx, dw, db"""
    Fr, C, relu, kind = case
    i = layernorm_nchw_inputs(case, dtype)
    y = _ln(i["x"], i["w"], i["b"], mutant)
    y = O.from_canonical(torch.relu(y) if relu else y, 1, Fr, H8, W8)
    out = _grads(y, i["cot"], dict(dx=i["x"], dw=i["w"], db=i["b"]))
    out["y"] = y.detach()
    return out


def posfuse_inputs(family, case, dtype=torch.float32):
    N, T, has_add, has_gamma, kind = case
    C, s = 512, seed_of(family, case)
    sc = 0.02 if kind == "flat" else 1.0
    ln = family == "ln_posfuse"          # (there x goes through LayerNorm(512) first: `flat` about 0.1, and a small affine keeps its output flat)
    return dict(x=_leaf(field((N * T, P64, C), s, kind, 0.1 if ln else 0.5), dtype), add=_leaf(sc * O.seeded_randn((N, P64, C), s + 1), dtype) if has_add else None,
                beta=_leaf(O.seeded_randn((T * P64, C), s + 2), dtype), gamma=_leaf(0.3 * O.seeded_randn((T * P64, C), s + 3), dtype) if has_gamma else None,
                lw=_leaf(sc * (1 + 0.1 * O.seeded_randn((C,), s + 5)), dtype), lb=_leaf(sc * 0.1 * O.seeded_randn((C,), s + 6), dtype),
                cot=O.seeded_randn((N * T, P64, C), s + 4).to(dtype))


def posfuse_reference(case, dtype=torch.float64, mutant=None):
    """posfuse 'layer' at P = 64, C = 512: -> y, dx, dadd, dbeta, dgamma (those that exist)"""
    T = case[1]
    i = posfuse_inputs("posfuse", case, dtype)
    if mutant is None:
        y = O.posfuse(i["x"], T, i["beta"], i["gamma"], i["add"], "layer")
    else:
        y = G.posfuse_restated(i["x"], T, i["beta"], i["gamma"], i["add"], "layer", mutant)
    out = _grads(y, i["cot"], dict(dx=i["x"], dadd=i["add"], dbeta=i["beta"], dgamma=i["gamma"]))
    out["y"] = y.detach()
    return out


def ln_posfuse_reference(case, dtype=torch.float64, mutant=None):
    """LayerNorm(512) then posfuse, forward only: -> y1 = LN(x), ln_mean / ln_rstd [rows], fused, mean / rstd [frames] of the fuse.
    The mutants are those of the SECOND norm (the first is the `layernorm` family's)."""
    N, T = case[0], case[1]
    i = posfuse_inputs("ln_posfuse", case, dtype)
    x = i["x"].detach()
    y1 = O.layernorm(x, i["lw"].detach(), i["lb"].detach())
    add = None if i["add"] is None else i["add"].detach()
    gamma = None if i["gamma"] is None else i["gamma"].detach()
    if mutant is None:
        fused = O.posfuse(y1, T, i["beta"].detach(), gamma, add, "layer")
    else:
        fused = G.posfuse_restated(y1, T, i["beta"].detach(), gamma, add, "layer", mutant)
    u = y1 if add is None else (y1.reshape(N, T, P64, 512) + add.reshape(N, 1, P64, 512)).reshape(N * T, P64, 512)
    mu, rs = frame_stats64(u, mutant=mutant if mutant in ("unbiased", "eps0") else None)
    lmu, lrs = _stats(x.reshape(-1, 512), (1,), 1e-5, None)
    return dict(y1=y1, ln_rstd=lrs.reshape(-1), fused=fused, mean=mu, rstd=rs)


def linear_stats_inputs(case):
    R, N, K = case
    s = SEED["linear_stats"] + 10 * LINEAR_STATS.index(case)
    return dict(x=O.seeded_randn((R, K), s) + 0.5, w=O.seeded_randn((N, K), s + 1) / math.sqrt(K),
                b=O.seeded_randn((N,), s + 2) + LINEAR_STATS_BIAS)


# ------------------------------------------------------------------------------------------------------------------- attention
def _plant(q, k, q_row, k_row, head):
    """make the score of (q_row, k_row) in `head` PLANTED after the d ** -0.5 scaling: both head slices are set along the key's
    direction, the lengths in the 3 : 1 of q and k elsewhere (49 and 16.3: the query's other scores and the key's other scores get
    sigma 6 - with the whole length on one side that row would have sigma 12.5, where the fp32 oracle leaves BOUND / 4)"""
    sl = slice(64 * head, 64 * head + 64)
    u = k[k_row, sl] / k[k_row, sl].norm()
    kn = math.sqrt(PLANTED * 8.0 / WIDE_Q)
    q[q_row, sl], k[k_row, sl] = u * (WIDE_Q * kn), u * kn


def attn_t_inputs(case, dtype=torch.float32):
    """`wide`: q x WIDE_Q; pixel 5, head 2: query 1's score on key `plant` is PLANTED; with the mask, query 0 (which may not see the
    last key) gets a PLANTED score on that last key too - it must not win"""
    N, Tq, Tk, mask, plant = case
    C, s = 64 * HEADS, seed_of("attn_t", case)
    q, k = WIDE_Q * O.seeded_randn((N * Tq * P64, C), s), O.seeded_randn((N * Tk * P64, C), s + 1)
    row = lambda t, p: t * P64 + p
    _plant(q, k, row(1, 5), row(plant, 5), 2)
    if mask:
        _plant(q, k, row(0, 9), row(Tk - 1, 9), 4)
    return dict(q=_leaf(q, dtype), k=_leaf(k, dtype), v=_leaf(O.seeded_randn((N * Tk * P64, C), s + 2), dtype),
                cot=O.seeded_randn((N * Tq * P64, C), s + 3).to(dtype))


def _attn_no_max(q, k, v, q_rows, k_rows, heads, mask):
    """softmax as exp(s) / sum exp(s) without the row maximum taken off, in the dtype of the kernels (fp32): overflows at 100"""
    d = q.shape[-1] // heads
    G_, L = q_rows.shape
    S = k_rows.shape[1]
    f = lambda t, n: t[n.reshape(-1)].reshape(G_, -1, heads, d).permute(0, 2, 1, 3).float()
    s = (f(q, q_rows) * d ** -0.5) @ f(k, k_rows).transpose(-1, -2)
    if mask is not None:
        s = s.masked_fill(mask.view(1, 1, L, S), float("-inf"))
    e = torch.exp(s)
    og = ((e / e.sum(-1, keepdim=True)) @ f(v, k_rows)).permute(0, 2, 1, 3).reshape(G_ * L, -1)
    o = torch.empty(q.shape[0], q.shape[1], dtype=torch.float32)
    o[q_rows.reshape(-1)] = og
    return o.to(q.dtype)


def attn_t_reference(case, dtype=torch.float64, mutant=None):
    N, Tq, Tk, mask, plant = case
    i = attn_t_inputs(case, dtype)
    m = O.encoder_temporal_mask(Tq) if (mask and mutant != "mask_ignored") else None
    q = i["q"] * 8.0 if mutant == "q_unscaled" else i["q"]
    core = _attn_no_max if mutant == "no_max" else O.attn_core
    y = core(q, i["k"], i["v"], O.temporal_groups(N, Tq, P64), O.temporal_groups(N, Tk, P64), HEADS, m)
    out = _grads(y, i["cot"], dict(dq=i["q"], dk=i["k"], dv=i["v"]))
    out["y"] = y.detach()
    return out


def attn_s_inputs(case, dtype=torch.float32):
    """packed q|k on the 8 x 8 grid; window 0 of frame 0, head 3: member 1's score on member `plant` is PLANTED"""
    Fr, ws, plant = case
    R, C, s = Fr * P64, 64 * HEADS, seed_of("attn_s", case)
    q, k = WIDE_Q * O.seeded_randn((R, C), s), O.seeded_randn((R, C), s + 1)
    rows = O.spatial_groups(Fr, H8, W8, ws)[0]
    _plant(q, k, int(rows[1]), int(rows[plant]), 3)
    return dict(qk=_leaf(torch.cat([q, k], 1), dtype), v=_leaf(O.seeded_randn((R, C), s + 2), dtype), cot=O.seeded_randn((R, C), s + 3).to(dtype))


def attn_s_reference(case, dtype=torch.float64, mutant=None):
    Fr, ws, plant = case
    C = 64 * HEADS
    i = attn_s_inputs(case, dtype)
    rows = O.spatial_groups(Fr, H8, W8, ws)
    q = i["qk"][:, :C] * 8.0 if mutant == "q_unscaled" else i["qk"][:, :C]
    core = _attn_no_max if mutant == "no_max" else O.attn_core
    y = core(q, i["qk"][:, C:], i["v"], rows, rows, HEADS, None)
    out = _grads(y, i["cot"], dict(dqk=i["qk"], dv=i["v"]))
    out["y"] = y.detach()
    return out


def attn_nl_inputs(case, dtype=torch.float32):
    """q (scores of sigma ~ 2: NL_Q x the length of a pooled key's direction), k, v [frames, H*W, A | A | 4A]; frame 0: query row 1 and key window `plant` lie along one positive
    direction with lengths 10 x 10 = PLANTED (the window's four cells at 1, 0.9, 0.8, 0.7 of it: no tie, the first is the maximum)"""
    route, A, Fr, H, W, plant = case
    s = seed_of("attn_nl", case)
    q, k = O.seeded_randn((Fr, H * W, A), s) * (NL_Q / A ** 0.5), O.seeded_randn((Fr, H * W, A), s + 1)
    u = O.seeded_randn((A,), s + 4).abs()
    u = u / u.norm() * math.sqrt(PLANTED)
    jh, jw = divmod(plant, W // 2)
    for n, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        k[0, (2 * jh + a) * W + 2 * jw + b] = u * (1.0 - 0.1 * n)
    q[0, 1] = u
    return dict(q=_leaf(q, dtype), k=_leaf(k, dtype), v=_leaf(O.seeded_randn((Fr, H * W, 4 * A), s + 2), dtype),
                cot=O.seeded_randn((Fr, H * W, 4 * A), s + 3).to(dtype))


def attn_nl_reference(case, dtype=torch.float64, mutant=None):
    """NonLocalAttenion2D's core, softmax(q pool(k)^T) pool(v) with nn.MaxPool2d((2, 2), stride=2) (oracle.ops has no such function:
    torch's max_pool2d and softmax in float64, as tests/test_hip_nl_grid.py has it): -> y, dq, dk, dv"""
    import torch.nn.functional as F
    route, A, Fr, H, W, plant = case
    i = attn_nl_inputs(case, dtype)
    pool2 = F.avg_pool2d if mutant == "avg_pool" else F.max_pool2d
    pool = lambda t: pool2(t.transpose(1, 2).reshape(Fr, t.shape[-1], H, W), 2, 2).flatten(2)
    sc = i["q"] @ pool(i["k"])
    if mutant == "no_max":
        e = torch.exp(sc.float())
        att = (e / e.sum(-1, keepdim=True)).to(dtype)
    else:
        att = torch.softmax(sc, dim=-1)
    y = att @ pool(i["v"]).transpose(1, 2)
    out = _grads(y, i["cot"], dict(dq=i["q"], dk=i["k"], dv=i["v"]))
    out["y"] = y.detach()
    return out


# ------------------------------------------------------------------------------------------------------------------- dispatch
def reference(family, case, dtype=torch.float64, mutant=None):
    if family.startswith("dw_"):
        return dw_reference(family, case, dtype, mutant)
    return globals()[family + "_reference"](case, dtype, mutant)


@functools.lru_cache(maxsize=None)
def ref64(family, case):
    """the float64 reference of a case: computed once, shared, never written to"""
    return reference(family, case, torch.float64)


@functools.lru_cache(maxsize=None)
def ref32(family, case):
    """the same oracle in fp32 on the CPU: the reference's own arithmetic noise"""
    return reference(family, case, torch.float32)


# ------------------------------------------------------------------------------------------------------------------- routes
def mid_chunks(L, frames, Ch):
    """(frames per chunk, chunks) of the fused middle's weight-gradient partials [wanted][10][Ch], read off the workspace query"""
    return G.split_chunks(frames, L.npvp_mlpdw_mid_bwd_workspace_bytes(frames, Ch) // (40 * Ch))
