"""The cases of tests/test_hip_helper_kernels.py (GPU) and tests/test_helper_kernel_cases_host.py (CPU): the small HBM-bound kernels
that close every training step and open every evaluation step - csrc/elementwise.hip (drop_apply, transpose, reduce / broadcast over
a middle axis, colsum, the depthwise table, gradient-norm clip, AdamW, the scalar losses), csrc/ae.hip (bias_act, act_bwd),
csrc/metrics.hip (sqdiff, SSIM) and csrc/data.hip (u8 -> fp32) - at the smallest shapes that reach each branch of their launchers.

Per family: a case table (every predicate read off the launcher, noted beside the table), an input builder (oracle.ops.seeded_randn,
one seed per (family, case): fp32 values; scalars that travel as `float` arguments are rounded to fp32 first), and
reference(family, case, dtype, mutant) -> {output name: tensor}: the operation in `dtype` arithmetic from those fp32 values -
float64 is the reference, float32 (torch's CPU ops in the formula's order) measures the arithmetic noise the bars must stay clear of.

KINDS says how each output is held (measure()):
  tensor  whole-tensor rel-L2 and worst-row rel-L2 (grid_kernel_cases.errors) within BOUND = 1e-5, that module's bar;
  elem    the same, and the LARGEST elementwise error |a - b| / max(|b|, floor) within BOUND: one wrong element out of thousands
          disappears in a rel-L2.  floor (floors()) is per element the sum of the absolute terms the element was rounded from: an
          element that cancels below it carries the rounding error of those terms, in any fp32 arithmetic;
  scalar  |a - b| relative to the sum of the absolute terms within SCALAR_BOUND = 1e-6, the bar of test_scalar_losses_against_the_
          oracle (a sum_all near zero is not judged against its own cancellation);
  bits    where the kernel's arithmetic is ONE fp32 operation per element (or a copy) the reference restates it in fp32 whatever
          `dtype` is, and the output must be equal to the bit.

MUTANTS are deliberately wrong references.  The host test requires `worst_ratio` (error / bar, the GPU test's comparison) to put each
at >= 10 in some case of its family, and the fp32 restatement at <= 1 / 4 in every case.  Neither bar is fitted to a kernel."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from grid_kernel_cases import BOUND, ROW_FLOOR, case_id, errors, rel  # noqa: F401  (rel, max_row_rel_err through errors)
from oracle import metrics as OM
from oracle import ops as O

SCALAR_BOUND = 1e-6
INF = float("inf")


def f32(x):
    """a Python float as the fp32 value a `float` argument of the C ABI carries"""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------------------- case tables
# npvp_adamw_step: grid = min(4096, ceil(ceil(n / 4) / 256)) blocks of 256 lanes, one float4 per lane and trip -> 4 194 304 elements
# per sweep; lanes c0..c3 test i + k against [clip_begin, clip_end); elements [n & ~3, n) by thread 0 of block 0.
# (n, clip range or None, write_back_grad, weight_decay, eps, calls).  n = 43: vector part [0, 40), tail [40, 43).
ADAMW_SWEEP = 4096 * 256 * 4
ADAMW = ((43, None, 1, 0.01, 1e-8, 1), (43, (0, 43), 1, 0.01, 1e-8, 1), (43, (5, 18), 0, 0.0, 1e-8, 1), (43, (5, 18), 1, 0.3, 1e-8, 1),
         (43, (6, 23), 1, 0.01, 1e-3, 1), (43, (7, 41), 1, 0.01, 1e-8, 2), (43, (7, 41), 0, 0.3, 1e-8, 1), (43, (40, 43), 1, 0.3, 1e-8, 1),
         (43, (3, 4), 1, 0.0, 1e-8, 1), (3, (1, 3), 1, 0.01, 1e-8, 1), (3, None, 0, 0.01, 1e-8, 1),
         (4200003, (1000001, 4200002), 1, 0.01, 1e-8, 1))
ADAMW_HYPER = ((1e-2, 3.0), (5e-3, 4.0))       # {lr, step} in device memory: the first call's, the second call's
ADAMW_BETAS = (0.9, 0.999)
ADAMW_COEF = 0.3
# npvp_grad_norm_clip: min(1024, ceil((n / 4) / 256)) blocks -> 1 048 576 elements per sweep, the tail by thread 0 of block 0.
# (n, kind): 'above' norm 5 against max_norm 1; 'below' norm 0.1 (coefficient exactly 1); 'zero'; 'small' norm 0.02 against
# max_norm 1e-3 - the only one in which the 1e-6 of the denominator is 5e-5 of it
LOSS_SWEEP = 1024 * 256 * 4
CLIP = tuple((n, k) for n in (3, 1001, 1050003) for k in ("above", "below", "zero")) + ((1001, "small"),)
CLIP_SCALE = {"above": (5.0, 1.0), "below": (0.1, 1.0), "zero": (0.0, 1.0), "small": (0.02, 1e-3)}      # (norm wanted, max_norm)
# npvp_l1_mean / npvp_sum_all: the same grid (loss_blocks); npvp_l1_mean_bwd: min(4096, .) blocks -> 4 194 304 per sweep.
# (n,): ties a == b on every 7th element
L1 = ((1,), (3,), (1001,), (1002,), (1003,), (1004,), (1050003,), (4200003,))
SUM = ((1,), (3,), (1001,), (1002,), (1003,), (1004,), (1050003,))
L1_LAM, L1_GOUT = 0.01, 3.0
# npvp_reduce_mid: min(4096, ceil(A Cc / 4 / 256)) blocks; npvp_broadcast_mid the same over A B Cc / 4.  (A, B, Cc, accumulate)
EW_SWEEP4 = 4096 * 256                           # float4s per sweep of an ew_blocks grid
MID = tuple((a, b, c, acc) for (a, b, c) in ((1, 1, 4), (3, 5, 1028), (3, 2, 1400004)) for acc in (0, 1))
MID_SCALE = 0.3
# npvp_transpose: 32 x 32 tiles, grid (ceil(C / 32), ceil(R / 32), batch).  (batch, R, C)
TRANSPOSE = ((1, 1, 1), (3, 37, 5), (2, 33, 64), (1, 9, 2048), (2, 64, 31))
# npvp_colsum: wanted = min(rows, 128) chunks, split_chunks (csrc/partials.h) -> rows per chunk and chunks used; the query reserves
# `wanted` partial rows.  (rows, N, ld, accumulate)
COLSUM = tuple((r, n, ld, acc) for (r, n, ld) in ((1, 4, 4), (100, 260, 272), (130, 1028, 1028), (1001, 512, 1024)) for acc in (0, 1))
# npvp_dwtb_build / npvp_dwtb_accumulate: ceil(10 C / 256) blocks of 256, one element each.  (C, has_b)
DWTB = tuple((c, hb) for c in (1, 20, 260) for hb in (1, 0))
# npvp_drop_apply: min(4096, ceil(rows (ncols / 4) / 256)) blocks.  (rows, ncols, p, mode, g1, g2); mode 1 keys (row / g1) % g2
DROP = tuple((r, nc, p, m, g1, g2) for (r, nc) in ((3, 4), (1030, 4100)) for p in (0.1, 0.5) for (m, g1, g2) in ((0, 1, 1), (1, 2, 103)))
DROP_SEED, DROP_SALT = 0x1E3779B97F4A7C15, 77
# npvp_bias_act: vec = inner % 4 == 0 and x, out, residual 16-byte aligned; min(16384, ceil(work / 256)) blocks with work = n / 4
# float4s (vec) or n elements -> 16 777 216 / 4 194 304 elements per sweep.  (layout, outer, inner, C, act, residual, misaligned)
AE_CAP = 16384 * 256
_BA_SHAPES = ((0, 5, 8, 8, 0), (0, 7, 6, 6, 0), (1, 6, 9, 3, 0), (1, 6, 16, 3, 0), (1, 6, 16, 3, 1))
BIAS_ACT = tuple((lay, o, i, c, act, r, mis) for (lay, o, i, c, mis) in _BA_SHAPES for act in range(4) for r in (0, 1)) + (
    (0, 1398187, 12, 12, 1, 1, 0),              # 16 777 216 + 1028 elements, vector
    (1, 23173, 181, 3, 1, 0, 0))                # 4 194 304 + 9 elements, scalar (inner % 4 == 1)
# npvp_act_bwd: min(16384, ceil(n / 256)) blocks, one element per lane and trip.  (n, act)
ACT_BWD = tuple((n, act) for n in (1, 1003) for act in range(4)) + ((AE_CAP + 9, 1), (AE_CAP + 9, 3))
# npvp_sqdiff_per_image: chunks = clamp(ceil(per / 16384), 1, 256) blocks per image, chunk = ceil(per / chunks), block j walks
# [j chunk, ..): float4s when (per | lo) & 3 == 0 and both image pointers are 16-byte aligned, scalars otherwise.
# (N, per, data_range, scale: 'mean' = 1 / per or 'one', misaligned)
SQDIFF = ((3, 1, 1.0, "mean", 0), (2, 1003, 255.0, "mean", 0), (2, 1003, 1.0, "one", 0), (2, 16388, 1.0, "one", 0),
          (2, 16388, 255.0, "mean", 0), (2, 4200004, 255.0, "mean", 0), (2, 1004, 1.0, "one", 1), (2, 1004, 255.0, "mean", 0))
# npvp_ssim_per_image: one instantiation per window, 32 x 32 tiles.  (window, N, C, H, W)
SSIM = tuple((ws,) + s for ws in (3, 5, 7, 11) for s in ((1, 1, 1, 1), (2, 3, 33, 31), (1, 1, 2, 70)))
# npvp_u8hwc_to_f32chw: here for the canaries only.  (C, H, W), 7 frames
U8 = ((1, 64, 64), (3, 45, 70), (4, 5, 3))
U8_FRAMES = 7

CASES = {"adamw": ADAMW, "clip": CLIP, "l1": L1, "sum": SUM, "mid": MID, "transpose": TRANSPOSE, "colsum": COLSUM, "dwtb": DWTB,
         "bias_act": BIAS_ACT, "act_bwd": ACT_BWD, "sqdiff": SQDIFF, "ssim": SSIM}
SEED = {f: 3000 + 1000 * i for i, f in enumerate(CASES)}
SEED["drop"], SEED["u8"] = 20000, 21000

KINDS = {"adamw": dict(dp="elem", m="elem", v="elem", g="bits"), "clip": dict(norm="scalar", coef="scalar"),
         "l1": dict(l1="scalar", da="bits"), "sum": dict(sum="scalar"), "mid": dict(reduce="elem", broadcast="bits"),
         "transpose": dict(t="bits"), "colsum": dict(colsum="elem"), "dwtb": dict(wtb="bits", gw="bits", gb="bits"),
         "bias_act": dict(y="elem"), "act_bwd": dict(dx="elem"), "sqdiff": dict(sq="elem"), "ssim": dict(ssim="elem")}

MUTANTS = {"adamw": ("no_bias_correction", "coupled_decay", "eps_in_sqrt", "range_shifted", "range_to_quads", "tail_unclipped"),
           "clip": ("no_1e-6", "no_clamp", "tail_skipped"),
           "l1": ("tail_skipped", "mean_over_quads", "sign0_is_1"),
           "sum": ("tail_skipped",),
           "mid": ("scale_on_out", "last_b_skipped"),
           "colsum": ("last_chunk_dropped", "stride_n"),
           "transpose": ("rc_swapped",),
           "dwtb": ("tap_channel_swapped",),
           "bias_act": ("channel_e_mod_c", "residual_before_act"),
           "act_bwd": ("sigmoid_grad_in_x",),
           "sqdiff": ("range_after_square", "tail_dropped"),
           "ssim": ("replicate_pad", "window_unnormalised", "c1_c2_swapped")}


def seed_of(family, case):
    return SEED[family] + 10 * CASES[family].index(case)


def ids(case):
    return case_id(tuple("-".join(map(str, v)) if isinstance(v, tuple) else v for v in case))


def label(family, case):
    return f"{family}[{ids(case)}]"


# ------------------------------------------------------------------------------------------------------------------- routes
def split_chunks(items, wanted):
    """csrc/partials.h split_chunks: -> (items per chunk, chunks that are not empty)"""
    per = -(-items // wanted)
    return per, -(-items // per)


def colsum_chunks(rows):
    """-> (chunks the workspace query reserves, rows per chunk, chunks used)"""
    wanted = min(rows, 128)
    return (wanted,) + split_chunks(rows, wanted)


def sqdiff_chunks(per):
    """-> (chunks, chunk length) of npvp_sqdiff_per_image (csrc/metrics.hip sq_chunks and the kernel's first lines)"""
    chunks = min(max(-(-per // 16384), 1), 256)
    return chunks, -(-per // chunks)


def sqdiff_block_is_vector(per, image, block, misaligned):
    chunks, chunk = sqdiff_chunks(per)
    return ((per | (block * chunk)) & 3) == 0 and (image * per + misaligned) % 4 == 0


def bias_act_is_vector(case):
    lay, outer, inner, C, act, r, mis = case
    return inner % 4 == 0 and not mis


# ------------------------------------------------------------------------------------------------------------------- comparison
def elem_err(a, b, floor):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    den = b.abs()
    den = torch.maximum(den, floor.detach().double().cpu().flatten()) if torch.is_tensor(floor) else den.clamp_min(float(floor))
    return float(((a - b).abs() / den.clamp_min(1e-300)).max())


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype == torch.float32 and a.numel() == b.numel() and torch.equal(a.flatten().view(torch.int32), b.flatten().view(torch.int32))


def measure(family, got, ref, floor):
    """-> [(output, metric, error, bar)] of a case's outputs `got` against `ref`; floor = floors(family, case).  A bar of 0 asks
    for equality: its error is 0 or the rel-L2 of the difference (inf if that is 0 too, or the shapes differ)."""
    assert set(got) == set(ref) == set(KINDS[family]), (sorted(got), sorted(ref))
    out = []
    for k, kind in KINDS[family].items():
        a, b = got[k], ref[k]
        if kind == "bits":
            e = 0.0 if same_bits(a, b) else (rel(a, b) or INF) if a.numel() == b.numel() else INF
            out.append((k, "bits", e, 0.0))
            continue
        assert tuple(a.shape) == tuple(b.shape), f"{k}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
        if kind == "scalar":
            out.append((k, "abs-rel", elem_err(a, b, floor[k]), SCALAR_BOUND))
            continue
        e, er = errors(a, b)
        out += [(k, "rel-l2", e, BOUND), (k, "row", er, BOUND)]
        if kind == "elem":
            out.append((k, "elem", elem_err(a, b, floor[k]), BOUND))
    return out


def ratio(e, bar):
    if e != e:
        return INF
    return (0.0 if e == 0 else INF) if bar == 0 else e / bar


def worst_ratio(family, case, got, ref=None):
    """the largest error / bar over the outputs of a case: what `close_case` holds to 1"""
    return max(ratio(e, bar) for (_, _, e, bar) in measure(family, got, ref64(family, case) if ref is None else ref, floors(family, case)))


def close_case(family, case, got, log=None):
    """the kernel's outputs of a case against the float64 reference, every output measured (and, with a log file, written as
    `case output metric error bar fp32-cpu-error`) before the case fails"""
    ref, fl = ref64(family, case), floors(family, case)
    rows = measure(family, got, ref, fl)
    if log:
        own = {(k, m): e for (k, m, e, _) in measure(family, ref32(family, case), ref, fl)}
        with open(log, "a") as f:
            for (k, m, e, bar) in rows:
                f.write(f"{label(family, case)} {k} {m} {e:.3e} {bar:.0e} {own[(k, m)]:.3e}\n")
    bad = [f"{k} {m} {e:.3e} > {bar:.0e}" for (k, m, e, bar) in rows if not ratio(e, bar) <= 1.0]
    assert not bad, f"{label(family, case)}: " + "; ".join(bad)
    for k, t in got.items():
        assert not torch.isnan(t).any(), f"{label(family, case)}: NaN in {k}"


# ------------------------------------------------------------------------------------------------------------------- AdamW, clip
def adamw_inputs(case):
    """pre-seeded state.  v = 1e-3 (0.1 + randn^2): with lr / bc1 = 0.037 and sqrt(bc2) = 0.055 at step 3 the update is 2e-3
    m / sqrt(v) - about |p| itself.  (At v of order 0.1 it is a tenth of that, and p afterwards - p before then shows the fp32
    rounding of p at 3e-6 of the update, in the CPU's fp32 too.)"""
    n, s = case[0], seed_of("adamw", case)
    return dict(p=0.1 * O.seeded_randn((n,), s), g=O.seeded_randn((n,), s + 1), m=O.seeded_randn((n,), s + 2),
                v=1e-3 * (0.1 + O.seeded_randn((n,), s + 3) ** 2), coef=torch.tensor(ADAMW_COEF, dtype=torch.float32))


def adamw_mask(n, rng, mutant=None):
    """which elements the clip coefficient multiplies"""
    i = torch.arange(n)
    if rng is None:
        return torch.zeros(n, dtype=torch.bool)
    b, e = rng
    if mutant == "range_shifted":
        b, e = b + 1, e + 1
    if mutant == "range_to_quads":
        b, e = b & ~3, (e + 3) & ~3
    mask = (i >= b) & (i < e)
    if mutant == "tail_unclipped":
        mask &= i < (n & ~3)
    return mask


def adamw_formula(p, g, m, v, lr, step, beta1, beta2, eps, wd, mutant=None):
    """one step of torch.optim.AdamW (decoupled decay, bias-corrected moments, eps outside the root): the tensor operations in the
    dtype of p, the scalars (1 - lr wd, 1 - beta^step, lr / bc1, sqrt(bc2)) as Python floats, which is how torch's own
    single-tensor AdamW takes them whatever the parameter's dtype.  -> p, m, v"""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    if mutant == "no_bias_correction":
        bc1, bc2 = 1.0, 1.0
    if mutant == "coupled_decay":
        g = g + wd * p
    else:
        p = p * (1.0 - lr * wd)
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    denom = torch.sqrt(v / bc2 + eps) if mutant == "eps_in_sqrt" else torch.sqrt(v) / math.sqrt(bc2) + eps
    return p - (lr / bc1) * m / denom, m, v


def adamw_reference(case, dtype=torch.float64, mutant=None):
    """-> dp (p afterwards - p before), m, v, and g afterwards (fp32: g * coef is one fp32 product) after `calls` calls"""
    n, rng, wb, wd, eps, calls = case
    i = adamw_inputs(case)
    mask = adamw_mask(n, rng, mutant)
    p, m, v, g32, coef = i["p"].to(dtype), i["m"].to(dtype), i["v"].to(dtype), i["g"], i["coef"]
    for (lr, step) in ADAMW_HYPER[:calls]:
        gc32 = torch.where(mask, g32 * coef, g32)
        p, m, v = adamw_formula(p, gc32.to(dtype), m, v, f32(lr), step, f32(ADAMW_BETAS[0]), f32(ADAMW_BETAS[1]), f32(eps), f32(wd), mutant)
        if wb:
            g32 = gc32
    return dict(dp=p - i["p"].to(dtype), m=m, v=v, g=g32)


def adamw_floors(case):
    """m = beta1 m + (1 - beta1) g and p = p decay - update are rounded from their terms: the floor of an element is the sum of the
    absolute terms for m, a tenth of |p| per call for the update (two roundings at |p| a call: 2^-23 |p| = 1.2e-7 |p| is BOUND / 4 of 0.05 |p|;
    an update below that is below what an fp32 parameter resolves) plus the update the absolute terms of m would give (where m
    cancels, the update inherits its error); v is a sum of positive terms: no floor"""
    n, rng, wb, wd, eps, calls = case
    i = adamw_inputs(case)
    mask = adamw_mask(n, rng)
    g, m, v, up = i["g"].double().abs(), i["m"].double().abs(), i["v"].double(), torch.zeros(n, dtype=torch.float64)
    for (lr, step) in ADAMW_HYPER[:calls]:          # the formula on |m| and |g|: -> the absolute terms of m, and the update they give
        gc = torch.where(mask, g * ADAMW_COEF, g)
        q, m, v = adamw_formula(torch.zeros_like(up), gc, m, v, f32(lr), step, f32(ADAMW_BETAS[0]), f32(ADAMW_BETAS[1]), f32(eps), 0.0)
        up, g = up - q, (gc if wb else g)
    return dict(dp=0.1 * calls * i["p"].abs().double() + up, m=m, v=0.0)


def clip_coef(norm, max_norm, mutant=None):
    c = max_norm / (norm + (0.0 if mutant == "no_1e-6" else 1e-6))
    return c if mutant == "no_clamp" else torch.clamp(c, max=1.0)


def clip_inputs(case):
    n, kind = case
    want, max_norm = CLIP_SCALE[kind]
    return dict(g=O.seeded_randn((n,), seed_of("clip", case)) * (want / math.sqrt(n)), max_norm=f32(max_norm))


def clip_reference(case, dtype=torch.float64, mutant=None):
    """torch.nn.utils.clip_grad_norm_: -> norm, coef = min(1, max_norm / (norm + 1e-6))"""
    i = clip_inputs(case)
    g = i["g"].to(dtype)
    if mutant == "tail_skipped":
        g = g[:case[0] & ~3]
    norm = torch.sqrt((g * g).sum())
    return dict(norm=norm.reshape(1), coef=clip_coef(norm, torch.tensor(i["max_norm"], dtype=dtype), mutant).reshape(1))


# ------------------------------------------------------------------------------------------------------------------- scalar losses
def l1_inputs(case):
    (n,), s = case, seed_of("l1", case)
    a, b = O.seeded_randn((n,), s), O.seeded_randn((n,), s + 1)
    b[::7] = a[::7]
    return dict(a=a, b=b, gout=torch.tensor([L1_GOUT], dtype=torch.float32), lam=f32(L1_LAM))


def l1_reference(case, dtype=torch.float64, mutant=None):
    """-> l1 = lam mean |a - b|; da = c sign(a - b) with c = (gout lam) / n in fp32 (exactly the kernel's three operations)"""
    (n,) = case
    i = l1_inputs(case)
    d = (i["a"].to(dtype) - i["b"].to(dtype)).abs()
    s = (d[:n & ~3] if mutant == "tail_skipped" else d).sum()
    l1 = s / (max(n & ~3, 1) if mutant == "mean_over_quads" else n) * i["lam"]
    c = (i["gout"] * torch.tensor(i["lam"], dtype=torch.float32)) / torch.tensor(float(n), dtype=torch.float32)
    sg = torch.sign(i["a"] - i["b"])
    if mutant == "sign0_is_1":
        sg = torch.where(i["a"] == i["b"], torch.ones_like(sg), sg)
    return dict(l1=l1.reshape(1), da=c * sg)


def sum_inputs(case):
    return dict(x=O.seeded_randn(case, seed_of("sum", case)))


def sum_reference(case, dtype=torch.float64, mutant=None):
    x = sum_inputs(case)["x"].to(dtype)
    return dict(sum=(x[:case[0] & ~3] if mutant == "tail_skipped" else x).sum().reshape(1))


# ------------------------------------------------------------------------------------------------------------------- layout helpers
def mid_inputs(case):
    A, B, Cc, acc = case
    s = seed_of("mid", case)
    return dict(x=O.seeded_randn((A, B, Cc), s), out0=O.seeded_randn((A, Cc), s + 1), y=O.seeded_randn((A, Cc), s + 2), scale=f32(MID_SCALE))


def mid_reference(case, dtype=torch.float64, mutant=None):
    """-> reduce [A, Cc] = scale sum_b x (+ out0); broadcast [A, B, Cc] = scale y (fp32: one product)"""
    A, B, Cc, acc = case
    i = mid_inputs(case)
    x = i["x"].to(dtype)
    s = (x[:, :B - 1] if mutant == "last_b_skipped" else x).sum(1)
    if mutant == "scale_on_out" and acc:
        r = (s + i["out0"].to(dtype)) * i["scale"]
    else:
        r = s * i["scale"] + (i["out0"].to(dtype) if acc else 0)
    bc = (i["y"] * torch.tensor(i["scale"], dtype=torch.float32))[:, None, :].expand(A, B, Cc).contiguous()
    return dict(reduce=r, broadcast=bc)


def mid_floors(case):
    i = mid_inputs(case)
    return dict(reduce=i["x"].double().abs().sum(1) * MID_SCALE + (i["out0"].double().abs() if case[3] else 0))


def transpose_inputs(case):
    return dict(x=O.seeded_randn(case, seed_of("transpose", case)))


def transpose_reference(case, dtype=torch.float64, mutant=None):
    """[batch][R][C] -> [batch][C][R], a copy.  Mutant: every batch read as [C][R] (R and C exchanged on the input side)"""
    b, R, C = case
    x = transpose_inputs(case)["x"]
    return dict(t=(x.reshape(b, C, R) if mutant == "rc_swapped" else x).transpose(1, 2).contiguous())


def colsum_inputs(case):
    """full [rows, ld]: the storage, gap columns included (the GPU test makes them NaN); x = full[:, :N]"""
    rows, N, ld, acc = case
    s = seed_of("colsum", case)
    return dict(full=O.seeded_randn((rows, ld), s), out0=O.seeded_randn((N,), s + 1))


def colsum_reference(case, dtype=torch.float64, mutant=None):
    rows, N, ld, acc = case
    i = colsum_inputs(case)
    x = i["full"][:, :N].to(dtype)
    if mutant == "stride_n":
        x = i["full"].flatten()[:rows * N].reshape(rows, N).to(dtype)
    if mutant == "last_chunk_dropped":
        _, per, used = colsum_chunks(rows)
        x = x[:(used - 1) * per]
    return dict(colsum=x.sum(0) + (i["out0"].to(dtype) if acc else 0))


def colsum_floors(case):
    i = colsum_inputs(case)
    return dict(colsum=i["full"][:, :case[1]].double().abs().sum(0) + (i["out0"].double().abs() if case[3] else 0))


def dwtb_inputs(case):
    C, hb = case
    s = seed_of("dwtb", case)
    return dict(w=O.seeded_randn((C, 9), s), b=O.seeded_randn((C,), s + 1) if hb else None, dwtb=O.seeded_randn((10, C), s + 2),
                gw0=O.seeded_randn((C, 9), s + 3), gb0=O.seeded_randn((C,), s + 4))


def dwtb_reference(case, dtype=torch.float64, mutant=None):
    """-> wtb [10][C] = (w [C][9] transposed, then b or zeros): copies; gw = gw0 + dwtb[:9] transposed, gb = gb0 + dwtb[9]: one fp32
    sum each"""
    C, hb = case
    i = dwtb_inputs(case)
    taps = i["w"].flatten().reshape(9, C) if mutant == "tap_channel_swapped" else i["w"].t()
    wtb = torch.cat([taps, (i["b"] if hb else torch.zeros(C)).reshape(1, C)], 0).contiguous()
    return dict(wtb=wtb, gw=i["gw0"] + i["dwtb"][:9].t(), gb=i["gb0"] + i["dwtb"][9])


def drop_inputs(case):
    rows, ncols = case[0], case[1]
    return dict(x=1.0 + O.seeded_randn((1030, 4100), SEED["drop"]).abs()[:rows, :ncols].contiguous())


def drop_inv_keep(p):
    """csrc/common.h make_drop_spec: 1.f / (1.f - p) in fp32"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


# ------------------------------------------------------------------------------------------------------------------- epilogues
def _act(u, act):
    return (u, torch.relu(u), torch.tanh(u), torch.sigmoid(u))[act]


def bias_act_inputs(case):
    lay, outer, inner, C, act, r, mis = case
    s = seed_of("bias_act", case)
    return dict(x=O.seeded_randn((outer, inner), s), bias=O.seeded_randn((C,), s + 1), res=O.seeded_randn((outer, inner), s + 2) if r else None)


def bias_act_reference(case, dtype=torch.float64, mutant=None):
    """y = act(x + bias[channel]) (+ residual); channel = column (layout 0) or row % C (layout 1)"""
    lay, outer, inner, C, act, r, mis = case
    i = bias_act_inputs(case)
    x, bias = i["x"].to(dtype), i["bias"].to(dtype)
    if lay == 0:
        b = bias.reshape(1, C)
    elif mutant == "channel_e_mod_c":
        b = bias[torch.arange(outer * inner) % C].reshape(outer, inner)
    else:
        b = bias[torch.arange(outer) % C].reshape(outer, 1)
    res = i["res"].to(dtype) if r else 0
    if mutant == "residual_before_act" and r:
        return dict(y=_act(x + b + res, act))
    return dict(y=_act(x + b, act) + res)


def bias_act_floors(case):
    i = bias_act_inputs(case)
    lay, outer, inner, C = case[:4]
    b = i["bias"].double().abs()
    b = b.reshape(1, C) if lay == 0 else b[torch.arange(outer) % C].reshape(outer, 1)
    return dict(y=i["x"].double().abs() + b + (i["res"].double().abs() if case[5] else 0))


def act_bwd_inputs(case):
    """y: the fp32 forward output act(x) the kernel is fed"""
    n, act = case
    s = seed_of("act_bwd", case)
    return dict(g=O.seeded_randn((n,), s), y=_act(O.seeded_randn((n,), s + 1).double(), act).float())


def act_bwd_reference(case, dtype=torch.float64, mutant=None):
    """dx = g act'(.) through the forward OUTPUT y: ReLU y > 0, tanh 1 - y^2, sigmoid y (1 - y)"""
    n, act = case
    i = act_bwd_inputs(case)
    g, y = i["g"].to(dtype), i["y"].to(dtype)
    if mutant == "sigmoid_grad_in_x" and act == 3:
        y = torch.sigmoid(y)
    d = (torch.ones_like(y), (y > 0).to(dtype), 1 - y * y, y * (1 - y))[act]
    return dict(dx=g * d)


def act_bwd_floors(case):
    return dict(dx=act_bwd_inputs(case)["g"].double().abs())          # |act'| <= 1, rounded at 1 (1 - y^2, 1 - y)


# ------------------------------------------------------------------------------------------------------------------- metrics
def sqdiff_inputs(case):
    N, per, rng, sk, mis = case
    s = seed_of("sqdiff", case)
    x = (0.5 + 0.25 * O.seeded_randn((N, per), s)).clamp(0, 1) * rng
    return dict(x=x, y=(x + 0.1 * rng * O.seeded_randn((N, per), s + 1)).clamp(0, rng), data_range=f32(rng), scale=f32(1.0 / per) if sk == "mean" else 1.0)


def sqdiff_reference(case, dtype=torch.float64, mutant=None):
    """sq[n] = scale sum_i ((x - y) / data_range)^2"""
    N, per, rng, sk, mis = case
    i = sqdiff_inputs(case)
    d = i["x"].to(dtype) - i["y"].to(dtype)
    if mutant == "tail_dropped":
        d = d[:, :per & ~3]
    inv = torch.tensor(1.0, dtype=dtype) / i["data_range"]
    sq = (d * d * inv) if mutant == "range_after_square" else (d * inv) ** 2
    return dict(sq=sq.sum(1) * i["scale"])


def ssim_inputs(case):
    ws, N, C, H, W = case
    s = seed_of("ssim", case)
    a = (0.5 + 0.25 * O.seeded_randn((N, C, H, W), s)).clamp(0, 1)
    return dict(a=a, b=(a + 0.1 * O.seeded_randn((N, C, H, W), s + 1)).clamp(0, 1), taps=OM.gaussian_taps(ws))


def ssim_restated(a, b, ws, mutant=None):
    """oracle.metrics.ssim_per_image (the fp32 taps of gaussian_taps, five zero-padded grouped convolutions, C1 = 0.01^2,
    C2 = 0.03^2) in the dtype of a, written out so that a mutant can get it wrong; mutant None equals the oracle (host test)"""
    C, r = a.shape[1], ws // 2
    g = OM.gaussian_taps(ws)
    if mutant == "window_unnormalised":
        g = torch.tensor([math.exp(-(k - r) ** 2 / 4.5) for k in range(ws)], dtype=torch.float32)
    g = g.to(a)
    win = torch.outer(g, g)[None, None].expand(C, 1, ws, ws).contiguous()
    pad = (lambda t: F.pad(t, (r, r, r, r), mode="replicate")) if mutant == "replicate_pad" else (lambda t: F.pad(t, (r, r, r, r)))
    blur = lambda t: F.conv2d(pad(t), win, groups=C)
    ma, mb = blur(a), blur(b)
    va, vb, cab = blur(a * a) - ma * ma, blur(b * b) - mb * mb, blur(a * b) - ma * mb
    c1, c2 = (0.03 ** 2, 0.01 ** 2) if mutant == "c1_c2_swapped" else (0.01 ** 2, 0.03 ** 2)
    smap = ((2 * ma * mb + c1) * (2 * cab + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2))
    return smap.mean(dim=(1, 2, 3))


def ssim_reference(case, dtype=torch.float64, mutant=None):
    i = ssim_inputs(case)
    a, b = i["a"].to(dtype), i["b"].to(dtype)
    return dict(ssim=OM.ssim_per_image(a, b, case[0]) if mutant is None else ssim_restated(a, b, case[0], mutant))


def u8_inputs(case):
    C, H, W = case
    rng = np.random.default_rng(SEED["u8"] + 100 * C + H)
    return dict(src=rng.integers(0, 256, size=(U8_FRAMES, H, W, C), dtype=np.uint8), mean=np.linspace(0.2, 0.6, C).astype(np.float32),
                std=np.linspace(1.1, 2.3, C).astype(np.float32))


def u8_reference(case):
    i = u8_inputs(case)
    return (i["src"].astype(np.float64).transpose(0, 3, 1, 2) / 255.0 - i["mean"].astype(np.float64)[None, :, None, None]) / \
        i["std"].astype(np.float64)[None, :, None, None]


# ------------------------------------------------------------------------------------------------------------------- dispatch
def inputs(family, case):
    return globals()[family + "_inputs"](case)


def reference(family, case, dtype=torch.float64, mutant=None):
    with torch.no_grad():
        return globals()[family + "_reference"](case, dtype, mutant)


def floors(family, case):
    """{output: floor} for the 'elem' and 'scalar' outputs of a case (see the module's head); 0 where every term has one sign"""
    if family + "_floors" in globals():
        return globals()[family + "_floors"](case)
    if family == "sum":
        return dict(sum=sum_inputs(case)["x"].double().abs().sum())
    return {k: 0.0 for k in KINDS[family]}              # clip, l1, sqdiff: sums of non-negative terms; ssim: a mean of O(1) values


@functools.lru_cache(maxsize=None)
def ref64(family, case):
    """the float64 reference of a case: computed once, shared, never written to"""
    return reference(family, case, torch.float64)


def ref32(family, case):
    """the same formula in fp32 on the CPU: the reference's own arithmetic noise"""
    return reference(family, case, torch.float32)


# ------------------------------------------------------------------------------------------------------------------- padded buffers
# (the GPU tests' operands and outputs: tests/test_hip_helper_kernels.py says what they are for; tests/test_hip_hot_kernels.py
# shares them)
DEV = "cuda:0"
PATTERN = 0x7FC0BEEF          # a quiet NaN with a payload: recognisable, and poison for whoever reads it as a number
PAD = 8                       # floats in front of and behind every view


class Flat:
    """n floats inside a larger allocation.  kind 'in': NaN around the values; 'out': the bit pattern around (and, without values,
    in) the view.  shift: floats by which the view starts off 16-byte alignment."""

    def __init__(self, values=None, n=None, kind="in", shift=0):
        self.n = int(values.numel() if values is not None else n)
        self.lo = PAD + shift
        self.base = torch.empty(self.n + 2 * PAD + 4, dtype=torch.float32, device=DEV)
        if kind == "in":
            self.base.fill_(float("nan"))
        else:
            self.base.view(torch.int32).fill_(PATTERN)
        self.v = self.base[self.lo:self.lo + self.n]
        if values is not None:
            self.v.copy_(values.flatten())
        self.ptr = self.v.data_ptr()
        assert self.ptr % 16 == 4 * (shift % 4)

    def intact(self):
        i = self.base.view(torch.int32)
        return bool((i[:self.lo] == PATTERN).all()) and bool((i[self.lo + self.n:] == PATTERN).all())

    def cpu(self, *shape):
        t = self.v.cpu()
        return t.reshape(shape) if shape else t


def out_flat(n, values=None):
    return Flat(values, n, kind="out")
