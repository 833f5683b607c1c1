"""The cases of tests/test_hip_grid_kernels.py (GPU) and tests/test_grid_kernel_cases_host.py (CPU): the norm, depthwise-conv,
im2col and attention kernels a feature grid other than 8 x 8 falls back to, at the smallest shapes that reach each of their branches.

Per family: a case table, an input builder (oracle.ops.seeded_randn: fp32 values, cast to the dtype asked for), and the reference =
the UNCHANGED oracle.ops functions in float64 on the CPU with autograd for every gradient (im2col, which the oracle does not have,
is F.pad + slicing; col2im is its autograd adjoint).  reference(family, case, dtype, mutant) -> {output name: tensor}.

MUTANTS are deliberately wrong references - the defects a kernel of each family can have.  The host test requires that `worst`
(the comparison the GPU test applies) puts each of them at >= 10 x BOUND in some case of its family: the tables can see what they
claim to see.  The same host test holds the fp32 CPU oracle to BOUND / 4 on every case, so the bound is not inside the reference's
own noise.

BOUND = 1e-5 for the whole-tensor rel-L2 and for the worst row (golden_cases.max_row_rel_err, floor 1e-6).  Not fitted to the
kernels: no GEMM is involved, and tests/test_hip_ops.py records a measured worst of 7e-6 over every op test, split-precision GEMMs
included.  Every case holds it (profiles/grid_kernels_errors.txt: worst 1.7e-6)."""
import functools
import math
import os

import torch
import torch.nn.functional as F

from golden_cases import max_row_rel_err
from oracle import ops as O

BOUND = 1e-5
ROW_FLOOR = 1e-6

# ------------------------------------------------------------------------------------------------------------------- case tables
# (frames, H, W, Ch).  3x3x260: a second block of 64 channel quads with ONE live quad, P % 4 = 1; 1x5 / 5x1: one row / one column
# (every vertical / horizontal tap out of the grid); 300 frames: more than the 256 chunks of the weight gradient's partials
DWCONV = ((3, 3, 3, 260), (2, 1, 5, 64), (2, 5, 1, 64), (3, 6, 10, 1024), (300, 2, 2, 4), (1, 10, 14, 64))
IM2COL = ((2, 3, 3, 4), (1, 1, 5, 512), (2, 6, 10, 64))
# (N, T, P, C, add, gamma, input): input 'plain' x = 0.5 + randn; 'flat' x = 0.5 + 0.02 randn (variance 4e-4: eps = 1e-5 is 2.5 % of
# it); 'shift' x = 30 + randn (the one-pass variance about a shift).  18x2x4x512: per_frame % 1024 == 0 yet the unfused backward
# (4 blocks, N > 16); 2x3x3x512: per_frame 1536 < 2048; 3x2x60x512: the fused backward (npvp_posfuse_bwd_fused == 1)
POSFUSE_LAYER = ((3, 4, 9, 512, 1, 1, "plain"), (18, 2, 9, 512, 1, 0, "plain"), (18, 2, 4, 512, 0, 1, "plain"),
                 (3, 2, 60, 512, 1, 1, "plain"), (2, 3, 3, 512, 0, 0, "plain"), (2, 2, 5, 48, 1, 1, "plain"),
                 (2, 3, 9, 512, 0, 1, "flat"), (3, 2, 60, 512, 1, 1, "shift"))
POSFUSE_INSTANCE = ((2, 3, 9, 512, 1, 1, "plain"), (2, 3, 9, 260, 0, 1, "plain"), (2, 3, 5, 512, 1, 0, "plain"),
                    (2, 3, 5, 260, 1, 1, "plain"), (2, 3, 60, 512, 0, 0, "plain"), (2, 3, 60, 260, 1, 1, "plain"),
                    (2, 3, 9, 260, 1, 1, "flat"))
POSFUSE_INSTANCE_TOO_MANY_PIXELS = 140
# (frames, P, Ch, residual, input)
FRAMELN = tuple((f, p, ch, r, "plain") for (f, p, ch) in ((1, 9, 512), (5, 9, 512), (33, 5, 48), (3, 60, 1024), (600, 1, 16))
                for r in (0, 1)) + ((5, 9, 512, 1, "flat"),)
FRAMELN_BAD_PER_FRAME = (2, 3, 4)              # per_frame = 12: forward runs, backward refuses ("multiple of 16")
FRAMELN_DROPPATH = dict(frames=32, frames_per_sample=2, P=5, Ch=48, p_dp=0.5)
# (rows, C, relu, input)
LAYERNORM = tuple((rows, C, relu, "plain") for C in (256, 768, 1024) for rows in (1, 3, 1001) for relu in (0, 1)) + ((3, 256, 0, "flat"),)
LAYERNORM_RES = (5, 768)
# (N, P, Tq, Tk, mask, heads); C = 64 heads.  heads 1 and 3 with 9 groups: 9 and 27 (group, head) pairs, a last block of 1 / 3 waves
ATTN_TEMPORAL = ((2, 9, 4, 4, 1, 8), (1, 9, 18, 2, 0, 8), (1, 60, 5, 28, 0, 8), (1, 9, 20, 20, 1, 8), (1, 9, 40, 33, 0, 8),
                 (1, 9, 4, 4, 0, 1), (1, 9, 5, 20, 0, 3))
ATTN_TEMPORAL_W = {9: 3, 60: 10}              # the grid width the models put into the configuration beside P (3 x 3, 6 x 10)
# (frames, H, W, window); 8 heads, C = 512
ATTN_SPATIAL = ((1, 4, 12, 4), (2, 12, 4, 4), (1, 2, 6, 2), (1, 8, 16, 8))
SPATIAL_HEADS = 8

CASES = {"dwconv": DWCONV, "im2col": IM2COL, "posfuse_layer": POSFUSE_LAYER, "posfuse_instance": POSFUSE_INSTANCE,
         "frameln": FRAMELN, "layernorm": LAYERNORM, "attn_temporal": ATTN_TEMPORAL, "attn_spatial": ATTN_SPATIAL}
SEED = {"dwconv": 1100, "im2col": 1200, "posfuse_layer": 1300, "posfuse_instance": 1400, "frameln": 1500, "layernorm": 1600,
        "attn_temporal": 1700, "attn_spatial": 1800, "layernorm_res": 1900, "droppath": 1950}

NORM_MUTANTS = ("unbiased", "eps0")
MUTANTS = {"dwconv": ("taps_transposed", "dgrad_unflipped", "wrap", "wgrad_last_pixel"),
           "im2col": ("wrap",),
           "posfuse_layer": NORM_MUTANTS + ("tail4", "table_by_n", "add_by_frame"),
           "posfuse_instance": NORM_MUTANTS + ("tail4", "table_by_n", "add_by_frame"),
           "frameln": NORM_MUTANTS + ("tail4",),
           "layernorm": NORM_MUTANTS,
           "attn_temporal": ("mask_transposed", "q_unscaled"),
           "attn_spatial": ("grid_swapped", "q_unscaled")}


def case_id(case):
    return "x".join(str(v) for v in case)


def seed_of(family, case):
    return SEED[family] + 10 * CASES[family].index(case)


# ------------------------------------------------------------------------------------------------------------------- comparison
def rel(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-300))


def errors(a, b):
    """-> (whole-tensor rel-L2, worst-row rel-L2) of a against the reference b"""
    assert tuple(a.shape) == tuple(b.shape), f"shape {tuple(a.shape)} vs {tuple(b.shape)}"
    return rel(a, b), max_row_rel_err(a, b, ROW_FLOOR)


def worst(got, ref):
    """the larger of the two errors, over every output of a case: what `close` holds against the bound"""
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    return max(max(errors(got[k], ref[k])) for k in ref)


def close(case, what, a, b, bound=BOUND, fp32=None):
    """a (the kernel's) against b (float64 reference): both errors within `bound`.  With NPVP_ERR_LOG set, appends
    `case what err row_err fp32_cpu_err` (fp32: the fp32 CPU oracle's tensor; its error against b is the larger of its two)."""
    e, er = errors(a, b)
    if os.environ.get("NPVP_ERR_LOG"):
        fe = "-" if fp32 is None else f"{max(errors(fp32, b)):.3e}"
        with open(os.environ["NPVP_ERR_LOG"], "a") as f:
            f.write(f"{case} {what} {e:.3e} {er:.3e} {fe}\n")
    assert e <= bound, f"{case} {what}: rel-L2 {e:.3e} > {bound:.1e}"
    assert er <= bound, f"{case} {what}: worst-row rel-L2 {er:.3e} > {bound:.1e}"


def close_all(family, case, got):
    """every output of a case (got: {name: tensor}) against the float64 reference, the fp32 CPU oracle's error logged beside it"""
    ref, f32 = ref64(family, case), ref32(family, case)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    failures = []
    for k in ref:
        try:
            close(f"{family}[{case_id(case)}]", k, got[k], ref[k], BOUND, f32[k])
        except AssertionError as e:              # (every output is measured and logged before the case fails)
            failures.append(str(e))
    assert not failures, "; ".join(failures)


# ------------------------------------------------------------------------------------------------------------------- helpers
def _leaf(t, dtype):
    return None if t is None else t.to(dtype).clone().requires_grad_()


def _grads(y, cot, leaves):
    """leaves {gradient name: leaf or None} -> {gradient name: d <y, cot> / d leaf}"""
    names = [k for k, v in leaves.items() if v is not None]
    return dict(zip(names, torch.autograd.grad((y * cot).sum(), [leaves[k] for k in names], retain_graph=True)))


def _field(shape, seed, kind):
    r = O.seeded_randn(shape, seed)
    return {"plain": 0.5 + r, "flat": 0.5 + 0.02 * r, "shift": 30.0 + r}[kind]


def _stats(u, dims, eps, mutant):
    """mean and 1 / sqrt(biased variance + eps) over `dims`; mutants: Bessel's n - 1, no eps"""
    mu = u.mean(dim=dims, keepdim=True)
    var = ((u - mu) ** 2).mean(dim=dims, keepdim=True)
    if mutant == "unbiased":
        n = math.prod(u.shape[d] for d in dims)
        var = var * (n / (n - 1.0)) if n > 1 else var
    return mu, torch.rsqrt(var + (0.0 if mutant == "eps0" else eps))


def _tail4(xh, u):
    """the last float4 of each frame's flat elements left as it came in (a vector loop that ends one step early)"""
    Fr = xh.shape[0]
    return torch.cat([xh.reshape(Fr, -1)[:, :-4], u.reshape(Fr, -1)[:, -4:]], 1).reshape(xh.shape)


# ------------------------------------------------------------------------------------------------------------------- depthwise 3x3
def dwconv_inputs(case, dtype=torch.float32):
    Fr, H, W, Ch = case
    s = seed_of("dwconv", case)
    return dict(a=_leaf(O.seeded_randn((Fr, H * W, Ch), s), dtype), w=_leaf(0.3 * O.seeded_randn((Ch, 3, 3), s + 1), dtype),
                b=_leaf(0.1 * O.seeded_randn((Ch,), s + 2), dtype), cot=O.seeded_randn((Fr, H * W, Ch), s + 3).to(dtype))


def _dwconv_wrap(h, w, b, H, W):
    """the convolution with indices taken modulo the grid instead of a zero border"""
    Fr, P, Ch = h.shape
    x = h.reshape(Fr, H, W, Ch)
    y = b.reshape(1, 1, 1, Ch).expand(Fr, H, W, Ch)
    for ky in (-1, 0, 1):
        for kx in (-1, 0, 1):
            y = y + torch.roll(x, (-ky, -kx), (1, 2)) * w[:, ky + 1, kx + 1]
    return y.reshape(Fr, P, Ch)


def dwconv_reference(case, dtype=torch.float64, mutant=None):
    """-> y, da, dw [9, Ch] (tap-major rows, as the kernel's wtb holds them), db"""
    Fr, H, W, Ch = case
    i = dwconv_inputs(case, dtype)
    a, w, b, cot = i["a"], i["w"], i["b"], i["cot"]
    if mutant == "taps_transposed":
        y = O.dwconv3x3(a, w.transpose(1, 2), b, H, W)
    elif mutant == "wrap":
        y = _dwconv_wrap(a, w, b, H, W)
    else:
        y = O.dwconv3x3(a, w, b, H, W)
    g = _grads(y, cot, dict(da=a, dw=w, db=b))
    if mutant == "dgrad_unflipped":             # the forward kernel run on the cotangent with the taps as they are
        g["da"] = O.dwconv3x3(cot, w.detach(), torch.zeros_like(b), H, W)
    if mutant == "wgrad_last_pixel":
        c2 = cot.clone()
        c2[:, H * W - 1] = 0
        g2 = _grads(y, c2, dict(dw=w, db=b))
        g["dw"], g["db"] = g2["dw"], g2["db"]
    return dict(y=y.detach(), da=g["da"].detach(), dw=g["dw"].reshape(Ch, 9).t().contiguous(), db=g["db"])


# ------------------------------------------------------------------------------------------------------------------- im2col
def im2col_inputs(case, dtype=torch.float32):
    Fr, H, W, C = case
    s = seed_of("im2col", case)
    return dict(x=_leaf(O.seeded_randn((Fr, H * W, C), s), dtype), cot=O.seeded_randn((Fr * H * W, 9 * C), s + 1).to(dtype))


def im2col(x, Fr, H, W, wrap=False):
    """[Fr, H*W, C] -> [Fr*H*W, 9 C]: column block tap = 3 (ky + 1) + (kx + 1) of row (f, h, w) is x[f, h + ky, w + kx] (0 outside)"""
    C = x.shape[-1]
    x4 = x.reshape(Fr, H, W, C)
    if wrap:
        taps = [torch.roll(x4, (-ky, -kx), (1, 2)) for ky in (-1, 0, 1) for kx in (-1, 0, 1)]
    else:
        xp = F.pad(x4, (0, 0, 1, 1, 1, 1))
        taps = [xp[:, ky + 1:ky + 1 + H, kx + 1:kx + 1 + W] for ky in (-1, 0, 1) for kx in (-1, 0, 1)]
    return torch.stack(taps, 3).reshape(Fr * H * W, 9 * C)


def im2col_reference(case, dtype=torch.float64, mutant=None):
    """-> cols, dx (= col2im of the cotangent: the autograd adjoint)"""
    Fr, H, W, C = case
    i = im2col_inputs(case, dtype)
    cols = im2col(i["x"], Fr, H, W, wrap=(mutant == "wrap"))
    return dict(cols=cols.detach(), dx=_grads(cols, i["cot"], dict(dx=i["x"]))["dx"])


# ------------------------------------------------------------------------------------------------------------------- posfuse
def posfuse_inputs(family, case, dtype=torch.float32):
    N, T, P, C, has_add, has_gamma, kind = case
    s = seed_of(family, case)
    return dict(x=_leaf(_field((N * T, P, C), s, kind), dtype),
                add=_leaf(O.seeded_randn((N, P, C), s + 1) * (0.02 if kind == "flat" else 1.0), dtype) if has_add else None,
                beta=_leaf(O.seeded_randn((T * P, C), s + 2), dtype),
                gamma=_leaf(0.3 * O.seeded_randn((T * P, C), s + 3), dtype) if has_gamma else None,
                cot=O.seeded_randn((N * T, P, C), s + 4).to(dtype))


def posfuse_restated(x, T, beta, gamma, add, norm, mutant=None):
    """oracle.ops.posfuse written with explicit frame -> (sample, time-step) indices, so that a mutant can get them wrong.
    mutant None equals O.posfuse (the host test holds it to that)."""
    Fr, P, C = x.shape
    N = Fr // T
    f = torch.arange(Fr)
    u = x
    if add is not None:
        u = x + add[(f % N) if mutant == "add_by_frame" else (f // T)]
    mu, rs = _stats(u, (1, 2) if norm == "layer" else (1,), 1e-5, mutant)
    xh = (u - mu) * rs
    if mutant == "tail4":
        xh = _tail4(xh, u)
    t = ((f // T) % T) if mutant == "table_by_n" else (f % T)
    if gamma is not None:
        xh = xh * (1 + gamma.reshape(T, P, C)[t])
    return xh + beta.reshape(T, P, C)[t]


def posfuse_reference(family, case, dtype=torch.float64, mutant=None):
    """-> y, dx, dadd, dbeta, dgamma (those that exist)"""
    T = case[1]
    norm = "layer" if family == "posfuse_layer" else "instance"
    i = posfuse_inputs(family, case, dtype)
    if mutant is None:
        y = O.posfuse(i["x"], T, i["beta"], i["gamma"], i["add"], norm)
    else:
        y = posfuse_restated(i["x"], T, i["beta"], i["gamma"], i["add"], norm, mutant)
    out = _grads(y, i["cot"], dict(dx=i["x"], dadd=i["add"], dbeta=i["beta"], dgamma=i["gamma"]))
    out["y"] = y.detach()
    return out


# ------------------------------------------------------------------------------------------------------------------- frame LN + GELU
def frameln_inputs(case, dtype=torch.float32, seed=None):
    Fr, P, Ch, has_res, kind = case
    s = seed_of("frameln", case) if seed is None else seed
    return dict(h=_leaf(_field((Fr, P, Ch), s, kind) - 0.2, dtype), w=_leaf(1 + 0.1 * O.seeded_randn((P, Ch), s + 1), dtype),
                b=_leaf(0.1 * O.seeded_randn((P, Ch), s + 2), dtype), res=_leaf(O.seeded_randn((Fr, P, Ch), s + 3), dtype) if has_res else None,
                cot=O.seeded_randn((Fr, P, Ch), s + 4).to(dtype))


def frame_ln_mutant(h, w, b, mutant):
    mu, rs = _stats(h, (1, 2), 1e-5, mutant)
    xh = (h - mu) * rs
    if mutant == "tail4":
        xh = _tail4(xh, h)
    return xh * w + b


def frameln_reference(case, dtype=torch.float64, mutant=None, seed=None, frame_scale=None):
    """-> out, dh, dw, db (+ dres).  frame_scale [frames] (drop-path: 0 or 1 / (1 - p) per frame) multiplies the branch."""
    i = frameln_inputs(case, dtype, seed)
    ln = O.frame_ln(i["h"], i["w"], i["b"]) if mutant is None else frame_ln_mutant(i["h"], i["w"], i["b"], mutant)
    y = O.gelu(ln)
    if frame_scale is not None:
        y = y * frame_scale.to(dtype).reshape(-1, 1, 1)
    if i["res"] is not None:
        y = y + i["res"]
    out = _grads(y, i["cot"], dict(dh=i["h"], dw=i["w"], db=i["b"], dres=i["res"]))
    out["out"] = y.detach()
    return out


def droppath_case():
    d = FRAMELN_DROPPATH
    return (d["frames"], d["P"], d["Ch"], 1, "plain")


# ------------------------------------------------------------------------------------------------------------------- LayerNorm
def layernorm_inputs(case, dtype=torch.float32, seed=None):
    rows, C, relu, kind = case
    s = seed_of("layernorm", case) if seed is None else seed
    return dict(x=_leaf(_field((rows, C), s, kind), dtype), w=_leaf(1 + 0.1 * O.seeded_randn((C,), s + 1), dtype),
                b=_leaf(0.1 * O.seeded_randn((C,), s + 2), dtype), cot=O.seeded_randn((rows, C), s + 3).to(dtype),
                cot_x=O.seeded_randn((rows, C), s + 4).to(dtype))


def layernorm_reference(case, dtype=torch.float64, mutant=None):
    """-> y, dx, dw, db"""
    i = layernorm_inputs(case, dtype)
    if mutant is None:
        y = O.layernorm(i["x"], i["w"], i["b"])
    else:
        mu, rs = _stats(i["x"], (1,), 1e-5, mutant)
        y = (i["x"] - mu) * rs * i["w"] + i["b"]
    y = torch.relu(y) if case[2] else y
    out = _grads(y, i["cot"], dict(dx=i["x"], dw=i["w"], db=i["b"]))
    out["y"] = y.detach()
    return out


def layernorm_res_case():
    return (LAYERNORM_RES[0], LAYERNORM_RES[1], 0, "plain")


def layernorm_res_reference(dtype=torch.float64):
    """(x, LN(x)) with BOTH outputs in the loss <x, cot_x> + <LN(x), cot>: -> x_out, y, dx, dw, db"""
    i = layernorm_inputs(layernorm_res_case(), dtype, SEED["layernorm_res"])
    y = O.layernorm(i["x"], i["w"], i["b"])
    gx, gw, gb = torch.autograd.grad((y * i["cot"]).sum() + (i["x"] * i["cot_x"]).sum(), [i["x"], i["w"], i["b"]])
    return dict(x_out=i["x"].detach(), y=y.detach(), dx=gx, dw=gw, db=gb)


# ------------------------------------------------------------------------------------------------------------------- attention
def attn_temporal_inputs(case, dtype=torch.float32):
    N, P, Tq, Tk, mask, heads = case
    C, s = 64 * heads, seed_of("attn_temporal", case)
    return dict(q=_leaf(O.seeded_randn((N * Tq * P, C), s), dtype), k=_leaf(O.seeded_randn((N * Tk * P, C), s + 1), dtype),
                v=_leaf(O.seeded_randn((N * Tk * P, C), s + 2), dtype), cot=O.seeded_randn((N * Tq * P, C), s + 3).to(dtype))


def attn_temporal_reference(case, dtype=torch.float64, mutant=None):
    """-> y, dq, dk, dv"""
    N, P, Tq, Tk, mask, heads = case
    i = attn_temporal_inputs(case, dtype)
    m = O.encoder_temporal_mask(Tq) if mask else None
    if m is not None and mutant == "mask_transposed":
        m = m.t()
    q = i["q"] * 8.0 if mutant == "q_unscaled" else i["q"]            # (d ** -0.5 = 1 / 8 undone)
    y = O.attn_core(q, i["k"], i["v"], O.temporal_groups(N, Tq, P), O.temporal_groups(N, Tk, P), heads, m)
    out = _grads(y, i["cot"], dict(dq=i["q"], dk=i["k"], dv=i["v"]))
    out["y"] = y.detach()
    return out


def attn_spatial_inputs(case, dtype=torch.float32):
    Fr, H, W, ws = case
    R, C, s = Fr * H * W, 64 * SPATIAL_HEADS, seed_of("attn_spatial", case)
    return dict(qk=_leaf(O.seeded_randn((R, 2 * C), s), dtype), v=_leaf(O.seeded_randn((R, C), s + 1), dtype),
                cot=O.seeded_randn((R, C), s + 2).to(dtype))


def attn_spatial_reference(case, dtype=torch.float64, mutant=None):
    """packed q|k: -> y, dqk, dv"""
    Fr, H, W, ws = case
    C = 64 * SPATIAL_HEADS
    i = attn_spatial_inputs(case, dtype)
    rows = O.spatial_groups(Fr, W, H, ws) if mutant == "grid_swapped" else O.spatial_groups(Fr, H, W, ws)
    q = i["qk"][:, :C] * 8.0 if mutant == "q_unscaled" else i["qk"][:, :C]
    y = O.attn_core(q, i["qk"][:, C:], i["v"], rows, rows, SPATIAL_HEADS, None)
    out = _grads(y, i["cot"], dict(dqk=i["qk"], dv=i["v"]))
    out["y"] = y.detach()
    return out


# ------------------------------------------------------------------------------------------------------------------- dispatch
def reference(family, case, dtype=torch.float64, mutant=None):
    if family.startswith("posfuse"):
        return posfuse_reference(family, case, dtype, mutant)
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
def split_chunks(items, wanted):
    """csrc/partials.h split_chunks: -> (items per chunk, chunks that are not empty)"""
    per = -(-items // wanted)
    return per, -(-items // per)


def frameln_chunks(L, frames, per_frame):
    """(frames per chunk, chunks) of the frame-LN backward: the chunks WANTED are read off the library's workspace query
    (psum [frames][4][2] floats, then [wanted][2 per_frame])"""
    wanted = (L.npvp_frameln_act_bwd_workspace_bytes(frames, per_frame) // 4 - 8 * frames) // (2 * per_frame)
    return split_chunks(frames, wanted)


def dwconv_chunks(L, frames, Ch):
    """the same for the depthwise weight gradient: partials [wanted][10][Ch]"""
    return split_chunks(frames, L.npvp_dwconv3x3_wgrad_workspace_bytes(frames, Ch) // (40 * Ch))


def attn_route(L_, S_):
    """npvp_attn_fwd / npvp_attn_bwd's choice (csrc/attn.hip): 16-row tiles on either side, (nq, nk) up to (2, 2) on the MFMA
    kernels, anything longer (33 .. 128 rows) on the generic ones"""
    nq, nk = -(-L_ // 16), -(-S_ // 16)
    return "generic" if (nq > 2 or nk > 2) else (nq, nk)
