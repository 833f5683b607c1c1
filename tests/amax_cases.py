"""The cases of tests/test_hip_amax_slots.py (GPU) and tests/test_amax_cases_host.py (CPU): every kernel that fills an amax slot
(include/npvp_hip.h: 32 words, 64 bytes apart, the tensor's bound is their maximum), run on inputs with a PLANTED maximum.

A randn tensor's largest element is matched within ~10 % by many others, so a producer that forgets its last rows, its residual add or
its second output still scales a randn tensor correctly.  Here ONE element of the stored output is at least twice every other (one
exponent step: missing it changes amax_scale's power of two), and it sits where a kernel is most likely to leave it out: the first
and the last element, the partial last block, wave 3 of a block, a block >= 32 (whose word wraps onto words 0..31), a row reached only
on the second trip of a grid-stride loop whose grid the launcher caps, and it enters through the operand that is most likely to be
left out of the bound (the residual, dres, the grid cut's addend, beta).

Producers: the norm, elementwise and grid kernels, npvp_amax, the weight splits, c_amax of the GEMMs (every unsplit kernel id x every
epilogue, the split-K reduction) and the attention kernels (o through v; dq, dk, dv through go, v and one column of k / q).

Per producer: a case table, `inputs(case)` (fp32 CPU tensors from oracle.ops.seeded_randn with the maximum planted; `at` = the
planted flat index per output, `keep` for dropout cases = the keep-scales the device drew), `oracle(case, inputs)` = the float64
reference {output name: tensor} of the region the kernel stores.  The host test proves on the CPU that every table plants what it
claims; the GPU test holds the kernels to it.  VALUE_BOUND is the bound of tests/grid_kernel_cases.py (the existing value test of
these kernels): 1e-5 on the whole tensor and on the worst row."""
import math

import torch

from oracle import ops as O

VALUE_BOUND = 1e-5          # tests/grid_kernel_cases.py BOUND
ROW_FLOOR = 1e-6
PAD = 1e30                  # what padding that must not count is filled with (large and finite)
WORDS, STRIDE = 32, 16      # csrc/common.h AMAX_WORDS, AMAX_STRIDE: word i at float offset 16 i of a 512-float slot

# The grid caps of the launchers, restated once (file:line of the launcher each comes from).  A table's `second_trip` case must
# exceed its cap, so that the planted row is reached only after the kernel's grid-stride loop has gone round.
CAPS = {
    "ln_fwd": dict(blocks=4096, rows_per_block=4),            # csrc/norm.hip:898  nb > 4096 ? 4096 : nb, 4 rows per block
    "ln_bwd": dict(blocks=512, rows_per_block=4),             # csrc/norm.hip:905  ln_bwd_blocks: b > 512 ? 512 : b
    "ew_blocks": dict(blocks=4096, float4_per_block=256),     # csrc/norm.hip:863 / csrc/elementwise.hip:175  ew_blocks: b > 4096
    "npvp_amax": dict(blocks=2048, float4_per_block=2048),    # csrc/gemm_f16.hip:784-785  8 float4 per thread, blocks > 2048
    "weights_amax": dict(blocks=16, float4_per_block=256),    # csrc/gemm_f16.hip:813,825  dim3(16, count): always loops
    "gridpad": dict(blocks=2048, rows_per_trip=2),            # csrc/gridpad.hip:105  b > 2048; two rows in flight per thread
}

POSITIONS = ("first", "last", "partial_block", "wave3", "wrap32", "second_trip")


def rel(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-300))


def case_id(case):
    return case["id"]


def _mk(producer, pos, **kw):
    c = dict(producer=producer, pos=pos, **kw)
    c["id"] = producer + "-" + "-".join(f"{k}{v}" for k, v in kw.items() if k not in ("via",)) + "-" + kw.get("via", "x") + "-" + pos
    return c


def _randn(shape, seed):
    return O.seeded_randn(shape, seed)


def _seed(case):
    return 7000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(case["id"])) % 100000


# ------------------------------------------------------------------------------------------------------------------- token LayerNorm
# one wave per row, 4 rows per block, one commit per block.  151 rows: 38 blocks (words wrap from block 32 on), the last block holds
# 3 rows (rows % 4 != 0)
def _ln_row(pos, rows, cap_rows):
    """(row, col index as a fraction) of a planted position of a [rows, C] LayerNorm tensor"""
    return {"first": 0, "last": rows - 1, "partial_block": rows - 2, "wave3": 7, "wrap32": 4 * 35 + 1,
            "second_trip": cap_rows + 4 * 33 + 2}[pos]


def _ln_tables():
    fwd, bwd = [], []
    capf = CAPS["ln_fwd"]["blocks"] * CAPS["ln_fwd"]["rows_per_block"]
    capb = CAPS["ln_bwd"]["blocks"] * CAPS["ln_bwd"]["rows_per_block"]
    for C in (256, 1024):
        for relu in (0, 1):
            for pos in ("first", "last", "partial_block", "wave3", "wrap32"):
                fwd.append(_mk("layernorm_fwd", pos, rows=151, C=C, relu=relu))
        for dres in (0, 1):
            for pos in ("first", "last", "partial_block", "wave3", "wrap32"):
                bwd.append(_mk("layernorm_bwd", pos, rows=151, C=C, dres=dres, via="dres" if dres else "dy"))
            bwd.append(_mk("layernorm_bwd", "second_trip", rows=2 * capb + 3, C=C, dres=dres, via="dres" if dres else "dy"))
    for relu in (0, 1):
        fwd.append(_mk("layernorm_fwd", "second_trip", rows=2 * capf + 3, C=256, relu=relu))
    return fwd, bwd


LAYERNORM_FWD, LAYERNORM_BWD = _ln_tables()


def layernorm_inputs(case):
    rows, C, s = case["rows"], case["C"], _seed(case)
    fwd = case["producer"] == "layernorm_fwd"
    cap = CAPS["ln_fwd" if fwd else "ln_bwd"]
    r = _ln_row(case["pos"], rows, cap["blocks"] * cap["rows_per_block"])
    c = {"first": 0, "last": C - 1}.get(case["pos"], (37 * r + 5) % C)
    x = _randn((rows, C), s)
    w = 1.0 + 0.05 * _randn((C,), s + 1)
    b = 0.1 * _randn((C,), s + 2)
    i = dict(x=x, w=w, b=b, at={("y" if fwd else "dx"): r * C + c})
    if fwd:
        x[r, c] = 1000.0                    # -> y ~ sqrt(C) w[c]
        w[c] = 2.0
        return i
    x64 = x.double()
    mu = x64.mean(-1)
    i["mean"] = mu.float()
    i["rstd"] = torch.rsqrt(((x64 - mu[:, None]) ** 2).mean(-1) + 1e-5).float()
    i["dy"] = _randn((rows, C), s + 3)
    if case["dres"]:
        i["dres"] = _randn((rows, C), s + 4)
        i["dres"][r, c] = 100.0
    else:
        i["dy"][r, c] = 1000.0
    return i


def layernorm_oracle(case, i):
    x, w, b = i["x"].double(), i["w"].double(), i["b"].double()
    if case["producer"] == "layernorm_fwd":
        y = O.layernorm(x, w, b)
        return dict(y=torch.relu(y) if case["relu"] else y)
    # the backward of y = xhat w + b given the SAVED statistics (fp32 values, as the kernel reads them)
    mu, rs = i["mean"].double()[:, None], i["rstd"].double()[:, None]
    xh = (x - mu) * rs
    g = i["dy"].double() * w
    dx = rs * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    if case["dres"]:
        dx = dx + i["dres"].double()
    return dict(dx=dx)


# ------------------------------------------------------------------------------------------------------------------- positional fuse
# npvp_posfuse_fwd (csrc/norm.hip:993): per_frame == 32768 -> posfuse_fwd_frame_kernel (one block of 1024 threads per frame: 16 waves,
# one commit per block); every other per_frame -> frame_stats_kernel + posfuse_apply_kernel (ew_blocks(total4, 256) blocks).
# Through x: a spike in one frame gives ~sqrt(per_frame) there.  Through beta: N = 1, so that beta[t, e] reaches one output element.
def _posfuse_tables():
    t = []
    for pos in ("first", "last", "wave3"):                                       # frame path: 2 x 3 frames of 64 x 512
        t.append(_mk("posfuse_fwd", pos, N=2, T=3, pf=32768, add=1, gamma=1, via="x"))
    t.append(_mk("posfuse_fwd", "last", N=1, T=3, pf=32768, add=0, gamma=0, via="beta"))
    t.append(_mk("posfuse_fwd", "wrap32", N=12, T=3, pf=32768, add=1, gamma=1, via="x"))      # frame 33 -> word 1
    # apply path: 2 x 3 frames of 9 x 48 = 432 (648 float4: 3 blocks, the last partial); 20 x 2 frames of 60 x 20 (12000 float4: 47 blocks)
    for pos in ("first", "last", "partial_block", "wave3"):
        t.append(_mk("posfuse_fwd", pos, N=2, T=3, pf=432, add=1, gamma=1, via="x"))
    t.append(_mk("posfuse_fwd", "last", N=1, T=3, pf=432, add=0, gamma=1, via="beta"))
    t.append(_mk("posfuse_fwd", "wrap32", N=20, T=2, pf=1200, add=1, gamma=0, via="x"))
    cap4 = CAPS["ew_blocks"]["blocks"] * CAPS["ew_blocks"]["float4_per_block"]
    t.append(_mk("posfuse_fwd", "second_trip", N=65, T=2, pf=4 * (2 * cap4 // 130 + 4), add=0, gamma=0, via="x"))
    return t


POSFUSE = _posfuse_tables()
# npvp_ln_posfuse_fwd: frames of 64 rows x 512 channels, TWO slots.  y1 through x (fused's spike is damped by gamma = -0.9 there),
# fused through beta (N = 1; y1 stays a plain LayerNorm output)
LN_POSFUSE = [_mk("ln_posfuse_fwd", pos, N=n, T=3, add=a, gamma=1, via=via)
              for (pos, n, a, via) in (("first", 2, 1, "x"), ("last", 2, 1, "x"), ("wave3", 2, 0, "x"), ("first", 1, 0, "beta"),
                                       ("last", 1, 0, "beta"))] + [_mk("ln_posfuse_fwd", "wrap32", N=12, T=3, add=1, gamma=1, via="x")]
# npvp_posfuse_instance_fwd: grid ((C + 255) / 256, N*T), 256 threads = one channel each.  P = 60; C = 260: a second block with 4 live
# channels.  The statistics run over only P values (a spike gives at most sqrt(P - 1) ~ 7.7), so the maximum comes in through beta
POSFUSE_INSTANCE = [_mk("posfuse_instance_fwd", pos, N=1, T=t, P=60, C=C, add=0, gamma=g, via="beta")
                    for (pos, t, C, g) in (("first", 3, 260, 1), ("last", 3, 260, 1), ("partial_block", 3, 260, 0), ("wave3", 3, 512, 1),
                                           ("wrap32", 20, 260, 0))]


def _pf_elem(case, per_frame, frames):
    """(frame, element) of the planted position"""
    pos = case["pos"]
    if pos == "first":
        return 0, 0
    if pos == "last":
        return frames - 1, per_frame - 1
    if pos == "wave3":                     # frame kernel: 1024 threads, thread t holds float4 t, t + 1024, ...; apply: float4 200 of block 0
        return (1, 4 * (3 * 64 + 5) + 2) if per_frame > 4 * 256 else divmod(4 * 200 + 1, per_frame)
    if pos == "partial_block":             # the last block of the apply kernel holds total4 % 256 float4
        return frames - 1, per_frame - 9
    if pos == "wrap32":
        return 33, per_frame // 3
    if pos == "second_trip":
        cap4 = CAPS["ew_blocks"]["blocks"] * CAPS["ew_blocks"]["float4_per_block"]
        f = (cap4 * 4) // per_frame + 2
        return f, per_frame // 5
    raise KeyError(pos)


def posfuse_inputs(case):
    N, T, s = case["N"], case["T"], _seed(case)
    ln = case["producer"] == "ln_posfuse_fwd"
    pf = 64 * 512 if ln else case["pf"]
    frames = N * T
    f, e = _pf_elem(case, pf, frames)
    x = 0.5 + _randn((frames, pf), s)
    i = dict(x=x, add=0.3 * _randn((N, pf), s + 1) if case["add"] else None, beta=0.2 * _randn((T, pf), s + 2),
             gamma=0.1 * _randn((T, pf), s + 3) if case["gamma"] else None)
    if ln:
        i["lw"], i["lb"] = 1.0 + 0.05 * _randn((512,), s + 4), 0.1 * _randn((512,), s + 5)
    if case["via"] == "beta":
        assert N == 1
        i["beta"][f % T, e] = 200.0
        i["at"] = {("fused" if ln else "y"): f * pf + e}
    elif ln:
        x[f, e] = 1000.0                   # row f*64 + e/512, column e%512: y1 ~ sqrt(512) lw
        i["lw"][e % 512] = 2.0
        i["gamma"][f % T, e] = -0.9        # ... and fused keeps a tenth of it
        i["at"] = {"y1": f * pf + e}
    else:
        x[f, e] = 1000.0 * math.sqrt(pf / 432.0)
        i["at"] = {"y": f * pf + e}
    return i


def posfuse_oracle(case, i):
    N, T = case["N"], case["T"]
    d = lambda t: None if t is None else t.double()
    if case["producer"] == "ln_posfuse_fwd":
        y1 = O.layernorm(i["x"].double().reshape(-1, 512), i["lw"].double(), i["lb"].double())
        fused = O.posfuse(y1.reshape(N * T, 64, 512), T, d(i["beta"]), d(i["gamma"]), None if i["add"] is None else d(i["add"]).reshape(N, 64, 512))
        return dict(y1=y1.reshape(N * T, -1), fused=fused.reshape(N * T, -1))
    pf = case["pf"]
    y = O.posfuse(i["x"].double().reshape(N * T, 1, pf), T, d(i["beta"]), d(i["gamma"]), None if i["add"] is None else d(i["add"]).reshape(N, 1, pf))
    return dict(y=y.reshape(N * T, pf))


def posfuse_instance_inputs(case):
    N, T, P, C, s = case["N"], case["T"], case["P"], case["C"], _seed(case)
    frames = N * T
    f, p, c = {"first": (0, 0, 0), "last": (frames - 1, P - 1, C - 1), "partial_block": (1, P // 2, C - 2), "wave3": (1, 7, 3 * 64 + 9),
               "wrap32": (17, 11, 41)}[case["pos"]]          # wrap32: block (0, 17) of a 2 x 20 grid
    i = dict(x=0.5 + _randn((frames, P, C), s), add=None, beta=0.2 * _randn((T, P, C), s + 2),
             gamma=0.1 * _randn((T, P, C), s + 3) if case["gamma"] else None)
    i["beta"][f % T, p, c] = 200.0
    i["at"] = {"y": (f * P + p) * C + c}
    return i


def posfuse_instance_oracle(case, i):
    y = O.posfuse(i["x"].double(), case["T"], i["beta"].double(), None if i["gamma"] is None else i["gamma"].double(), None, norm="instance")
    return dict(y=y.reshape(case["N"] * case["T"], -1))


# ------------------------------------------------------------------------------------------------------------------- frame LayerNorm + GELU
# forward: ew_blocks(total4, 256); forward from partials: one block per 4096 elements; backward: grid ((per_frame / 4 + 255) / 256,
# fln_chunks(frames)), thread = 4 elements of the frame, loop over a chunk's frames.  per_frame = 1312: 328 float4, the second block
# has 72 live threads - wave 1 of it is PARTIAL (8 live lanes) and waves 2, 3 take the early-commit branch (csrc/norm.hip:726)
def _fln_tables():
    fwd, parts, bwd, apply_ = [], [], [], []
    for res in (0, 1):
        via = "res" if res else "h"
        for pos in ("first", "last", "partial_block", "wave3"):
            fwd.append(_mk("frameln_act_fwd", pos, frames=3, pf=1312, res=res, drop=0, dp=0, via=via))
        fwd.append(_mk("frameln_act_fwd", "wrap32", frames=34, pf=1312, res=res, drop=0, dp=0, via=via))
    cap4 = CAPS["ew_blocks"]["blocks"] * CAPS["ew_blocks"]["float4_per_block"]
    fwd.append(_mk("frameln_act_fwd", "second_trip", frames=66, pf=4 * (2 * cap4 // 66 + 4), res=1, drop=0, dp=0, via="res"))
    for (res, drop, dp) in ((0, 1, 0), (1, 0, 1), (0, 1, 1)):
        fwd.append(_mk("frameln_act_fwd", "last", frames=8, pf=1312, res=res, drop=drop, dp=dp, via="res" if res else "h"))
    for pos, frames in (("first", 3), ("last", 3), ("wave3", 3), ("wrap32", 18)):            # 2 blocks per frame: frame 16 -> blocks 32, 33
        parts.append(_mk("frameln_act_fwd_parts", pos, frames=frames, pf=8192, res=1, drop=0, dp=0, via="res"))
    parts.append(_mk("frameln_act_fwd_parts", "last", frames=3, pf=8192, res=0, drop=0, dp=0, via="h"))
    for table, name in ((bwd, "frameln_act_bwd"), (apply_, "frameln_act_bwd_apply")):
        for pos in ("first", "last", "partial_block", "wave3"):
            table.append(_mk(name, pos, frames=5, pf=1312, res=0, drop=0, dp=0, via="dout"))
        # 40 float4-blocks of 256 x 2 chunks: blockIdx.x runs to 39 (the commit word is blockIdx.x)
        table.append(_mk(name, "wrap32", frames=5, pf=4 * (39 * 256 + 72), res=0, drop=0, dp=0, via="dout"))
    bwd.append(_mk("frameln_act_bwd", "last", frames=8, pf=1312, res=0, drop=1, dp=1, via="dout"))
    return fwd, parts, bwd, apply_


FRAMELN_FWD, FRAMELN_FWD_PARTS, FRAMELN_BWD, FRAMELN_BWD_APPLY = _fln_tables()
FLN_DROP_P, FLN_DP_P, FLN_FRAMES_PER_SAMPLE = 0.25, 0.25, 2
FLN_PARTS_NB = 2048.0          # values per statistics partial of the _parts case (J = per_frame / nb)


def _fln_elem(case):
    frames, pf, pos = case["frames"], case["pf"], case["pos"]
    if pos == "first":
        return 0, 0
    if pos == "last":
        return frames - 1, pf - 1
    fwd = case["producer"] == "frameln_act_fwd"
    if pos == "partial_block":             # forward: the last block of the flat walk; backward: a live lane of the last block's partial wave
        return (frames - 1, pf - 18) if fwd else (frames - 2, pf - 6)
    if pos == "wave3":                     # forward: float4 456 = thread 200 of block 1; the others: thread 209 of a frame's first block
        return (1, 4 * (456 - pf // 4) + 1) if fwd else (1, 4 * (3 * 64 + 17) + 1)
    if pos == "wrap32":
        if case["producer"] == "frameln_act_fwd":
            return 33, pf // 3                                # block 33 * 328 / 256 = 42
        if case["producer"] == "frameln_act_fwd_parts":
            return 16, 4096 + 4 * 77 + 3                        # block 16 * 2 + 1 = 33
        return 3, 4 * (37 * 256 + 100) + 2                      # blockIdx.x = 37
    if pos == "second_trip":
        cap4 = CAPS["ew_blocks"]["blocks"] * CAPS["ew_blocks"]["float4_per_block"]
        return (cap4 * 4) // pf + 3, pf // 7
    raise KeyError(pos)


def frameln_inputs(case, keep=None):
    """keep (dropout cases): {"drop": keep-scale per element [frames, pf] or None, "dp": per frame [frames] or None} as the device
    draws them; the planted element moves to the next one both masks keep"""
    frames, pf, s = case["frames"], case["pf"], _seed(case)
    f, e = _fln_elem(case)
    if keep is not None and case["via"] != "res":
        alive = torch.ones(frames, pf)
        if keep.get("drop") is not None:
            alive = alive * keep["drop"].reshape(frames, pf).cpu()
        if keep.get("dp") is not None:
            alive = alive * keep["dp"].reshape(frames, 1).cpu()
        flat = (alive.flatten() != 0).nonzero().flatten()
        idx = flat[flat <= f * pf + e][-1].item()              # the last kept element at or before the nominal position
        f, e = divmod(idx, pf)
    h = 0.5 + _randn((frames, pf), s)
    i = dict(h=h, w=1.0 + 0.05 * _randn((pf,), s + 1), b=0.1 * _randn((pf,), s + 2),
             res=_randn((frames, pf), s + 3) if case["res"] else None, keep=keep)
    h64 = None
    name = case["producer"]
    if name in ("frameln_act_fwd", "frameln_act_fwd_parts"):
        if case["via"] == "res":
            i["res"][f, e] = 100.0
        else:
            h[f, e] = 1000.0 * math.sqrt(pf / 1312.0)           # gelu(sqrt(pf) w) = sqrt(pf) w
        i["at"] = {"out": f * pf + e}
    else:
        h[f, e] = h[f].mean() + h[f].std()                      # y ~ 1: gelu'(1) = 1.08
        i["dout"] = _randn((frames, pf), s + 4)
        i["dout"][f, e] = 1000.0
        i["at"] = {"dh": f * pf + e}
    h64 = h.double()
    mu = h64.mean(-1)
    var = ((h64 - mu[:, None]) ** 2).mean(-1)
    i["mean"], i["rstd"] = mu.float(), torch.rsqrt(var + 1e-5).float()
    if name == "frameln_act_fwd_parts":
        J = int(pf / FLN_PARTS_NB)
        hp = h64.reshape(frames, J, -1)
        pm = hp.mean(-1)
        i["part"] = torch.stack([pm, ((hp - pm[..., None]) ** 2).sum(-1)], -1).float().contiguous()      # [frames][J][(mean_j, M2_j)]
    if name == "frameln_act_bwd_apply":
        # psum [frames][nparts = 2][2] = partial (sum g, sum g hhat) of the two halves of each frame
        xh, g = _fln_g(case, i)
        half = pf // 2
        i["psum"] = torch.stack([torch.stack([g[:, :half].sum(-1), (g * xh)[:, :half].sum(-1)], -1),
                                 torch.stack([g[:, half:].sum(-1), (g * xh)[:, half:].sum(-1)], -1)], 1).float().contiguous()
    return i


def _fln_scale(case, i):
    frames, pf = case["frames"], case["pf"]
    sc = torch.ones(frames, pf, dtype=torch.float64)
    k = i.get("keep")
    if k:
        if k.get("drop") is not None:
            sc = sc * k["drop"].reshape(frames, pf).double().cpu()
        if k.get("dp") is not None:
            sc = sc * k["dp"].reshape(frames, 1).double().cpu()
    return sc


def _gelu_grad(y):
    return 0.5 * (1.0 + torch.erf(y / math.sqrt(2.0))) + y * torch.exp(-0.5 * y * y) / math.sqrt(2.0 * math.pi)


def _fln_g(case, i):
    """xhat and g = dout * keep-scale * gelu'(y) * w from the SAVED statistics"""
    xh = (i["h"].double() - i["mean"].double()[:, None]) * i["rstd"].double()[:, None]
    w = i["w"].double()
    y = xh * w + i["b"].double()
    return xh, i["dout"].double() * _fln_scale(case, i) * _gelu_grad(y) * w


def frameln_oracle(case, i):
    name = case["producer"]
    if name == "frameln_act_fwd_parts":
        # the statistics the kernel merges from the fp32 partials (csrc/common.h frame_stats_merge)
        p = i["part"].double()
        J = p.shape[1]
        m = p[..., 0].mean(-1)
        m2 = (p[..., 1] + FLN_PARTS_NB * (p[..., 0] - m[:, None]) ** 2).sum(-1)
        mu, rs = m, torch.rsqrt(m2 / (FLN_PARTS_NB * J) + 1e-5)
    else:
        mu, rs = i["mean"].double(), i["rstd"].double()
    if name in ("frameln_act_fwd", "frameln_act_fwd_parts"):
        xh = (i["h"].double() - mu[:, None]) * rs[:, None]
        out = O.gelu(xh * i["w"].double() + i["b"].double()) * _fln_scale(case, i)
        if i["res"] is not None:
            out = out + i["res"].double()
        return dict(out=out)
    xh, g = _fln_g(case, i)
    if name == "frameln_act_bwd_apply":                      # the statistics come in as fp32 partial sums
        ps = i["psum"].double().sum(1) / case["pf"]
        s1, s2 = ps[:, :1], ps[:, 1:]
    else:
        s1, s2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    return dict(dh=rs[:, None] * (g - s1 - xh * s2))


# ------------------------------------------------------------------------------------------------------------------- elementwise, grid
# npvp_drop_apply: ew_blocks(rows * ncols / 4, 256).  37 x 260: 2405 float4 = 10 blocks, the last with 101 live threads;
# 140 x 260: 36 blocks.  mode 0: one decision per element; mode 1: per row group (row / g1) % g2
def _drop_tables():
    t = []
    for mode in (0, 1):
        for pos in ("first", "last", "partial_block", "wave3"):
            t.append(_mk("drop_apply", pos, rows=37, cols=260, mode=mode))
        t.append(_mk("drop_apply", "wrap32", rows=140, cols=260, mode=mode))
    cap4 = CAPS["ew_blocks"]["blocks"] * CAPS["ew_blocks"]["float4_per_block"]
    t.append(_mk("drop_apply", "second_trip", rows=2 * cap4 // 256 + 5, cols=1024, mode=0))
    return t


DROP_APPLY = _drop_tables()
DROP_P, DROP_G1, DROP_G2 = 0.3, 4, 1 << 20


def drop_inputs(case, keep=None):
    rows, cols, pos = case["rows"], case["cols"], case["pos"]
    n = rows * cols
    cap4 = CAPS["ew_blocks"]["blocks"] * CAPS["ew_blocks"]["float4_per_block"]
    idx = {"first": 0, "last": n - 1, "partial_block": n - 4 * 50 - 2, "wave3": 4 * (256 + 3 * 64 + 20) + 3, "wrap32": 4 * (34 * 256 + 9),
           "second_trip": 4 * (cap4 + 33 * 256 + 70) + 1}[pos]
    if keep is not None:
        flat = (keep.flatten().cpu() != 0).nonzero().flatten()
        idx = flat[flat <= idx][-1].item() if bool((flat <= idx).any()) else flat[0].item()
    x = _randn((rows, cols), _seed(case))
    x.view(-1)[idx] = 100.0
    return dict(x=x, keep=keep, at={"out": idx})


def drop_oracle(case, i):
    return dict(out=i["x"].double() * (1.0 if i["keep"] is None else i["keep"].double().cpu().reshape(i["x"].shape)))


# grid pad / cut (F, H, W, Hp, Wp, top, left, C, extra trailing rows): 256 >> lg rows per block, lg = log2 of the lanes per row.
# C = 48: 12 float4 -> 16 lanes, 16 rows per block.  6 x 10 -> 8 x 12 (top 1, left 1) is the centre pad of tests/window_pad_cases.py
def _grid_tables():
    pad, cut = [], []
    small = dict(F=3, H=6, W=10, Hp=8, Wp=12, top=1, left=1, C=48)
    for pos in ("first", "last", "partial_block", "wave3"):
        pad.append(_mk("grid_center_pad", pos, tail=5, **small))
        cut.append(_mk("grid_center_cut", pos, addend=1, via="addend", **small))
    cut.append(_mk("grid_center_cut", "last", addend=0, via="src", **small))
    wide = dict(F=12, H=6, W=10, Hp=8, Wp=12, top=1, left=1, C=48)                 # 1152 / 720 rows: 72 / 45 blocks of 16 rows
    pad.append(_mk("grid_center_pad", "wrap32", tail=0, **wide))
    cut.append(_mk("grid_center_cut", "wrap32", addend=1, via="addend", **wide))
    # second trip: 2048 blocks x 1 row (C = 1024: 256 lanes) x 2 rows in flight = 4096 rows per trip
    big = dict(F=72, H=6, W=10, Hp=8, Wp=12, top=1, left=1, C=1024)                # 6912 padded / 4320 centre rows
    pad.append(_mk("grid_center_pad", "second_trip", tail=3, **big))
    cut.append(_mk("grid_center_cut", "second_trip", addend=1, via="addend", **big))
    return pad, cut


GRID_PAD, GRID_CUT = _grid_tables()


def _grid_rows(case):
    return case["F"] * case["H"] * case["W"], case["F"] * case["Hp"] * case["Wp"]


def _centre_index(case):
    """padded row of every centre row, in centre-row order"""
    F, H, W, Hp, Wp, top, left = (case[k] for k in ("F", "H", "W", "Hp", "Wp", "top", "left"))
    f = torch.arange(F).view(F, 1, 1)
    y = torch.arange(H).view(1, H, 1)
    x = torch.arange(W).view(1, 1, W)
    return (f * Hp * Wp + (y + top) * Wp + (x + left)).reshape(-1)


def grid_inputs(case):
    inner, outer = _grid_rows(case)
    C, pos, s = case["C"], case["pos"], _seed(case)
    centre = _centre_index(case)
    lanes = min(256, 1 << max(0, math.ceil(math.log2(C // 4))))
    rpb = 256 // lanes
    trip = CAPS["gridpad"]["blocks"] * rpb * CAPS["gridpad"]["rows_per_trip"]
    if case["producer"] == "grid_center_pad":
        # planted in a SOURCE row; the position names where its padded row lies
        src = _randn((inner, C), s)
        want = {"first": 0, "last": inner - 1, "partial_block": inner - 2, "wave3": None, "wrap32": None, "second_trip": None}[pos]
        if want is None:
            lo = {"wave3": 3 * (rpb // 4), "wrap32": 33 * rpb, "second_trip": trip + 33 * rpb}[pos]
            want = int((centre >= lo).nonzero()[0])
        col = {"first": 0, "last": C - 1}.get(pos, C // 2 + 1)
        src[want, col] = 100.0
        return dict(src=src, at={"dst": int(centre[want]) * C + col})
    srcp = _randn((outer, C), s)
    keepm = torch.zeros(outer, dtype=torch.bool)
    keepm[centre] = True
    srcp[~keepm] = PAD                        # the border rows are cut away: they must not count
    r = {"first": 0, "last": inner - 1, "partial_block": inner - 3, "wave3": 3 * (rpb // 4) + 1, "wrap32": 34 * rpb + 2,
         "second_trip": trip + 35 * rpb}[pos]
    col = {"first": 0, "last": C - 1}.get(pos, C // 2 + 1)
    i = dict(src=srcp, addend=_randn((inner, C), s + 1) if case["addend"] else None)
    if case["via"] == "addend":
        i["addend"][r, col] = 100.0
    else:
        srcp[centre[r], col] = 100.0
    i["at"] = {"dst": r * C + col}
    return i


def grid_oracle(case, i):
    inner, outer = _grid_rows(case)
    centre = _centre_index(case)
    if case["producer"] == "grid_center_pad":
        dst = torch.zeros(outer + case["tail"], case["C"], dtype=torch.float64)
        dst[centre] = i["src"].double()
        return dict(dst=dst)
    dst = i["src"].double()[centre]
    return dict(dst=dst if i["addend"] is None else dst + i["addend"].double())


# ------------------------------------------------------------------------------------------------------------------- npvp_amax
# blocks = ceil(n4 / 2048) up to 2048, 256 threads.  Strided: the columns [cols, ld) hold PAD and must not count
def _amax_tables():
    t = []
    for ld in (260, 264):
        for pos in ("first", "last", "wave3"):
            t.append(_mk("amax", pos, rows=37, cols=260, ld=ld))
        t.append(_mk("amax", "wrap32", rows=136, cols=2048, ld=2048 + 4 * (ld - 260)))           # 69632 float4: 34 blocks
    cap = CAPS["npvp_amax"]
    t.append(_mk("amax", "second_trip", rows=cap["blocks"] * cap["float4_per_block"] // 1024 + 16, cols=4096, ld=4096))
    return t


AMAX = _amax_tables()


def amax_inputs(case):
    rows, cols, ld, pos = case["rows"], case["cols"], case["ld"], case["pos"]
    x = torch.full((rows, ld), PAD)
    x[:, :cols] = _randn((rows, cols), _seed(case))
    n4 = rows * cols // 4
    nb = min(CAPS["npvp_amax"]["blocks"], (n4 + 2047) // 2048)
    q = {"first": 0, "last": n4 - 1, "wave3": 3 * 64 + 11, "wrap32": min(n4 - 1, 33 * 256 + 5),
         "second_trip": nb * 256 * 8 + 35 * 256 + 7}[pos]      # float4 index: thread q % (nb * 256), trip q / (nb * 256)
    q = min(q, n4 - 1)
    r, c = divmod(4 * q + (3 if pos == "last" else 1), cols)
    x[r, c] = -100.0
    return dict(x=x, at={"x": r * cols + c})


def amax_oracle(case, i):
    return dict(x=i["x"][:, :case["cols"]].double())


# ------------------------------------------------------------------------------------------------------------------- weight splits
# weights_amax_kernel: dim3(16, count) blocks of 256 threads - 4096 float4 per trip, so a [64, 512] weight (8192 float4) loops twice.
# Both entry points ZERO the slot first: a slot pre-filled above the maximum must come back as the exact new maximum.
SPLIT_WEIGHT = [_mk("split_weight_f16", pos, N=64, K=512, ld=ld) for ld in (512, 520) for pos in ("first", "last", "wave3", "second_trip")]
# three records (N, K, ld); the spike in the last row of the last record; the table of the three slots is handed over
SPLIT_WEIGHTS = [_mk("split_weights_f16", pos, records="64x512,128x64,72x264") for pos in ("last", "second_trip")]
SPLIT_RECORDS = ((64, 512, 512), (128, 64, 72), (72, 264, 264))


def split_inputs(case):
    s = _seed(case)
    if case["producer"] == "split_weight_f16":
        recs = ((case["N"], case["K"], case["ld"]),)
    else:
        recs = SPLIT_RECORDS
    ws = []
    for j, (N, K, ld) in enumerate(recs):
        w = torch.full((N, ld), PAD)
        w[:, :K] = 0.05 * (j + 1) * _randn((N, K), s + j)
        ws.append(w)
    N, K, ld = recs[-1]
    n4 = N * K // 4
    q = {"first": 0, "last": n4 - 1, "wave3": 3 * 64 + 11, "second_trip": (n4 - (K // 4) + 3) if len(recs) > 1 else 4096 + 33 * 64}[case["pos"]]
    r, c = divmod(4 * q + (3 if case["pos"] == "last" else 2), K)
    ws[-1][r, c] = 3.0
    return dict(w=ws, recs=recs, at={f"w{len(recs) - 1}": r * K + c})


def split_oracle(case, i):
    return {f"w{j}": w[:, :K].double() for j, (w, (N, K, ld)) in enumerate(zip(i["w"], i["recs"]))}


# ------------------------------------------------------------------------------------------------------------------- GEMM c_amax
# npvp_gemm_f32's c_amax, every kernel id an unsplit launch can take (0, 1, 2, 4, 5, 7), at the smallest shape tests/gemm_route_cases.py
# holds for it, crossed with the epilogues.  The planted element is the LAST valid one (M - 1, N - 1): the last row / quad of an edge
# tile wherever the shape is ragged (the CHECK epilogue).  C lives in a buffer with ldc = N + 8 whose padding holds 1e30.
GEMM_SHAPES = {0: "f32 fwd ragged", 1: "db3 fwd no planes under f16x3", 2: "wide v1 fwd ragged", 4: "wide v2 fwd ragged rows",
               5: "f16 v1 fwd ragged", 7: "f16 v3 dgrad 260 rows"}
# the operand the maximum comes in through: the product itself (one row of A with a single entry, against a large weight entry),
# the product + bias, the residual, the base of an accumulating launch
GEMM_EPILOGUES = {"gelu_aux": "bias", "act3": "product", "dropout": "product", "droppath": "product", "residual": "residual",
                  "accumulate": "base"}
# rowstats (bias-only epilogue, M % 64 == 0, N % 128 == 0) has shapes of its own in the route table
GEMM_ROWSTATS = {1: "db3 rowstats 1025 frames", 2: "wide v1 rowstats 97 frames", 4: "wide v2 rowstats 5 frames",
                 5: "f16 v1 rowstats ragged columns", 7: "f16 128x128 rowstats 5 frames"}
GEMM_SPLIT = ("db3 wgrad 5 splits", "wgrad f16 3 x 22 ragged")         # the split-K reduce kernel commits the slot
GEMM_DROP_P, GEMM_DP_G1 = 0.25, 4
LDC_PAD = 8


def _route_case(name):
    import gemm_route_cases as T
    (c,) = [c for c in T.CASES if c["name"] == name]
    return c


def _gemm_tables():
    t = []
    for kid, name in GEMM_SHAPES.items():
        for ep, via in GEMM_EPILOGUES.items():
            t.append(_mk("gemm", "last", kid=kid, ep=ep, via=via, shape=name))
    for kid, name in GEMM_ROWSTATS.items():
        t.append(_mk("gemm", "last", kid=kid, ep="rowstats", via="bias", shape=name))
    for name in GEMM_SPLIT:
        t.append(_mk("gemm", "last", kid=_route_case(name)["route"][0], ep="split", via="product", shape=name))
        t.append(_mk("gemm", "first", kid=_route_case(name)["route"][0], ep="split_accumulate", via="base", shape=name))
    return t


GEMM = _gemm_tables()


def gemm_inputs(case, keep=None):
    """A [M, K] (wgrad: dy [K, M]), W (fwd [N, K], dgrad [K, N], wgrad: x [K, N]) and the epilogue's operands"""
    rc = _route_case(case["shape"])
    M, N, Kk, role, ep, s = rc["M"], rc["N"], rc["K"], rc["role"], case["ep"], _seed(case)
    r, c = (0, 0) if case["pos"] == "first" else (M - 1, N - 1)
    if keep is not None:
        alive = (keep.cpu() != 0)
        rows_alive = alive.any(1).nonzero().flatten()
        r = int(rows_alive[-1])
        c = int(alive[r].nonzero().flatten()[-1])
    i = dict(role=role, M=M, N=N, K=Kk, mode=rc["mode"], planes=rc["planes"], keep=keep, at={"C": r * N + c})
    k0 = Kk // 2 + 1
    if role == "wgrad":
        A, W = _randn((Kk, M), s), _randn((Kk, N), s + 1)
        if case["via"] == "product":
            A[k0, r], W[k0, c] = 64.0, 64.0
    else:
        A = _randn((M, Kk), s)
        W = _randn((N, Kk) if role == "fwd" else (Kk, N), s + 1) / math.sqrt(Kk)
        if case["via"] in ("product", "bias"):
            A[r] = 0.0
            A[r, k0] = 16.0
            if role == "fwd":
                W[c, k0] = 4.0
            else:
                W[k0, c] = 4.0
    i["A"], i["W"] = A, W
    if ep in ("gelu_aux", "rowstats"):
        i["bias"] = _randn((N,), s + 2)
        i["bias"][c] = 3.0
    if ep == "act3":
        i["aux_in"] = _randn((M, N), s + 3)
        i["aux_in"][r, c] = 1.0
    if ep == "residual":
        i["residual"] = _randn((M, N), s + 4)
        i["residual"][r, c] = 100.0
    if ep in ("accumulate", "split_accumulate"):
        i["base"] = _randn((M, N), s + 5)
        i["base"][r, c] = 100.0 if ep == "accumulate" else 2.0e4
    return i


def gemm_oracle(case, i):
    A, W = i["A"].double(), i["W"].double()
    ref = A.T @ W if i["role"] == "wgrad" else (A @ W.T if i["role"] == "fwd" else A @ W)
    ep = case["ep"]
    out = {}
    if "bias" in i:
        ref = ref + i["bias"].double()
    if ep == "gelu_aux":
        out["aux_out"] = ref
        ref = O.gelu(ref)
    if ep == "act3":
        ref = ref * _gelu_grad(i["aux_in"].double())
    if i.get("keep") is not None:
        ref = ref * i["keep"].double().cpu()
    if "residual" in i:
        ref = ref + i["residual"].double()
    if "base" in i:
        ref = ref + i["base"].double()
    out["C"] = ref
    return out


# ------------------------------------------------------------------------------------------------------------------- attention
# Every kernel csrc/attn.hip launches, by the launcher's conditions (csrc/attn.hip:964-977, 998-1014): nq = ceil(L / 16), nk = ceil(S / 16);
# nq > 2 or nk > 2 -> the generic pair; else forward attn_fwd_mfma_kernel<nq, nk>, backward attn_bwd_mfma_kernel<1, nk> for nq == 1 and
# attn_bwd_staged1_kernel<2, nk> for nq == 2; npvp_attn_long_* -> the streaming trio (fwd, bwd_q, bwd_kv), tiles of 64 rows.
# Temporal shapes: N = 1, P = 9, 3 heads -> 27 (group, head) pairs, no multiple of 4 (the MFMA kernels run 4 per block).
# (mode, dim0, P, W, ws, Tq, Tk, heads, long)
ATTN_SHAPES = {
    "mfma11": (1, 1, 9, 3, 0, 5, 5, 3, 0),            # L = S = 5: fwd<1,1>, bwd_mfma<1,1>
    "mfma12": (1, 1, 9, 3, 0, 5, 20, 3, 0),           # L = 5, S = 20: fwd<1,2>, bwd_mfma<1,2>
    "staged21": (1, 1, 9, 3, 0, 20, 5, 3, 0),         # L = 20, S = 5: fwd<2,1>, bwd_staged1<2,1>
    "staged22": (1, 1, 9, 3, 0, 20, 20, 3, 0),        # L = S = 20: fwd<2,2>, bwd_staged1<2,2>
    "generic40x33": (1, 1, 9, 3, 0, 40, 33, 3, 0),    # nq = nk = 3: the generic pair at its lower edge
    "generic100x128": (1, 1, 9, 3, 0, 100, 128, 3, 0),    # ... at its upper edge, Tq != Tk
    "long65": (1, 1, 9, 3, 0, 65, 65, 3, 1),          # two tiles of 64, the second with ONE row
    "long129": (1, 1, 9, 3, 0, 129, 129, 3, 1),       # three tiles
    "spatial4": (0, 2, 64, 8, 4, 0, 0, 8, 0),         # ws 4: L = S = 16 -> fwd<1,1>, bwd_mfma<1,1>; 2 frames x 4 windows x 8 heads
    "spatial8": (0, 2, 64, 8, 8, 0, 0, 8, 0),         # ws 8: L = S = 64 -> the generic pair
    "spatial8long": (0, 2, 64, 8, 8, 0, 0, 8, 1),     # the same window through the streaming kernels
}
ATTN_DROP_P = 0.2
ATTN_PAD_ROWS = 8                                     # rows of q, k, v (and go) beyond the sequence: 1e30, must not count


def _attn_tables():
    fwd, bwd = [], []
    for name, sh in ATTN_SHAPES.items():
        square = sh[0] == 1 and sh[5] == sh[6]
        fwd.append(_mk("attn_fwd", "last", shape=name, mask=0, drop=0, via="v"))
        fwd.append(_mk("attn_fwd", "first", shape=name, mask=0, drop=0, via="v"))
        fwd.append(_mk("attn_fwd", "last", shape=name, mask=0, drop=1, via="v"))
        for tgt in ("dq", "dk", "dv"):
            bwd.append(_mk("attn_bwd", "last", shape=name, mask=0, drop=0, via=tgt))
        bwd.append(_mk("attn_bwd", "first", shape=name, mask=0, drop=0, via="dv"))
        bwd.append(_mk("attn_bwd", "last", shape=name, mask=0, drop=1, via="dv"))
        bwd.append(_mk("attn_bwd", "last", shape=name, mask=0, drop=1, via="dq"))
        if square:                                   # the encoder's mask: every query but the last may not see the last time step
            fwd.append(_mk("attn_fwd", "last", shape=name, mask=1, drop=0, via="v"))
            bwd.append(_mk("attn_bwd", "last", shape=name, mask=1, drop=0, via="dq"))
            bwd.append(_mk("attn_bwd", "last", shape=name, mask=1, drop=0, via="dv"))
    return fwd, bwd


ATTN_FWD, ATTN_BWD = _attn_tables()


def attn_geometry(case):
    """-> (q_rows [G, L], k_rows [G, S], rows of q, rows of k / v, heads, mask [L, S] or None)"""
    mode, dim0, P, W, ws, Tq, Tk, heads, _ = ATTN_SHAPES[case["shape"]]
    if mode == 0:
        g = O.spatial_groups(dim0, P // W, W, ws)
        return g, g, dim0 * P, dim0 * P, heads, None
    mask = None
    if case["mask"]:
        assert Tq == Tk
        mask = O.encoder_temporal_mask(Tq)
    return O.temporal_groups(dim0, Tq, P), O.temporal_groups(dim0, Tk, P), dim0 * Tq * P, dim0 * Tk * P, heads, mask


def attn_keep_shape(case):
    qr, kr, _, _, heads, _ = attn_geometry(case)
    return (qr.shape[0], heads, qr.shape[1], kr.shape[1])       # the dropout key is the flat index of the [G, heads, L, S] weights


def attn_inputs(case, keep=None):
    qr, kr, nq_rows, nk_rows, heads, mask = attn_geometry(case)
    G, L = qr.shape
    S = kr.shape[1]
    C, s = heads * 64, _seed(case)
    g, h, l, j = (0, 0, 0, 0) if case["pos"] == "first" else (G - 1, heads - 1, L - 1, S - 1)
    if keep is not None:               # the last query row of the planted (group, head) that keeps the planted key
        alive = (keep.reshape(G, heads, L, S)[g, h, :, j].cpu() != 0).nonzero().flatten()
        cand = alive[alive <= l]
        l = int(cand[-1]) if len(cand) else int(alive[0])
        if mask is not None and l != L - 1:
            j = S - 2 if j == S - 1 else j
    rq, rk = int(qr[g, l]), int(kr[g, j])
    hc = slice(h * 64, (h + 1) * 64)
    c1, c2 = h * 64 + 63, h * 64 + 1
    pad = ATTN_PAD_ROWS
    q, k, v = (torch.full((n + pad, C), PAD) for n in (nq_rows, nk_rows, nk_rows))
    q[:nq_rows], k[:nk_rows], v[:nk_rows] = 0.3 * _randn((nq_rows, C), s), 0.5 * _randn((nk_rows, C), s + 1), _randn((nk_rows, C), s + 2)
    i = dict(q=q, k=k, v=v, keep=keep)
    tgt = case["via"]
    if case["producer"] == "attn_bwd":
        go = torch.full((nq_rows + pad, C), PAD)
        go[:nq_rows] = _randn((nq_rows, C), s + 3)
        go[rq, c1] = 100.0
        i["go"] = go
    if tgt == "v":
        q[rq, hc], k[rk, hc] = 6.0, 0.5            # score 24 above the rest: query rq reads key rk alone, nobody else prefers it
        v[rk, c1] = 100.0
        i["at"] = {"o": rq * C + c1}
    elif tgt == "dv":
        # score 3 above the rest: p[rq, rk] is 20 x every other weight of the row, so dv[rk, c1] = p[rq, rk] go[rq, c1] stands alone.  (Not
        # the one-hot row of the forward case: with p = 1 the softmax gradient p (dp - sum p dp) cancels two values of ~100 and the other
        # gradients of that row would be fp32 noise - a fault of the case, not of a kernel.)
        q[rq, hc], k[rk, hc] = 0.75, 0.5
        i["at"] = {"dv": rk * C + c1}
    elif tgt == "dq":
        v[rk, c1] = 10.0
        q[:nq_rows, c2] = 0.0                      # the scores do not see column c2 ...
        k[rk, c2] = 2.0 * S                        # ... dq[rq, c2] = ds[rq, rk] k[rk, c2] / 8 does
        i["at"] = {"dq": rq * C + c2}
    else:
        v[rk, c1] = 10.0
        k[:nk_rows, c2] = 0.0
        q[rq, c2] = 2.0 * S
        i["at"] = {"dk": rk * C + c2}
    return i


def attn_oracle(case, i):
    qr, kr, nq_rows, nk_rows, heads, mask = attn_geometry(case)
    G, L = qr.shape
    S = kr.shape[1]
    C = heads * 64
    q, k, v = (i[n][:r].double().clone().requires_grad_() for n, r in (("q", nq_rows), ("k", nk_rows), ("v", nk_rows)))
    qg = q[qr.reshape(-1)].reshape(G, L, heads, 64).permute(0, 2, 1, 3)
    kg = k[kr.reshape(-1)].reshape(G, S, heads, 64).permute(0, 2, 1, 3)
    vg = v[kr.reshape(-1)].reshape(G, S, heads, 64).permute(0, 2, 1, 3)
    sc = (qg * 0.125) @ kg.transpose(-1, -2)
    if mask is not None:
        sc = sc.masked_fill(mask.view(1, 1, L, S), float("-inf"))
    p = torch.softmax(sc, dim=-1)
    if i.get("keep") is not None:
        p = p * i["keep"].double().cpu().reshape(G, heads, L, S)
    og = (p @ vg).permute(0, 2, 1, 3).reshape(G * L, C)
    o = torch.zeros(nq_rows, C, dtype=torch.float64).index_add(0, qr.reshape(-1), og)
    if case["producer"] == "attn_fwd":
        return dict(o=o.detach())
    dq, dk, dv = torch.autograd.grad((o * i["go"][:nq_rows].double()).sum(), [q, k, v])
    return dict(dq=dq, dk=dk, dv=dv)


# ------------------------------------------------------------------------------------------------------------------- the registry
PRODUCERS = {
    "layernorm_fwd": (LAYERNORM_FWD, layernorm_inputs, layernorm_oracle),
    "layernorm_bwd": (LAYERNORM_BWD, layernorm_inputs, layernorm_oracle),
    "posfuse_fwd": (POSFUSE, posfuse_inputs, posfuse_oracle),
    "ln_posfuse_fwd": (LN_POSFUSE, posfuse_inputs, posfuse_oracle),
    "posfuse_instance_fwd": (POSFUSE_INSTANCE, posfuse_instance_inputs, posfuse_instance_oracle),
    "frameln_act_fwd": (FRAMELN_FWD, frameln_inputs, frameln_oracle),
    "frameln_act_fwd_parts": (FRAMELN_FWD_PARTS, frameln_inputs, frameln_oracle),
    "frameln_act_bwd": (FRAMELN_BWD, frameln_inputs, frameln_oracle),
    "frameln_act_bwd_apply": (FRAMELN_BWD_APPLY, frameln_inputs, frameln_oracle),
    "drop_apply": (DROP_APPLY, drop_inputs, drop_oracle),
    "grid_center_pad": (GRID_PAD, grid_inputs, grid_oracle),
    "grid_center_cut": (GRID_CUT, grid_inputs, grid_oracle),
    "amax": (AMAX, amax_inputs, amax_oracle),
    "split_weight_f16": (SPLIT_WEIGHT, split_inputs, split_oracle),
    "split_weights_f16": (SPLIT_WEIGHTS, split_inputs, split_oracle),
    "gemm": (GEMM, gemm_inputs, gemm_oracle),
    "attn_fwd": (ATTN_FWD, attn_inputs, attn_oracle),
    "attn_bwd": (ATTN_BWD, attn_inputs, attn_oracle),
}

# the planted positions each producer has a region for (the host test holds the tables to this)
REQUIRED = {
    "layernorm_fwd": ("first", "last", "partial_block", "wave3", "wrap32", "second_trip"),
    "layernorm_bwd": ("first", "last", "partial_block", "wave3", "wrap32", "second_trip"),
    "posfuse_fwd": ("first", "last", "partial_block", "wave3", "wrap32", "second_trip"),
    "ln_posfuse_fwd": ("first", "last", "wave3", "wrap32"),                      # one block per frame, whole frames: no partial block, no loop
    "posfuse_instance_fwd": ("first", "last", "partial_block", "wave3", "wrap32"),
    "frameln_act_fwd": ("first", "last", "partial_block", "wave3", "wrap32", "second_trip"),
    "frameln_act_fwd_parts": ("first", "last", "wave3", "wrap32"),               # whole blocks of 4096 elements, no loop
    "frameln_act_bwd": ("first", "last", "partial_block", "wave3", "wrap32"),    # the grid is not capped
    "frameln_act_bwd_apply": ("first", "last", "partial_block", "wave3", "wrap32"),
    "drop_apply": ("first", "last", "partial_block", "wave3", "wrap32", "second_trip"),
    "grid_center_pad": ("first", "last", "partial_block", "wave3", "wrap32", "second_trip"),
    "grid_center_cut": ("first", "last", "partial_block", "wave3", "wrap32", "second_trip"),
    "amax": ("first", "last", "wave3", "wrap32", "second_trip"),
    "split_weight_f16": ("first", "last", "wave3", "second_trip"),               # 16 blocks: no word wraps
    "split_weights_f16": ("last", "second_trip"),
    "attn_fwd": ("first", "last"),                      # last: the last query row and the last key row of a partial tile
    "attn_bwd": ("first", "last"),
    "gemm": ("first", "last"),                          # tiles, not a grid-stride loop; the edge tile's last row and quad
}


def has_dropout(case):
    return case["producer"] == "drop_apply" or bool(case.get("drop") or case.get("dp")) or case.get("ep") in ("dropout", "droppath")


def all_cases():
    return [c for table, _, _ in PRODUCERS.values() for c in table]


def build(case, keep=None):
    """-> (inputs, oracle outputs) of a case; keep: the device's keep-scales for a dropout case"""
    _, inputs, oracle = PRODUCERS[case["producer"]]
    i = inputs(case, keep) if has_dropout(case) else inputs(case)
    return i, oracle(case, i)


def planted_ok(out, at):
    """-> (|max|, its flat index, the largest other |value|) of a stored output; the case holds iff index == at and other < max / 2"""
    a = out.detach().abs().flatten()
    m, idx = a.max(0)
    rest = a.clone()
    rest[idx] = 0
    return float(m), int(idx), float(rest.max())


def trips(case):
    """(work items of the capped loop, items per trip) of a second_trip case: the host test requires items > per trip and the planted
    index beyond the first trip"""
    p = case["producer"]
    if p in ("layernorm_fwd", "layernorm_bwd"):
        cap = CAPS["ln_fwd" if p == "layernorm_fwd" else "ln_bwd"]
        return case["rows"], cap["blocks"] * cap["rows_per_block"], case["C"]
    if p in ("posfuse_fwd", "frameln_act_fwd"):
        n = (case["N"] * case["T"] if p == "posfuse_fwd" else case["frames"]) * case["pf"]
        return n // 4, CAPS["ew_blocks"]["blocks"] * CAPS["ew_blocks"]["float4_per_block"], 4
    if p == "drop_apply":
        return case["rows"] * case["cols"] // 4, CAPS["ew_blocks"]["blocks"] * CAPS["ew_blocks"]["float4_per_block"], 4
    if p == "amax":
        return case["rows"] * case["cols"] // 4, CAPS["npvp_amax"]["blocks"] * CAPS["npvp_amax"]["float4_per_block"], 4
    if p in ("split_weight_f16", "split_weights_f16"):
        N, K, _ = (case["N"], case["K"], 0) if p == "split_weight_f16" else SPLIT_RECORDS[-1]
        return N * K // 4, CAPS["weights_amax"]["blocks"] * CAPS["weights_amax"]["float4_per_block"], 4
    if p in ("grid_center_pad", "grid_center_cut"):
        inner, outer = _grid_rows(case)
        return (outer + case["tail"] if p == "grid_center_pad" else inner), CAPS["gridpad"]["blocks"] * CAPS["gridpad"]["rows_per_trip"], case["C"]
    raise KeyError(p)
