"""GPU: attention over sequences longer than 128 - the streaming MFMA kernels (npvp_attn_long_fwd / npvp_attn_long_bwd, which
npvp_amd.ops takes when max(L, S) >= ops.ATTN_LONG_MIN) against the CPU oracle (oracle.ops.attn_core) on the same seeded inputs:
forward and every gradient, the bar of tests/test_hip_ops.py (rel-L2 1e-4 whole tensor and worst row).  Shapes are the smallest at
which a streaming kernel can go wrong: first length past the old limit, ragged and tile-aligned (64-row tiles, 16-row blocks)
query / key counts, the encoder mask's dead key at the end of a full and of a partial tile, many queries on few keys and the
reverse, windows of 12 x 12 tokens.  C = 512, 8 heads, N = 1, P = 8 for the temporal cases (64 workgroups per query tile)."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import golden_cases as GC
from oracle import ops as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4           # whole tensor and worst row: the bar of every attention test (tests/test_hip_ops.py), inside north_star's 1e-3
C, HEADS, P = 512, 8, 8


def close(a, b, what):
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    e, er = GC.rel_err(a, b), GC.max_row_rel_err(a, b, 1e-6)
    GC.log_err("attn_long", os.environ.get("PYTEST_CURRENT_TEST", "").split("::")[-1].split(" ")[0] + " " + what, e, er)
    print(f"{what}: rel-L2 {e:.3e} worst row {er:.3e}")
    assert e < TOL, f"{what}: rel-L2 {e:.3e} >= {TOL:.1e}"
    assert er < TOL, f"{what}: worst-row rel-L2 {er:.3e} >= {TOL:.1e}"


@pytest.fixture(scope="module")
def K():
    import npvp_amd
    from npvp_amd import ops
    assert torch.cuda.is_available()
    ops.rng.manual_seed(1234, torch.device(DEV))
    ops.set_gemm_precision("f16x3")          # the default arithmetic (the attention cores are the same kernels in every GEMM mode)
    return ops


def g(t):
    return t.detach().to(DEV).requires_grad_()


@functools.lru_cache(maxsize=None)
def temporal_ref(Tq, Tk, mask):
    """inputs, cotangent and the oracle's (y, dq, dk, dv) of one temporal / cross case: computed once, shared, never modified"""
    q = O.seeded_randn((Tq * P, C), 81).requires_grad_()
    k = O.seeded_randn((Tk * P, C), 82).requires_grad_(); v = O.seeded_randn((Tk * P, C), 83).requires_grad_()
    cot = O.seeded_randn((Tq * P, C), 84)
    m = O.encoder_temporal_mask(Tq) if mask else None
    y = O.attn_core(q, k, v, O.temporal_groups(1, Tq, P), O.temporal_groups(1, Tk, P), HEADS, m)
    ref = torch.autograd.grad((y * cot).sum(), [q, k, v])
    return (q.detach(), k.detach(), v.detach(), cot), (y.detach(),) + tuple(ref)


def cfg_t(Tq, Tk, mask, p=0.0):
    from npvp_amd.ops import AttnCfg
    return AttnCfg(1, 1, P, 8, 0, Tq, Tk, HEADS, mask, p)


def run_attn(K, q, k, v, cot, cfg):
    ins = [g(q), g(k), g(v)]
    y = K.attn(ins[0], ins[1], ins[2], cfg)
    return (y.detach(),) + tuple(torch.autograd.grad((y * cot.to(DEV)).sum(), ins))


def check_temporal(K, Tq, Tk, mask):
    (q, k, v, cot), want = temporal_ref(Tq, Tk, mask)
    got = run_attn(K, q, k, v, cot, cfg_t(Tq, Tk, mask))
    for a, b, n in zip(got, want, ["y", "dq", "dk", "dv"]):
        close(a, b, n)


# ------------------------------------------------------------------------------- 1. temporal / cross
@pytest.mark.parametrize("Tq,Tk,mask", [(129, 129, 1), (137, 137, 0), (192, 192, 1), (200, 200, 1), (257, 3, 0), (130, 2, 0), (5, 150, 0)])
def test_temporal_and_cross(K, Tq, Tk, mask):
    check_temporal(K, Tq, Tk, mask)


def test_separate_operands_with_padded_row_strides(K):
    """q, k, v as the left C columns of [R, C + 32] buffers: every operand with its own row stride"""
    T = 137
    (q, k, v, cot), want = temporal_ref(T, T, 0)
    big = [torch.zeros(T * P, C + 32, device=DEV).requires_grad_() for _ in range(3)]
    with torch.no_grad():
        for b, t in zip(big, (q, k, v)):
            b[:, :C] = t.to(DEV)
    y = K.attn(big[0][:, :C], big[1][:, :C], big[2][:, :C], cfg_t(T, T, 0))
    grads = torch.autograd.grad((y * cot.to(DEV)).sum(), big)
    close(y, want[0], "y")
    for a, b, n in zip(grads, want[1:], ["dq", "dk", "dv"]):
        close(a[:, :C], b, n)
        assert not bool(a[:, C:].any()), f"{n}: the padding columns are not part of the operand"


def test_packed_qk(K):
    """q | k as the halves of one [R, 2C] projection output (attn_packed: one amax slot for d(q|k))"""
    T = 137
    (q, k, v, cot), want = temporal_ref(T, T, 0)
    qk, vg = g(torch.cat([q, k], 1)), g(v)
    y = K.attn_packed(qk, vg, cfg_t(T, T, 0))
    dqk, dv = torch.autograd.grad((y * cot.to(DEV)).sum(), [qk, vg])
    close(y, want[0], "y"); close(dqk, torch.cat([want[1], want[2]], 1), "dqk"); close(dv, want[3], "dv")


# ------------------------------------------------------------------------------- 2. spatial windows
@pytest.mark.parametrize("frames,H,W", [(2, 12, 12), (1, 12, 24)])
def test_spatial_window_of_144_tokens(K, frames, H, W):
    """ws = 12: L = S = 144; the 12 x 24 grid has two windows per frame (window origins with nww > 1)"""
    from npvp_amd.ops import AttnCfg
    ws, R = 12, frames * H * W
    qk = O.seeded_randn((R, 2 * C), 71).requires_grad_(); v = O.seeded_randn((R, C), 72).requires_grad_()
    cot = O.seeded_randn((R, C), 73)
    rows = O.spatial_groups(frames, H, W, ws)
    y = O.attn_core(qk[:, :C], qk[:, C:], v, rows, rows, HEADS, None)
    rqk, rv = torch.autograd.grad((y * cot).sum(), [qk, v])
    qkg, vg = g(qk), g(v)
    yg = K.attn_packed(qkg, vg, AttnCfg(0, frames, H * W, W, ws, 0, 0, HEADS, 0, 0.0))
    gqk, gv = torch.autograd.grad((yg * cot.to(DEV)).sum(), [qkg, vg])
    close(yg, y.detach(), "y"); close(gqk, rqk, "dqk"); close(gv, rv, "dv")


# ------------------------------------------------------------------------------- 3. dropout
class _Inject:
    """hands the recorded masks to the oracle's F.dropout in call order (the mechanism of tests/test_hip_dropout.py)"""

    def __init__(self, masks):
        self.masks, self.i = masks, 0

    def dropout(self, x, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return x
        assert self.i < len(self.masks), "the oracle asked for more dropout sites than the HIP path recorded"
        (drop, kind, count), m = self.masks[self.i]
        self.i += 1
        assert kind == "elem" and count == x.numel(), f"HIP recorded ({kind}, {count}), the oracle wants (elem, {x.numel()})"
        return x * m.view(x.shape)


def record(K, fn):
    """-> (fn(), [(site, mask on the CPU)]) with the dropout sites of fn's forward kernels recorded"""
    K.DropRecorder.sites = []
    try:
        out = fn()
        sites = K.DropRecorder.sites
    finally:
        K.DropRecorder.sites = None
    return out, [(s, K.DropRecorder.mask(s, torch.device(DEV)).cpu()) for s in sites]


def test_dropout_mask_forward_and_replay(K):
    T, p = 137, 0.1
    (q, k, v, cot), _ = temporal_ref(T, T, 0)
    K.rng.manual_seed(4242, torch.device(DEV))
    ins = [g(q), g(k), g(v)]
    y, masks = record(K, lambda: K.attn(ins[0], ins[1], ins[2], cfg_t(T, T, 0, p)))
    got = torch.autograd.grad((y * cot.to(DEV)).sum(), ins, retain_graph=True)
    again = torch.autograd.grad((y * cot.to(DEV)).sum(), ins)
    for a, b, n in zip(got, again, ["dq", "dk", "dv"]):
        assert torch.equal(a, b), f"{n}: a second backward of the same forward must replay the same mask, bit for bit"
    assert [(s[1], s[2]) for s, _ in masks] == [("elem", P * HEADS * T * T)]
    m = masks[0][1]
    assert all(x == 0.0 or abs(x - 1.0 / (1.0 - p)) < 1e-6 for x in m.unique().tolist())
    keep = float((m != 0).double().mean())
    assert abs(keep - (1.0 - p)) < 0.01, f"keep fraction {keep:.4f}"
    inj = _Inject(masks)
    old = F.dropout
    torch.nn.functional.dropout = inj.dropout
    try:
        qr, kr, vr = (t.clone().requires_grad_() for t in (q, k, v))
        yr = O.attn_core(qr, kr, vr, O.temporal_groups(1, T, P), O.temporal_groups(1, T, P), HEADS, None, p, True)
        ref = torch.autograd.grad((yr * cot).sum(), [qr, kr, vr])
    finally:
        torch.nn.functional.dropout = old
    assert inj.i == 1
    close(y.detach(), yr.detach(), "y")
    for a, b, n in zip(got, ref, ["dq", "dk", "dv"]):
        close(a, b, n)


# ------------------------------------------------------------------------------- 4. the same function as the existing kernels
@pytest.mark.parametrize("Tq,Tk,mask", [(10, 10, 1), (33, 33, 0), (64, 64, 1), (65, 65, 0), (128, 128, 1), (48, 5, 0)])
def test_short_sequences_through_the_streaming_kernels(K, Tq, Tk, mask):
    old = K.ATTN_LONG_MIN
    try:
        K.ATTN_LONG_MIN = 1
        check_temporal(K, Tq, Tk, mask)
    finally:
        K.ATTN_LONG_MIN = old


@pytest.mark.parametrize("Tq,Tk,mask", [(40, 40, 0), (10, 10, 1), (18, 18, 1), (28, 2, 0), (40, 40, 1)])
def test_dropout_mask_is_the_one_of_the_existing_route(K, Tq, Tk, mask):
    """one dropout key and one mask for every route: the generic kernels (40 rows), the MFMA backward (10), the staged backward
    <2,2> (18) and <2,1> (28 x 2), each against the streaming kernels under the same seed and salt"""
    p = 0.1
    (q, k, v, cot), _ = temporal_ref(Tq, Tk, mask)
    outs = []
    old = K.ATTN_LONG_MIN
    for lo in (old, 1):
        K.rng.manual_seed(977, torch.device(DEV))             # same seed, and the same salt: the first site after seeding
        ins = [g(q), g(k), g(v)]
        try:
            K.ATTN_LONG_MIN = lo                              # (the route is chosen when a node runs: backward inside the try too)
            y, masks = record(K, lambda: K.attn(ins[0], ins[1], ins[2], cfg_t(Tq, Tk, mask, p)))
            grads = torch.autograd.grad((y * cot.to(DEV)).sum(), ins)
        finally:
            K.ATTN_LONG_MIN = old
        assert len(masks) == 1
        outs.append((masks[0][0][0].salt, masks[0][1], y.detach(), grads))
    assert outs[0][0] == outs[1][0], "both runs must key their site with the same salt"
    assert torch.equal(outs[0][1], outs[1][1]), "recorded masks differ between the two routes"
    # the recorded mask is a replay through npvp_drop_apply: what the two KERNELS drew shows in their outputs
    close(outs[1][2], outs[0][2], "y streaming vs existing route")
    for a, b, n in zip(outs[1][3], outs[0][3], ["dq", "dk", "dv"]):          # ... and, for the replay in backward, in their gradients
        close(a, b, n + " streaming vs existing route")


# ------------------------------------------------------------------------------- 5. bit reproducibility
def test_bit_reproducible(K):
    (q, k, v, cot), _ = temporal_ref(200, 200, 1)
    a = run_attn(K, q, k, v, cot, cfg_t(200, 200, 1))
    b = run_attn(K, q, k, v, cot, cfg_t(200, 200, 1))
    for x, y, n in zip(a, b, ["y", "dq", "dk", "dv"]):
        assert torch.equal(x, y), n


# ------------------------------------------------------------------------------- 6. amax slots
def test_amax_slots_feed_the_gemms(K):
    """linear(attn(q, k, v)) in the default f16x3 arithmetic: the GEMM scales its operand by the amax slot the attention kernel
    committed for o (forward) and the dgrad's output feeds the streaming backward; an uncommitted or wrong slot breaks the scale"""
    T = 137
    (q, k, v, cot), _ = temporal_ref(T, T, 0)
    w, b = 0.05 * O.seeded_randn((C, C), 91), 0.1 * O.seeded_randn((C,), 92)
    qr = q.clone().requires_grad_()
    yr = O.linear(O.attn_core(qr, k, v, O.temporal_groups(1, T, P), O.temporal_groups(1, T, P), HEADS, None), w, b)
    (gr,) = torch.autograd.grad((yr * cot).sum(), [qr])
    qg = g(q)
    yg = K.linear(K.attn(qg, k.to(DEV), v.to(DEV), cfg_t(T, T, 0)), w.to(DEV), b.to(DEV))
    (gq,) = torch.autograd.grad((yg * cot.to(DEV)).sum(), [qg])
    close(yg.detach(), yr.detach(), "y"); close(gq, gr, "dq")


# ------------------------------------------------------------------------------- 7. whole predictor
@pytest.mark.parametrize("case", [("D", 1, 2, 132, 91, (1, 1)), ("S", 1, 3, 130, 11, (1, 1))], ids=["D_2_132", "S_3_130"])
def test_whole_predictor(K, case):
    """More than 128 target frames through the whole Predictor, forward and gradients, against the oracle (computed in-process):
    decoder temporal (132 x 132) and encoder-decoder (132 x 2) attention; NPVP-S: 130 frames through the MASKED encoder temporal
    attention of the posterior.  The bar of test_against_oracle_larger."""
    import npvp_amd
    import larger_oracle as LO
    seed, past, fut, want = LO.compute(case)
    args, kw = LO.predictor_args(case)
    hip = npvp_amd.Predictor(*args, **kw)
    O.key_hashed_fill(hip, 7)
    got = LO.run(hip.to(DEV), DEV, past, fut, case)
    for a, b, n in zip(got, want, ["y", "g_past", "g_tied_norm"]):
        e = GC.rel_err(a, b)
        GC.log_err(f"attn_long_predictor_{case[0]}", n, e)
        print(f"{n}: rel-L2 {e:.3e} (input seed {seed})")
        assert e < 5e-4, f"{n}: {e:.3e} (input seed {seed})"
