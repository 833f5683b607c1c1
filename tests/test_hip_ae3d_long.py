"""GPU: the learn_3d=True autoencoder on clips of more than 32 frames - the key-tiled temporal attention kernels (csrc/ae_temporal.hip,
ops.temporal_attn_long / _packed, npvp_temporal_attn_long_fwd / _bwd) against float64, the Factorized3DConvAttn block through the
trainable path against the reference fixture of a 50-frame clip (tests/golden/ae3d_long_block_*.npz), ae_train_step / ae_val_step
against the stock PyTorch-ROCm step at T = 40 and at the KTH protocol (10 past + 40 future), and the frozen fused pair on 40 frames.
Bounds and constructions: tests/test_hip_ae3d.py's."""
import copy

import pytest
import torch

import ae3d_cases as AC
import ae3d_long_cases as LC
import golden_cases as GC
from oracle import ops as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNEL_TOL = 1e-5                                    # hand-written kernels vs float64, no MIOpen involved
GRAD_TOL, LOSS_TOL, NORM_TOL = 5e-3, 1e-4, 0.15      # MIOpen convolutions and ReLU kinks in the path (tests/test_hip_ae_train.py)
ZERO_GRAD = AC.ZERO_GRAD
PT_8_32 = (6, 4)                                     # pixels per workgroup of the key-tiled kernels at (8, 32), T = 33: forward, backward
rel = AC.rel


@pytest.fixture(scope="module")
def npvp():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import npvp_amd
    return npvp_amd


def worst_row(got, want):
    """largest row error, each row against the larger of its own norm and the tensor's RMS row norm (tests/test_hip_ae3d.py)"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    rn = want.norm(dim=1)
    floor = (want.norm() / want.shape[0] ** 0.5).clamp_min(1e-30)
    return float(((got - want).norm(dim=1) / torch.maximum(rn, floor)).max())


def _run_packed(npvp, q, k, v, go, N, T, HW, ld=None, op=None):
    A, V = q.shape[1], v.shape[1]
    ld = ld or 2 * A + V
    qkv = torch.zeros(q.shape[0], ld)
    qkv[:, :A], qkv[:, A:2 * A], qkv[:, 2 * A:2 * A + V] = q, k, v
    leaf = qkv.to(DEV).requires_grad_()
    o = (op or npvp.ops.temporal_attn_long_packed)(leaf, N, T, HW, A, V)
    o.backward(go.to(DEV))
    g = leaf.grad
    return o.detach(), g[:, :A], g[:, A:2 * A], g[:, 2 * A:2 * A + V], g[:, 2 * A + V:]


def _assert_close(got, want, what):
    for name, g, w in zip(("o", "dq", "dk", "dv"), got, want):
        e, r = rel(g, w), worst_row(g, w)
        print(f"{what} {name}: rel-L2 {e:.2e} worst row {r:.2e}")
        assert e < KERNEL_TOL and r < KERNEL_TOL, (what, name, e, r)


# ------------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("A,V,T", LC.KERNEL_CASES)
def test_temporal_attn_long_vs_float64(npvp, A, V, T):
    N, HW = 2, 5
    q, k, v, go = AC.kernel_inputs(A, V, N, T, HW)
    want = AC.temporal_attn_ref64(q, k, v, go, N, T, HW)
    _assert_close(_run_packed(npvp, q, k, v, go, N, T, HW)[:4], want, f"({A},{V}) T={T}")


@pytest.mark.parametrize("A,V,HW", [(8, 32, hw) for hw in sorted({1} | {hw for pt in PT_8_32 for hw in (pt - 1, pt, pt + 1, 4 * pt + 3)})] + [(64, 256, 3)])
def test_temporal_attn_long_pixel_tiles(npvp, A, V, HW):
    """(8, 32) at T = 33 (two frame tiles, 17 + 16) takes 6 pixels per workgroup in the forward and 4 in the backward: for either, the
    last tile of a clip partial, exact, one over, and 4 PT + 3 = full tiles and a partial one; (64, 256) takes one or two pixels"""
    N, T = 2, 33
    q, k, v, go = AC.kernel_inputs(A, V, N, T, HW, seed=520)
    _assert_close(_run_packed(npvp, q, k, v, go, N, T, HW)[:4], AC.temporal_attn_ref64(q, k, v, go, N, T, HW), f"({A},{V}) HW={HW}")


@pytest.mark.parametrize("T", [9, 32])
def test_up_to_32_frames_are_the_one_tile_kernels(npvp, T):
    """T <= 32: o, dq, dk and dv of the long op are the bits of ops.temporal_attn_packed, with as many launches"""
    N, HW, A, V = 2, 5, 16, 64
    q, k, v, go = AC.kernel_inputs(A, V, N, T, HW, seed=525)
    L = npvp._lib.lib()
    n0 = L.npvp_launch_count()
    old = _run_packed(npvp, q, k, v, go, N, T, HW, op=npvp.ops.temporal_attn_packed)
    n1 = L.npvp_launch_count()
    new = _run_packed(npvp, q, k, v, go, N, T, HW)
    n2 = L.npvp_launch_count()
    assert all(torch.equal(a, b) for a, b in zip(old, new))
    assert n2 - n1 == n1 - n0 == 2


def test_unpacked_sequences(npvp):
    """ops.temporal_attn_long on (M, T, d) sequences, (64, 256) at T = 33: three frame tiles of 11, two 128-column chunks of v"""
    M, T, A, V = 3, 33, 64, 256
    q, k, v, go = AC.kernel_inputs(A, V, 1, T, M, seed=530)          # rows = t M + m
    want = AC.temporal_attn_ref64(q, k, v, go, 1, T, M)
    seq = lambda t: t.reshape(T, M, -1).transpose(0, 1).contiguous().to(DEV).requires_grad_()
    qs, ks, vs = seq(q), seq(k), seq(v)
    o = npvp.ops.temporal_attn_long(qs, ks, vs, T)
    o.backward(go.reshape(T, M, V).transpose(0, 1).to(DEV))
    rows = lambda t: t.detach().transpose(0, 1).reshape(T * M, -1)
    _assert_close((rows(o), rows(qs.grad), rows(ks.grad), rows(vs.grad)), want, "unpacked (64,256) T=33")


def test_rescale_both_ways(npvp):
    """(16, 64) at T = 40, two key tiles.  Pixel 1 of clip 0: q[t=3] = k[t=39] with squared norm 120 - the max arrives in the last key
    tile, what the first tile summed is rescaled by exp(-120) (exp(120) itself overflows fp32).  Pixel 2 of clip 1: q[t=35] = k[t=0] -
    the max sits in the first tile and every later tile is scaled down to it.  Everything finite and within KERNEL_TOL of float64."""
    N, T, HW, A, V = 2, 40, 5, 16, 64
    q, k, v, go = AC.kernel_inputs(A, V, N, T, HW, seed=550)
    row = lambda n, t, p: (n * T + t) * HW + p
    big = torch.full((A,), (120.0 / A) ** 0.5)
    q[row(0, 3, 1)] = k[row(0, 39, 1)] = big
    q[row(1, 35, 2)] = k[row(1, 0, 2)] = big
    got = _run_packed(npvp, q, k, v, go, N, T, HW)
    assert all(torch.isfinite(t).all() for t in got)
    _assert_close(got[:4], AC.temporal_attn_ref64(q, k, v, go, N, T, HW), "rescale")


def test_separate_buffers_and_poison(npvp):
    """through the C ABI: q / k / v / o / go / dq / dk / dv / D in buffers of their own, each with another leading dimension and 8
    guard rows around it: NaN around the inputs (none is read: every result is finite and right), a bit pattern around the outputs
    and around D (none is changed); lse is float64's log-sum-exp"""
    N, T, HW, A, V = 2, 33, 17, 8, 32
    R = N * T * HW
    q, k, v, go = AC.kernel_inputs(A, V, N, T, HW, seed=560)
    want = AC.temporal_attn_ref64(q, k, v, go, N, T, HW)
    PAT = -1.2345e33
    GUARD = 8                                             # rows in front of and behind the operand

    def embed(t, ld, fill, rows=R):
        buf = torch.full((rows + 2 * GUARD, ld), fill)
        if t is not None:
            buf[GUARD:GUARD + rows, :t.shape[1]] = t
        return buf.to(DEV)
    nan = float("nan")
    ins = [embed(q, 12, nan), embed(k, 16, nan), embed(v, 36, nan), embed(go, 40, nan)]
    outs = [embed(None, 44, PAT), embed(None, 8, PAT), embed(None, 20, PAT), embed(None, 32, PAT)]         # o, dq, dk, dv
    Dbuf = embed(None, 4, PAT, rows=2 * R // 4)                                                           # D [2][R] as rows of 4 floats
    lse = torch.full((R + 2 * GUARD,), PAT).to(DEV)
    body = lambda b: b[GUARD:GUARD + R]
    L = npvp._lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    qp, kp, vp, gp = (body(b).data_ptr() for b in ins)
    op, dqp, dkp, dvp = (body(b).data_ptr() for b in outs)
    lp, Dp = lse[GUARD:].data_ptr(), Dbuf[GUARD:].data_ptr()
    assert L.npvp_temporal_attn_long_fwd(qp, 12, kp, 16, vp, 36, op, 44, lp, N, T, HW, A, V, st) == 0, L.npvp_last_error()
    assert L.npvp_temporal_attn_long_bwd(qp, 12, kp, 16, vp, 36, gp, 40, lp, Dp, dqp, 8, dkp, 20, dvp, 32, N, T, HW, A, V, st) == 0, \
        L.npvp_last_error()
    torch.cuda.synchronize()
    widths = (V, A, A, V)
    got = [body(b)[:, :w] for b, w in zip(outs, widths)]
    assert all(torch.isfinite(g).all() for g in got)
    _assert_close(got, want, "separate buffers")
    for b, w in zip(outs, widths):
        c = b.cpu()
        assert bool((c[:GUARD] == PAT).all()) and bool((c[GUARD + R:] == PAT).all()) and bool((c[GUARD:GUARD + R, w:] == PAT).all())
    for b, t in zip(ins, (q, k, v, go)):                  # the inputs are read only
        c = b.cpu()
        assert torch.equal(c[GUARD:GUARD + R, :t.shape[1]], t) and bool(torch.isnan(c[:GUARD]).all()) and bool(torch.isnan(c[GUARD + R:]).all())
    d, ls = Dbuf.cpu(), lse.cpu()
    assert bool((d[:GUARD] == PAT).all()) and bool((d[GUARD + 2 * R // 4:] == PAT).all())
    assert bool(torch.isfinite(d[GUARD:GUARD + 2 * R // 4]).all()) and bool((d[GUARD:GUARD + 2 * R // 4] != PAT).all())
    assert bool((ls[:GUARD] == PAT).all()) and bool((ls[GUARD + R:] == PAT).all())
    qs, ks = (t.double().reshape(N, T, HW, -1).transpose(1, 2) for t in (q, k))          # (N, HW, T, A), as AC.temporal_attn_ref splits
    want_lse = torch.logsumexp(qs @ ks.transpose(-1, -2), -1).transpose(1, 2).reshape(R)
    assert rel(ls[GUARD:GUARD + R], want_lse) < 1e-5


def test_clips_and_pixels_do_not_mix_and_runs_repeat(npvp):
    N, T, HW, A, V = 2, 40, 6, 32, 128
    q, k, v, go = AC.kernel_inputs(A, V, N, T, HW, seed=570)
    base = _run_packed(npvp, q, k, v, go, N, T, HW)
    again = _run_packed(npvp, q, k, v, go, N, T, HW)
    assert all(torch.equal(a, b) for a, b in zip(base, again))                      # bit-identical on a repeated run
    clip0 = slice(0, T * HW)
    q2, k2, v2, go2 = (t.clone() for t in (q, k, v, go))
    for t in (q2, k2, v2, go2):
        t[T * HW:] = t[T * HW:] * -0.7 + 0.3                                        # every frame of clip 1
    other = _run_packed(npvp, q2, k2, v2, go2, N, T, HW)
    assert all(torch.equal(a[clip0], b[clip0]) for a, b in zip(base[:4], other))
    assert not torch.equal(base[0][T * HW:], other[0][T * HW:])
    q3, k3, v3, go3 = (t.clone() for t in (q, k, v, go))
    pix = torch.arange(N * T * HW) % HW == 3                                        # pixel 3 of every frame of both clips
    for t in (q3, k3, v3, go3):
        t[pix] = t[pix] * 1.3 - 0.2
    other = _run_packed(npvp, q3, k3, v3, go3, N, T, HW)
    assert all(torch.equal(a[~pix], b[~pix]) for a, b in zip(base[:4], other))
    assert not torch.equal(base[0][pix], other[0][pix])


def test_padded_packed_rows(npvp):
    """ld = 2A+V rounded up to 32 (what the model's GEMM hands over): the gradient's pad columns are exactly zero"""
    N, T, HW, A, V = 2, 33, 7, 8, 32
    q, k, v, go = AC.kernel_inputs(A, V, N, T, HW, seed=540)
    got = _run_packed(npvp, q, k, v, go, N, T, HW, ld=64)
    _assert_close(got[:4], AC.temporal_attn_ref64(q, k, v, go, N, T, HW), "ld=64")
    assert got[4].shape[1] == 16 and float(got[4].abs().max()) == 0.0


# -------------------------------------------------------------------------------------------------------------------- the block
@pytest.mark.parametrize("cf", [True, False], ids=["conv", "attn"])
def test_long_block_through_the_trainable_path(npvp, cf):
    """Factorized3DConvAttn(64, learn_3d=True) through models/ae_train._fact on channels-last frames of one 50-frame clip against the
    reference fixture, at the bars of tests/test_hip_ae3d.py::test_block_through_the_trainable_path"""
    from npvp_amd.models import Factorized3DConvAttn
    from npvp_amd.models.ae_train import _fact
    N, T, H, W = LC.LONG_BLOCK
    gold, tag = GC.load(LC.long_block_file(cf)), LC.long_block_tag(cf)
    blk = O.key_hashed_fill(Factorized3DConvAttn(AC.BLOCK_C, conv_first=cf, learn_3d=True), LC.BLOCK_SEED).to(DEV)
    blk = blk.to(memory_format=torch.channels_last)
    x, cot = LC.long_block_input()
    blk.eval()
    with torch.no_grad():
        ye = _fact(blk, x.to(DEV).contiguous(memory_format=torch.channels_last), T)
    assert rel(ye, gold[f"{tag}.eval"]) < 1e-4
    blk.train()
    xi = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
    y = _fact(blk, xi, T)
    (y * cot.to(DEV)).sum().backward()
    assert rel(y, gold[f"{tag}.y"]) < 1e-4, rel(y, gold[f"{tag}.y"])
    for k, v in blk.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            assert rel(v, gold[f"{tag}.stat.{k}"]) < 1e-4, k
        elif k.endswith("num_batches_tracked"):
            assert int(v) == 1, k
    got, want = [xi.grad.reshape(-1)], [torch.as_tensor(gold[f"{tag}.dx"]).reshape(-1)]
    zero_bound = 1e-6 * cot.numel() ** 0.5             # rounding noise of an exactly-zero gradient (tests/test_ae3d_host.py)
    for n, p in blk.named_parameters():
        g = torch.as_tensor(gold[f"{tag}.grad.{n}"])
        if n.endswith(ZERO_GRAD):
            assert float(p.grad.abs().max()) < zero_bound and float(g.abs().max()) < zero_bound, n
            continue
        nh, ng = float(p.grad.double().norm()), float(g.double().norm())
        print(f"{tag} {n}: rel-L2 {rel(p.grad, g):.2e}")
        if n.startswith(("attn2d.Wq.", "attn2d.Wk.")):
            # a 2 x 2 grid pools to ONE key: the 2-D softmax is 1 whatever q and k are (dS = P (dP - D) = 0), so the gradients of the
            # query and key projections are exactly 0 - in the reference (the fixture holds zeros) and here, bit for bit
            assert ng == 0.0 and nh == 0.0, (n, nh, ng)
            continue
        assert ng > 0 and abs(nh - ng) <= NORM_TOL * ng, (n, nh, ng)
        got.append(p.grad.reshape(-1).cpu()); want.append(g.reshape(-1))
    got[0] = got[0].cpu()
    assert rel(torch.cat(got), torch.cat(want)) < GRAD_TOL


# --------------------------------------------------------------------------------------------------------------------- the step
def _pair(npvp, AE, ch, seed):
    enc, dec = npvp.build_autoencoder(AE, ch)
    O.key_hashed_fill(npvp.AEPair(enc, dec), seed)
    return enc, dec


def _frames(B, T, ch, S, seed, past=None):
    x = torch.tanh(O.seeded_randn((B, T, ch, S, S), seed))
    past = T // 2 if past is None else past
    return x[:, :past].contiguous().to(DEV), x[:, past:].contiguous().to(DEV)


def _stock_step(enc, dec, opt, past, fut):
    opt.zero_grad()
    x = torch.cat([past, fut], 1)
    loss = (dec(enc(x)) - x).abs().mean()
    loss.backward()
    opt.step()
    return loss.detach()


def test_ae3d_train_step_at_40_frames_matches_stock(npvp):
    """tests/test_hip_ae3d.py::test_ae3d_train_step_matches_stock with AE_SMALL at (B, T, S) = (1, 40, 8): 3 steps of the HIP path and
    of the stock path from the same weights and frames - losses, step-1 gradients, parameters and running statistics after step 3;
    then ae_val_step at the KTH protocol (10 past + 40 future frames, one encoder call on 50) against the stock eval loss"""
    AE, ch, B, T, S = AC.AE_SMALL, 1, 1, 40, 8
    enc, dec = _pair(npvp, AE, ch, 7)
    s_enc, s_dec = copy.deepcopy(enc).to(DEV), copy.deepcopy(dec).to(DEV)
    enc, dec = enc.to(DEV).to(memory_format=torch.channels_last), dec.to(DEV)
    npvp.prepare_trainable_autoencoder(enc, dec)
    opt = npvp.ae_optimizer(enc, dec, lr=1e-4)
    s_opt = torch.optim.Adam(list(s_enc.parameters()) + list(s_dec.parameters()), lr=1e-4, betas=(0.5, 0.999))
    s_pair = npvp.AEPair(s_enc, s_dec)
    called = []
    real = npvp.ops.temporal_attn_long_packed
    npvp.ops.temporal_attn_long_packed = lambda *a, **k: called.append(1) or real(*a, **k)
    try:
        for step in range(3):
            past, fut = _frames(B, T, ch, S, 60 + step)
            lh = npvp.ae_train_step(enc, dec, opt, past, fut)
            ls = _stock_step(s_enc, s_dec, s_opt, past, fut)
            assert abs(float(lh) - float(ls)) <= LOSS_TOL * abs(float(ls)), (step, float(lh), float(ls))
            if step == 0:
                hg, sg, skipped = [], [], 0
                for (n, p), (_, q) in zip(opt.ae_pair.named_parameters(), s_pair.named_parameters()):
                    hg.append(p.grad.reshape(-1)); sg.append(q.grad.reshape(-1))
                    if n.endswith(ZERO_GRAD):
                        assert float(p.grad.abs().max()) < 1e-6 and float(q.grad.abs().max()) < 1e-6, n
                        skipped += 1
                        continue
                    assert q.grad is not None and float(q.grad.norm()) > 0.0, n       # (gamma != 0: every parameter gets a gradient)
                    nh, ns = float(p.grad.double().norm()), float(q.grad.double().norm())
                    assert abs(nh - ns) <= NORM_TOL * ns, (n, nh, ns)
                assert skipped == 8 * sum(type(m).__name__ == "Factorized3DConvAttn" for m in enc.modules())
                assert rel(torch.cat(hg), torch.cat(sg)) < GRAD_TOL
        hs, ss = opt.ae_pair.state_dict(), s_pair.state_dict()
        assert list(hs) == list(ss)
        for kk in hs:
            if kk.endswith(ZERO_GRAD):
                continue
            if kk.endswith("num_batches_tracked"):
                assert int(hs[kk]) == int(ss[kk]) == 3
            else:
                assert rel(hs[kk], ss[kk]) < GRAD_TOL, (kk, rel(hs[kk], ss[kk]))
        steps_calls = len(called)
        past, fut = _frames(B, 50, ch, S, 70, past=10)                          # KTH: 10 -> 40
        lv, rec = npvp.ae_val_step(enc, dec, past, fut)
    finally:
        npvp.ops.temporal_attn_long_packed = real
    blocks = sum(type(m).__name__ == "Factorized3DConvAttn" for m in enc.modules())
    assert steps_calls == 3 * blocks and len(called) == 4 * blocks               # every temporal attention took the key-tiled op
    s_enc.eval(); s_dec.eval()
    with torch.no_grad():
        x = torch.cat([past, fut], 1)
        lvs = (s_dec(s_enc(x)) - x).abs().mean()
    assert rec.shape == x.shape
    assert abs(float(lv) - float(lvs)) <= LOSS_TOL * abs(float(lvs)) and enc.training and dec.training


# -------------------------------------------------------------------------------------------------------------- the frozen pair
def test_frozen_fused_pair_on_40_frames(npvp):
    """build_frozen_autoencoder(learn_3d=True) + to_device_layout on (1, 40, 1, 8, 8) frames (KTH's 40 future frames in one encoder
    call): the fused eval encoder against the unfused stock eval encoder at the forward bar (1e-4), through the library's kernels"""
    enc, dec = npvp.build_frozen_autoencoder(AC.AE_SMALL, 1)
    O.key_hashed_fill(npvp.AEPair(enc, dec), LC.PAIR_SEED)
    frames = torch.tanh(O.seeded_randn((1, 40, 1, 8, 8), 400)).to(DEV)
    s_enc = copy.deepcopy(enc).to(DEV).eval()
    fe, fd = npvp.to_device_layout(enc, dec, DEV)
    n0 = npvp._lib.lib().npvp_launch_count()
    with torch.no_grad():
        got, stock = fe(frames), s_enc(frames)
        rec = fd(got)
    assert npvp._lib.lib().npvp_launch_count() > n0
    assert rel(got, stock) < 1e-4, rel(got, stock)
    assert torch.isfinite(rec).all() and rec.shape == frames.shape


# ------------------------------------------------------------------------------------------------------------------ the one node
def test_each_packed_op_calls_its_own_exports(npvp):
    """the four packed attention ops share one autograd node: each makes exactly one _fwd and one _bwd call, of its own stem and of no
    other, and hands the backward a scratch D (the 22 arguments of the header) everywhere but in npvp_temporal_attn_bwd (21: it has
    no D).  (The numbers are held to float64 by the tests of each op.)"""
    L, ops = npvp._lib.lib(), npvp.ops
    stems = ("npvp_nonlocal_attn", "npvp_nonlocal_attn_grid", "npvp_temporal_attn", "npvp_temporal_attn_long")
    real = {s + p: getattr(L, s + p) for s in stems for p in ("_fwd", "_bwd")}
    calls = []
    count = lambda name: lambda *a: calls.append((name, len(a))) or real[name](*a)
    A, V, ld = 8, 32, 48
    cases = [(ops.nonlocal_attn_packed, stems[0], (1, 64, 64), 22),               # the smallest config shape at A = 8
             (ops.nonlocal_attn_grid_packed, stems[1], (2, 3, 5), 22),            # odd in both directions
             (ops.temporal_attn_packed, stems[2], (2, 3, 5), 21),
             (ops.temporal_attn_long_packed, stems[3], (1, 33, 3), 22)]           # the shortest clip on the key-tiled kernels
    assert all(len(npvp._lib.SIGNATURES[stem + "_bwd"][1]) == n for _, stem, _, n in cases)
    try:
        for name in real:
            setattr(L, name, count(name))
        for op, stem, (n0, n1, n2), nbwd in cases:
            del calls[:]
            qkv = O.seeded_randn((n0 * n1 * n2, ld), 610).mul_(0.5).to(DEV).requires_grad_()
            o = op(qkv, n0, n1, n2, A, V)
            o.backward(torch.ones_like(o))
            torch.cuda.synchronize()
            assert calls == [(stem + "_fwd", 15), (stem + "_bwd", nbwd)], (stem, calls)
            assert o.shape == (n0 * n1 * n2, V) and torch.isfinite(qkv.grad).all()
    finally:
        for name, f in real.items():
            setattr(L, name, f)
