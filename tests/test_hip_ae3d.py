"""GPU: the learn_3d=True autoencoder - the temporal attention kernels (csrc/ae_temporal.hip, ops.temporal_attn / _packed) against
float64, the Factorized3DConvAttn block through the trainable path against the reference fixtures (tests/golden/ae3d_block*.npz),
ae_train_step against the stock PyTorch-ROCm step of the same modules, and the frozen fused pair.  Bounds: tests/test_hip_ae_train.py's."""
import copy

import pytest
import torch

import ae3d_cases as AC
import golden_cases as GC
from oracle import ops as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNEL_TOL = 1e-5                                    # hand-written kernels vs float64, no MIOpen involved
GRAD_TOL, LOSS_TOL, NORM_TOL = 5e-3, 1e-4, 0.15      # MIOpen convolutions and ReLU kinks in the path (tests/test_hip_ae_train.py)
ZERO_GRAD = AC.ZERO_GRAD
BLOCK_SEED, PAIR_SEED = 310, 410
# one learn_3d=False step of the KTH pair, (B, T, S) = (2, 4, 64), the second of a run: kernels launched through the C ABI, counted with
# the parent commit's package and with this one in the same GPU session (both 222)
PARENT_LAUNCHES_AE64 = 222
rel = AC.rel


@pytest.fixture(scope="module")
def npvp():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import npvp_amd
    return npvp_amd


def worst_row(got, want):
    """largest row error, each row against the larger of its own norm and the tensor's RMS row norm (a row's rounding error scales with
    the operands that were summed, not with what is left after they cancel: dq rows near 0 are held to the typical row)"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    rn = want.norm(dim=1)
    floor = (want.norm() / want.shape[0] ** 0.5).clamp_min(1e-30)
    return float(((got - want).norm(dim=1) / torch.maximum(rn, floor)).max())


def _run_packed(npvp, q, k, v, go, N, T, HW, ld=None):
    A, V = q.shape[1], v.shape[1]
    ld = ld or 2 * A + V
    qkv = torch.zeros(q.shape[0], ld)
    qkv[:, :A], qkv[:, A:2 * A], qkv[:, 2 * A:2 * A + V] = q, k, v
    leaf = qkv.to(DEV).requires_grad_()
    o = npvp.ops.temporal_attn_packed(leaf, N, T, HW, A, V)
    o.backward(go.to(DEV))
    g = leaf.grad
    return o.detach(), g[:, :A], g[:, A:2 * A], g[:, 2 * A:2 * A + V], g[:, 2 * A + V:]


def _assert_close(got, want, what):
    for name, g, w in zip(("o", "dq", "dk", "dv"), got, want):
        e, r = rel(g, w), worst_row(g, w)
        print(f"{what} {name}: rel-L2 {e:.2e} worst row {r:.2e}")
        assert e < KERNEL_TOL and r < KERNEL_TOL, (what, name, e, r)


# ------------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("T", [1, 2, 3, 9, 32])
@pytest.mark.parametrize("A,V", AC.DIMS)
def test_temporal_attn_vs_float64(npvp, A, V, T):
    N, HW = 2, 5
    q, k, v, go = AC.kernel_inputs(A, V, N, T, HW)
    want = AC.temporal_attn_ref64(q, k, v, go, N, T, HW)
    got = _run_packed(npvp, q, k, v, go, N, T, HW)
    if T == 1:          # softmax over one frame: exact
        assert torch.equal(got[0].cpu(), v) and torch.equal(got[3].cpu(), go)
        assert float(got[1].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0
    _assert_close(got[:4], want, f"({A},{V}) T={T}")


@pytest.mark.parametrize("HW", [1, 15, 16, 17, 64 + 3])
def test_temporal_attn_pixel_tiles(npvp, HW):
    """(8, 32) at T = 5 takes 16 pixels per workgroup: the last tile of a clip partial, exact, one over; 67 spans four full tiles"""
    N, T, A, V = 2, 5, 8, 32
    q, k, v, go = AC.kernel_inputs(A, V, N, T, HW, seed=520)
    _assert_close(_run_packed(npvp, q, k, v, go, N, T, HW)[:4], AC.temporal_attn_ref64(q, k, v, go, N, T, HW), f"HW={HW}")


def test_temporal_attn_wide_tile_and_unpacked(npvp):
    """(64, 256) at T = 32: one pixel per workgroup, two 128-column chunks of v; through ops.temporal_attn on (M, T, d) sequences"""
    M, T, A, V = 3, 32, 64, 256
    q, k, v, go = AC.kernel_inputs(A, V, 1, T, M, seed=530)          # rows = t M + m
    want = AC.temporal_attn_ref64(q, k, v, go, 1, T, M)
    seq = lambda t: t.reshape(T, M, -1).transpose(0, 1).contiguous().to(DEV).requires_grad_()
    qs, ks, vs = seq(q), seq(k), seq(v)
    o = npvp.ops.temporal_attn(qs, ks, vs, T)
    o.backward(go.reshape(T, M, V).transpose(0, 1).to(DEV))
    rows = lambda t: t.detach().transpose(0, 1).reshape(T * M, -1)
    _assert_close((rows(o), rows(qs.grad), rows(ks.grad), rows(vs.grad)), want, "unpacked (64,256) T=32")


def test_temporal_attn_padded_packed_rows(npvp):
    """ld = 2A+V rounded up to 32 (what the model's GEMM hands over): the gradient's pad columns are exactly zero"""
    N, T, HW, A, V = 2, 3, 7, 8, 32
    q, k, v, go = AC.kernel_inputs(A, V, N, T, HW, seed=540)
    got = _run_packed(npvp, q, k, v, go, N, T, HW, ld=64)
    _assert_close(got[:4], AC.temporal_attn_ref64(q, k, v, go, N, T, HW), "ld=64")
    assert got[4].shape[1] == 16 and float(got[4].abs().max()) == 0.0


def test_temporal_attn_overflow_needs_the_max(npvp):
    """q = k with squared norm 120 at one pixel and frame: exp(120) overflows fp32, the max-subtracted softmax does not"""
    N, T, HW, A, V = 2, 3, 5, 16, 64
    q, k, v, go = AC.kernel_inputs(A, V, N, T, HW, seed=550)
    r = (0 * T + 1) * HW + 2
    q[r] = k[r] = torch.full((A,), (120.0 / A) ** 0.5)
    got = _run_packed(npvp, q, k, v, go, N, T, HW)
    assert all(torch.isfinite(t).all() for t in got)
    _assert_close(got[:4], AC.temporal_attn_ref64(q, k, v, go, N, T, HW), "overflow")


def _c_abi_call(npvp, bufs, lds, N, T, HW, A, V):
    """forward + backward through the C ABI on explicit pointers: bufs / lds = (q, k, v, o, go, dq, dk, dv) and their leading dimensions"""
    L = npvp._lib.lib()
    q, k, v, o, go, dq, dk, dv = (b.data_ptr() for b in bufs)
    lq, lk, lv, lo, lg, ldq, ldk, ldv = lds
    lse = torch.empty(N * T * HW, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    rc = L.npvp_temporal_attn_fwd(q, lq, k, lk, v, lv, o, lo, lse.data_ptr(), N, T, HW, A, V, st)
    assert rc == 0, L.npvp_last_error()
    rc = L.npvp_temporal_attn_bwd(q, lq, k, lk, v, lv, go, lg, lse.data_ptr(), dq, ldq, dk, ldk, dv, ldv, N, T, HW, A, V, st)
    assert rc == 0, L.npvp_last_error()
    torch.cuda.synchronize()
    return lse


def test_temporal_attn_separate_buffers_and_poison(npvp):
    """q / k / v / o / go / dq / dk / dv in buffers of their own, each with another leading dimension, each inside a larger buffer:
    NaN around the inputs (none is read: every result is finite and right), a bit pattern around the outputs (none is changed)"""
    N, T, HW, A, V = 2, 5, 17, 8, 32
    R = N * T * HW
    q, k, v, go = AC.kernel_inputs(A, V, N, T, HW, seed=560)
    want = AC.temporal_attn_ref64(q, k, v, go, N, T, HW)
    PAT = -1.2345e33
    GUARD = 8                                             # rows in front of and behind the operand

    def embed(t, ld, fill):
        buf = torch.full((R + 2 * GUARD, ld), fill)
        if t is not None:
            buf[GUARD:GUARD + R, :t.shape[1]] = t
        return buf.to(DEV)
    nan = float("nan")
    ins = [embed(q, 12, nan), embed(k, 16, nan), embed(v, 36, nan), embed(go, 40, nan)]
    outs = [embed(None, 44, PAT), embed(None, 8, PAT), embed(None, 20, PAT), embed(None, 32, PAT)]         # o, dq, dk, dv
    body = lambda b: b[GUARD:GUARD + R]
    bufs = [body(ins[0]), body(ins[1]), body(ins[2]), body(outs[0]), body(ins[3]), body(outs[1]), body(outs[2]), body(outs[3])]
    _c_abi_call(npvp, bufs, (12, 16, 36, 44, 40, 8, 20, 32), N, T, HW, A, V)
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


def test_clips_and_pixels_do_not_mix_and_runs_repeat(npvp):
    N, T, HW, A, V = 2, 4, 6, 32, 128
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


# -------------------------------------------------------------------------------------------------------------------- the block
class _OneBlock(torch.nn.Module):
    def __init__(self, blk):
        super().__init__()
        self.blk = blk


@pytest.mark.parametrize("cf", [True, False], ids=["conv", "attn"])
@pytest.mark.parametrize("N,T,H,W", AC.BLOCK_CASES)
def test_block_through_the_trainable_path(npvp, N, T, H, W, cf):
    """Factorized3DConvAttn(64, learn_3d=True) through models/ae_train._fact on channels-last frames against the reference fixture:
    output and running statistics at the suite's golden bar (1e-4), gradients at GRAD_TOL and per tensor at NORM_TOL, then eval"""
    from npvp_amd.models import Factorized3DConvAttn
    from npvp_amd.models.ae_train import _fact
    gold, tag = GC.load(AC.block_file(N, T, H, W)), AC.block_tag(N, T, H, W, cf)
    blk = O.key_hashed_fill(Factorized3DConvAttn(AC.BLOCK_C, conv_first=cf, learn_3d=True), BLOCK_SEED).to(DEV)
    blk = blk.to(memory_format=torch.channels_last)
    x, cot = AC.block_input(N, T, H, W)
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
        assert ng > 0 and abs(nh - ng) <= NORM_TOL * ng, (n, nh, ng)
        got.append(p.grad.reshape(-1).cpu()); want.append(g.reshape(-1))
    got[0] = got[0].cpu()
    assert rel(torch.cat(got), torch.cat(want)) < GRAD_TOL


# --------------------------------------------------------------------------------------------------------------------- the step
def _pair(npvp, AE, ch, seed):
    enc, dec = npvp.build_autoencoder(AE, ch)
    O.key_hashed_fill(npvp.AEPair(enc, dec), seed)
    return enc, dec


def _frames(B, T, ch, S, seed):
    x = torch.tanh(O.seeded_randn((B, T, ch, S, S), seed))
    return x[:, : T // 2].contiguous().to(DEV), x[:, T // 2:].contiguous().to(DEV)


def _stock_step(enc, dec, opt, past, fut):
    opt.zero_grad()
    x = torch.cat([past, fut], 1)
    loss = (dec(enc(x)) - x).abs().mean()
    loss.backward()
    opt.step()
    return loss.detach()


@pytest.mark.parametrize("cfg", ["small", "64"])
def test_ae3d_train_step_matches_stock(npvp, cfg):
    """tests/test_hip_ae_train.py::test_ae_train_step_matches_stock with learn_3d=True: 3 steps of the HIP path and of the stock path
    from the same weights and frames - losses, step-1 gradients, parameters and running statistics after step 3"""
    AE, ch, B, T, S = (AC.AE_SMALL, 1, 2, 4, 8) if cfg == "small" else (AC.AE64_3D, 1, 2, 4, 64)
    enc, dec = _pair(npvp, AE, ch, 7)
    s_enc, s_dec = copy.deepcopy(enc).to(DEV), copy.deepcopy(dec).to(DEV)
    enc, dec = enc.to(DEV).to(memory_format=torch.channels_last), dec.to(DEV)
    npvp.prepare_trainable_autoencoder(enc, dec)
    opt = npvp.ae_optimizer(enc, dec, lr=1e-4)
    s_opt = torch.optim.Adam(list(s_enc.parameters()) + list(s_dec.parameters()), lr=1e-4, betas=(0.5, 0.999))
    s_pair = npvp.AEPair(s_enc, s_dec)
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
    past, fut = _frames(B, T, ch, S, 70)
    lv, rec = npvp.ae_val_step(enc, dec, past, fut)
    s_enc.eval(); s_dec.eval()
    with torch.no_grad():
        x = torch.cat([past, fut], 1)
        lvs = (s_dec(s_enc(x)) - x).abs().mean()
    assert abs(float(lv) - float(lvs)) <= LOSS_TOL * abs(float(lvs)) and enc.training and dec.training


def test_learn_3d_false_step_is_the_parents(npvp):
    """the learn_3d=False step does not depend on the new code: the same loss bits on two runs, no temporal kernel among its launches,
    and as many launches through the C ABI as the parent commit makes for this step (counted there, see PARENT_LAUNCHES_AE64).
    MIOpen's default solvers are not bit-reproducible from one run to the next, on the parent commit either (measured: the encoder's
    output moved in every one of ten runs of a fresh pair, the first-step loss by up to 2 ulp), so the two runs ask MIOpen for its
    deterministic solvers (torch.backends.cudnn.deterministic); with them the losses of BOTH steps - the second follows a whole
    backward pass and an optimiser step - repeated bit for bit in twenty runs.  Everything else in the step is this library's."""
    AE = dict(AC.AE64_3D, learn_3d=False)
    L = npvp._lib.lib()
    called = []
    real = npvp.ops.temporal_attn_packed
    npvp.ops.temporal_attn_packed = lambda *a, **k: called.append(1) or real(*a, **k)
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        runs = []
        for _ in range(2):
            enc, dec = _pair(npvp, AE, 1, 7)
            enc, dec = enc.to(DEV).to(memory_format=torch.channels_last), dec.to(DEV)
            npvp.prepare_trainable_autoencoder(enc, dec)
            opt = npvp.ae_optimizer(enc, dec, lr=1e-4)
            past, fut = _frames(2, 4, 1, 64, 60)
            loss0 = npvp.ae_train_step(enc, dec, opt, past, fut)             # (first step: one-time setup launches)
            torch.cuda.synchronize()
            n0 = L.npvp_launch_count()
            loss1 = npvp.ae_train_step(enc, dec, opt, past, fut)
            torch.cuda.synchronize()
            runs.append((L.npvp_launch_count() - n0, float(loss0).hex(), float(loss1).hex()))
    finally:
        npvp.ops.temporal_attn_packed = real
        torch.backends.cudnn.deterministic = det
    print("learn_3d=False step: (launches, loss bits of steps 1 and 2)", runs)
    assert not called and runs[0] == runs[1]
    assert runs[0][0] == PARENT_LAUNCHES_AE64, runs


# -------------------------------------------------------------------------------------------------------------- the frozen pair
def test_frozen_fused_pair(npvp):
    """build_frozen_autoencoder(learn_3d=True) + to_device_layout: the fused eval encoder against the unfused stock eval encoder and
    against the reference fixture, at tests/test_hip_golden.py::test_frozen_autoencoder's forward bar (1e-4)"""
    gold = GC.load("ae3d_pair")
    enc, dec = npvp.build_frozen_autoencoder(AC.AE_SMALL, 1)
    O.key_hashed_fill(npvp.AEPair(enc, dec), PAIR_SEED)
    frames = AC.pair_frames().to(DEV)
    s_enc = copy.deepcopy(enc).to(DEV).eval()
    fe, fd = npvp.to_device_layout(enc, dec, DEV)
    n0 = npvp._lib.lib().npvp_launch_count()
    with torch.no_grad():
        got, stock = fe(frames), s_enc(frames)
        rec = fd(got)
    assert npvp._lib.lib().npvp_launch_count() > n0
    assert rel(got, stock) < 1e-4 and rel(got, gold["enc_eval"]) < 1e-4, (rel(got, stock), rel(got, gold["enc_eval"]))
    assert torch.isfinite(rec).all() and rec.shape == frames.shape


def test_full_val_step_with_a_3d_pair(npvp):
    enc, dec = npvp.build_frozen_autoencoder(dict(AC.AE64_3D, out_layer='Sigmoid'), 1)
    O.key_hashed_fill(enc, 121); O.key_hashed_fill(dec, 122)
    enc, dec = npvp.to_device_layout(enc, dec, DEV)
    m = GC._small_predictor(npvp, False, 151, DEV)
    g_ = torch.Generator().manual_seed(153)
    pf, ff = torch.rand(1, 3, 1, 64, 64, generator=g_).to(DEV), torch.rand(1, 4, 1, 64, 64, generator=g_).to(DEV)
    s = npvp.full_val_step(m, enc, dec, pf, ff, 0.01, 1e-6)
    for k in ("loss", "Image_L1", "PF_L1"):
        assert torch.isfinite(torch.as_tensor(s[k])).all(), k
    assert s["pred"].shape[:2] == (1, 4) and torch.isfinite(s["pred"]).all()
