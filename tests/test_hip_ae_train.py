"""GPU: the Stage-1 autoencoder training path (csrc/ae_train.hip, ops.bn_act_train / nonlocal_attn / reflect_pad,
prepare_trainable_autoencoder, ae_train_step) against float64 CPU references and against the stock PyTorch-ROCm step."""
import copy

import pytest
import torch
import torch.nn.functional as F

from oracle import ops as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNEL_TOL = 1e-5        # hand-written kernels vs float64, no MIOpen involved


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def npvp():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import npvp_amd
    return npvp_amd


def _bn_ref(x, w, b, res, act, rm, rv):
    y = F.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-5)
    if act:
        y = torch.relu(y)
    return y + res if res is not None else y


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
@pytest.mark.parametrize("layout", ["channels_last", "nchw"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("shape", [(3, 64, 3, 3), (5, 32, 6, 6), (4, 512, 8, 8), (2, 128, 32, 32)])
def test_bn_act_train_vs_float64(npvp, layout, act, with_res, shape):
    """forward, backward (x, weight, bias, residual) and the running-statistic update; odd row / plane counts included"""
    N, C, H, W = shape
    if layout == "nchw" and H * W % 4:           # (planes of H*W % 4 == 0; the odd count is then the planes')
        W += 1
        shape = (N, C, H, W)
    x = O.seeded_randn(shape, 1) * 1.7 + 0.6
    w, b = 1 + 0.1 * O.seeded_randn((C,), 2), 0.1 * O.seeded_randn((C,), 3)
    res = O.seeded_randn(shape, 4) if with_res else None
    g = O.seeded_randn(shape, 5)
    rm, rv = 0.1 * O.seeded_randn((C,), 6), 0.5 + O.seeded_randn((C,), 7).abs()
    xd, wd, bd = (t.double().requires_grad_() for t in (x, w, b))
    rd = res.double().requires_grad_() if with_res else None
    rmd, rvd = rm.double(), rv.double()
    yd = _bn_ref(xd, wd, bd, rd, act, rmd, rvd)
    yd.backward(g.double())
    mf = torch.channels_last if layout == "channels_last" else torch.contiguous_format
    xg = x.to(DEV).contiguous(memory_format=mf).requires_grad_()
    wg, bg = w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    rg = res.to(DEV).contiguous(memory_format=mf).requires_grad_() if with_res else None
    rmg, rvg = rm.to(DEV), rv.to(DEV)
    yg = npvp.ops.bn_act_train(xg, wg, bg, rmg, rvg, 0.1, 1e-5, act, True, rg)
    yg.backward(g.to(DEV).contiguous(memory_format=mf))
    assert rel(yg, yd) < KERNEL_TOL
    assert rel(xg.grad, xd.grad) < KERNEL_TOL
    assert rel(wg.grad, wd.grad) < KERNEL_TOL and rel(bg.grad, bd.grad) < KERNEL_TOL
    if with_res:
        assert rel(rg.grad, rd.grad) < KERNEL_TOL
    assert rel(rmg, rmd) < KERNEL_TOL and rel(rvg, rvd) < KERNEL_TOL


@pytest.mark.parametrize("layout", ["channels_last", "nchw"])
def test_bn_eval_uses_running_statistics(npvp, layout):
    N, C, H, W = 3, 64, 4, 4
    x = O.seeded_randn((N, C, H, W), 11)
    w, b = 1 + 0.1 * O.seeded_randn((C,), 12), 0.1 * O.seeded_randn((C,), 13)
    rm, rv = 0.1 * O.seeded_randn((C,), 14), 0.5 + O.seeded_randn((C,), 15).abs()
    xd, wd, bd = (t.double().requires_grad_() for t in (x, w, b))
    yd = torch.relu(F.batch_norm(xd, rm.double(), rv.double(), wd, bd, False, 0.1, 1e-5))
    g = O.seeded_randn((N, C, H, W), 16)
    yd.backward(g.double())
    mf = torch.channels_last if layout == "channels_last" else torch.contiguous_format
    xg = x.to(DEV).contiguous(memory_format=mf).requires_grad_()
    wg, bg = w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    rmg, rvg = rm.to(DEV), rv.to(DEV)
    yg = npvp.ops.bn_act_train(xg, wg, bg, rmg, rvg, 0.1, 1e-5, 1, False)
    yg.backward(g.to(DEV).contiguous(memory_format=mf))
    assert rel(yg, yd) < KERNEL_TOL and rel(xg.grad, xd.grad) < KERNEL_TOL and rel(wg.grad, wd.grad) < KERNEL_TOL
    assert torch.equal(rmg.cpu(), rm) and torch.equal(rvg.cpu(), rv)          # eval leaves the running statistics alone


# ------------------------------------------------------------------------------------------------------- non-local attention
def _attn_ref(q, k, v, H, W):
    Fr, P, A = q.shape
    pool = lambda t: F.max_pool2d(t.transpose(1, 2).reshape(Fr, t.shape[-1], H, W), 2, 2).flatten(2)    # (F, d, HW/4)
    att = torch.softmax(q @ pool(k), dim=-1)
    return att @ pool(v).transpose(1, 2)


NL_SHAPES = [(64, 64), (128, 32), (256, 16), (512, 8)]       # (C, grid): every (C, grid) pair of the five AE configs
# (C, H, W) the config kernels also take (H even, W a power of two, the config's cell count) that are not square: the smallest with
# one pooled row (Hp = 1), with one pooled column (Wp = 1: the window decode's shift is 0), and with W != sqrt(HW)
NL_RECT = [(512, 2, 32), (512, 32, 2), (128, 16, 64)]
NL_CASES = [pytest.param(C, S, S, id=f"{C}-{S}") for C, S in NL_SHAPES] + [pytest.param(C, H, W, id=f"{C}-{H}x{W}") for C, H, W in NL_RECT]


def _nl_inputs(C, H, W, Fr, seed, tie=False):
    A, V = C // 8, C // 2
    q = O.seeded_randn((Fr, H * W, A), seed) * (1.5 / A ** 0.5)
    k = O.seeded_randn((Fr, H * W, A), seed + 1)
    v = O.seeded_randn((Fr, H * W, V), seed + 2)
    if tie:       # whole windows of equal values (a post-ReLU zero pixel gives exactly the bias): the first element must win
        k[0, 1] = k[0, 0]; v[0, 1] = v[0, 0]
        k[0, W] = k[0, 0]; v[0, W + 1] = v[0, W]
        k[1, W + 1] = k[1, W]; k[1, 1] = k[1, W]
    return q, k, v


@pytest.mark.parametrize("C,H,W", NL_CASES)
@pytest.mark.parametrize("tie", [False, True])
def test_nonlocal_attn_vs_float64(npvp, C, H, W, tie):
    q, k, v = _nl_inputs(C, H, W, 2, 20 + C, tie)
    go = O.seeded_randn((2, H * W, C // 2), 30 + C)
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    od = _attn_ref(qd, kd, vd, H, W)
    od.backward(go.double())
    qg, kg, vg = (t.to(DEV).requires_grad_() for t in (q, k, v))
    og = npvp.ops.nonlocal_attn(qg, kg, vg, H, W)
    og.backward(go.to(DEV))
    assert rel(og, od) < KERNEL_TOL
    for a, b in ((qg.grad, qd.grad), (kg.grad, kd.grad), (vg.grad, vd.grad)):
        assert rel(a, b) < KERNEL_TOL
    if tie:    # exactly where torch routes the window's gradient: the tied later elements get none
        assert torch.equal(kg.grad.cpu() == 0, kd.grad == 0) and torch.equal(vg.grad.cpu() == 0, vd.grad == 0)
        assert float(kg.grad[0, 1].abs().max()) == 0.0 and float(vg.grad[0, 1].abs().max()) == 0.0


def test_nonlocal_attn_rejects_other_shapes(npvp):
    q = torch.zeros(1, 36, 8, device=DEV)
    with pytest.raises(RuntimeError):
        npvp.ops.nonlocal_attn(q, q, torch.zeros(1, 36, 32, device=DEV), 6, 6)
    with pytest.raises(RuntimeError):
        npvp.ops.nonlocal_attn(torch.zeros(1, 64, 12, device=DEV), torch.zeros(1, 64, 12, device=DEV), torch.zeros(1, 64, 48, device=DEV), 8, 8)


# --------------------------------------------------------------------------------------------------------- reflection pad
@pytest.mark.parametrize("layout", ["channels_last", "nchw"])
@pytest.mark.parametrize("P,shape", [(3, (3, 3, 16, 16)), (3, (2, 32, 8, 8)), (1, (2, 512, 8, 8)), (3, (1, 64, 4, 6))])
def test_reflect_pad_vs_float64(npvp, layout, P, shape):
    x = O.seeded_randn(shape, 40)
    g = O.seeded_randn((shape[0], shape[1], shape[2] + 2 * P, shape[3] + 2 * P), 41)
    xd = x.double().requires_grad_()
    yd = F.pad(xd, (P, P, P, P), mode="reflect")
    yd.backward(g.double())
    mf = torch.channels_last if layout == "channels_last" else torch.contiguous_format
    xg = x.to(DEV).contiguous(memory_format=mf).requires_grad_()
    yg = npvp.ops.reflect_pad(xg, P)
    yg.backward(g.to(DEV).contiguous(memory_format=mf))
    assert torch.equal(yg.cpu(), yd.float().detach())
    assert rel(xg.grad, xd.grad) < KERNEL_TOL


# ------------------------------------------------------------------------------------------------------------ determinism
def test_new_kernels_are_bit_reproducible(npvp):
    def run():
        outs = []
        x = (O.seeded_randn((6, 128, 16, 16), 50) + 0.3).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
        w, b = torch.ones(128, device=DEV, requires_grad=True), torch.zeros(128, device=DEV, requires_grad=True)
        rm, rv = torch.zeros(128, device=DEV), torch.ones(128, device=DEV)
        y = npvp.ops.bn_act_train(x, w, b, rm, rv, 0.1, 1e-5, 1, True, x)
        y.backward(O.seeded_randn(y.shape, 51).to(DEV).contiguous(memory_format=torch.channels_last))
        outs += [y, x.grad, w.grad, b.grad, rm, rv]
        xn = O.seeded_randn((5, 64, 32, 32), 52).to(DEV).requires_grad_()
        yn = npvp.ops.bn_act_train(xn, w[:64].detach().clone().requires_grad_(), b[:64].detach().clone(), None, None, 0.1, 1e-5, 0, True)
        yn.backward(O.seeded_randn(yn.shape, 53).to(DEV))
        outs += [yn, xn.grad]
        q, k, v = (t.to(DEV).requires_grad_() for t in _nl_inputs(64, 64, 64, 2, 54))
        o = npvp.ops.nonlocal_attn(q, k, v, 64, 64)
        o.backward(O.seeded_randn(o.shape, 55).to(DEV))
        outs += [o, q.grad, k.grad, v.grad]
        xp = O.seeded_randn((2, 32, 16, 16), 56).to(DEV).requires_grad_()
        yp = npvp.ops.reflect_pad(xp, 3)
        yp.backward(O.seeded_randn(yp.shape, 57).to(DEV))
        outs += [yp, xp.grad]
        return [t.detach().cpu().clone() for t in outs]
    a, b = run(), run()
    for i, (u, w) in enumerate(zip(a, b)):
        assert torch.equal(u, w), i


# ------------------------------------------------------------------------------------------------------ the training step
AE64 = dict(ngf=64, n_downsampling=3, num_res_blocks=2, out_layer='Tanh', learn_3d=False)
AE128 = dict(ngf=32, n_downsampling=4, num_res_blocks=3, out_layer='Tanh', learn_3d=False)
# Gradients and updated parameters pass through MIOpen convolutions and ReLU masks: a few units within rounding noise of 0 flip with
# MIOpen's algorithm choice, each a finite gradient change - the bound tests/test_hip_golden.py::test_frozen_autoencoder uses for the
# decoder's input gradient (5e-3 rel-L2) holds for the whole pair's gradient and for every parameter and running statistic after 3
# steps.  Gradients are not compared tensor by tensor: small ones next to the input collect the flips of every ReLU above them and
# moved from run to run of the same code (an encoder BatchNorm weight gradient: 8e-3 in one run, 4.6e-2 in another, within bound
# in a third; a scalar gamma's, one sum whose terms cancel to ~1e-5: 7 %).  Losses: the suite's 1e-4.
# Per tensor, the gradient NORM is held to NORM_TOL: those flips moved a BatchNorm weight gradient by 4.6e-2 rel-L2 and a scalar gamma's
# (one sum whose terms cancel to ~1e-5) by 7.3 % between paths; a glue error in a small tensor (gamma, Wq / Wk, the attention's
# BatchNorm) moves its norm by O(1).
GRAD_TOL, LOSS_TOL, NORM_TOL = 5e-3, 1e-4, 0.15
# Parameters whose exact gradient is 0, each a per-channel constant that a training-mode BatchNorm or a softmax removes: the bias of
# the convolution right before a BatchNorm; the key bias (it adds q.b to every score of a row: the softmax removes it); the value
# bias (it adds b to every row of o, the rows of P summing to 1) and out_proj's bias (both reach the BatchNorm after out_proj as a
# per-channel constant).  Both paths give rounding noise there (~1e-10), and Adam turns that noise into steps of +-lr.
ZERO_GRAD = ("spatial_conv.0.bias", "attn2d.Wk.bias", "attn2d.Wv.bias", "attn2d.out_proj.bias")


def _pair(npvp, AE, ch, seed):
    enc, dec = npvp.build_autoencoder(AE, ch)
    pair = npvp.AEPair(enc, dec)
    O.key_hashed_fill(pair, seed)         # (gamma = 0.1 randn: the attention weights and their BatchNorm get gradients)
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


@pytest.mark.parametrize("cfg", ["64", "128"])
def test_ae_train_step_matches_stock(npvp, cfg):
    """3 steps of the HIP path and of the stock path (same modules in train mode + torch.optim.Adam(betas=(0.5, 0.999))) from the
    same weights and frames: losses, gradients of step 1, parameters and BatchNorm running statistics after step 3"""
    AE, ch, B, T, S = (AE64, 1, 2, 4, 64) if cfg == "64" else (AE128, 3, 1, 2, 128)
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
            hg, sg = [], []
            for (n, p), (_, q) in zip(opt.ae_pair.named_parameters(), s_pair.named_parameters()):
                hg.append(p.grad.reshape(-1)); sg.append(q.grad.reshape(-1))
                if n.endswith(ZERO_GRAD):
                    assert float(p.grad.abs().max()) < 1e-6 and float(q.grad.abs().max()) < 1e-6
                    continue
                assert q.grad is not None and float(q.grad.norm()) > 0.0, n       # (gamma != 0: every parameter gets a gradient)
                nh, ns = float(p.grad.double().norm()), float(q.grad.double().norm())
                assert abs(nh - ns) <= NORM_TOL * ns, (n, nh, ns)
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
    # validation: eval mode, running statistics; modes restored
    past, fut = _frames(B, T, ch, S, 70)
    lv, rec = npvp.ae_val_step(enc, dec, past, fut)
    s_enc.eval(); s_dec.eval()
    with torch.no_grad():
        x = torch.cat([past, fut], 1)
        lvs = (s_dec(s_enc(x)) - x).abs().mean()
    assert abs(float(lv) - float(lvs)) <= LOSS_TOL * abs(float(lvs)) and enc.training and dec.training


@pytest.mark.parametrize("tag", ["64", "128"])
def test_ae_train_step_vs_reference_fixture(npvp, tag):
    """two steps of ae_train_step against the reference LitAE's own two steps (tests/golden/ae_train_{tag}.npz, KTH / KITTI pair):
    losses, per-parameter gradient norms and gradient heads of step 1, BatchNorm running statistics after step 1, parameter heads
    after steps 1 and 2; bounds as in test_ae_train_step_matches_stock"""
    import ae_train_cases as AC
    import golden_cases as GC
    gold = GC.load(f"ae_train_{tag}")
    ci, AE = AC.CASES[tag][:2]
    torch.manual_seed(0)
    enc, dec = npvp.build_autoencoder(AE, ci)
    AC.fill(npvp.AEPair(enc, dec))
    enc, dec = enc.to(DEV).to(memory_format=torch.channels_last), dec.to(DEV)
    npvp.prepare_trainable_autoencoder(enc, dec)
    opt = npvp.ae_optimizer(enc, dec, lr=AC.LR)
    assert list(AC.param_names(opt.ae_pair)) == list(gold["param_names"])
    assert list(AC.state_keys(opt.ae_pair)) == list(gold["state_keys"])
    res = AC.record(opt.ae_pair, lambda p, f: npvp.ae_train_step(enc, dec, opt, p, f), tag, DEV)
    for k in ("loss_0", "loss_1"):
        assert abs(float(res[k]) - float(gold[k])) <= LOSS_TOL * abs(float(gold[k])), (k, float(res[k]), float(gold[k]))
    keep = [i for i, n in enumerate(gold["param_names"]) if not str(n).endswith(ZERO_GRAD)]
    for i, n in enumerate(gold["param_names"]):
        nh, ng = float(res["grad_norm"][i]), float(gold["grad_norm"][i])
        if i in keep:
            assert abs(nh - ng) <= NORM_TOL * ng, (str(n), nh, ng)
        else:
            assert nh < 1e-6 and ng < 1e-6, (str(n), nh, ng)
    assert rel(res["grad_head"][keep], torch.as_tensor(gold["grad_head"][keep])) < GRAD_TOL
    assert rel(res["running"], torch.as_tensor(gold["running"])) < 1e-3         # forward only: MIOpen vs CPU convolutions
    for k in ("param_head_0", "param_head_1"):
        for i in keep:
            assert rel(res[k][i], torch.as_tensor(gold[k][i])) < GRAD_TOL, (k, str(gold["param_names"][i]))


def test_ae_step_peak_memory_below_stock(npvp):
    """one 128x128 step (the KITTI pair, 8 frames): the HIP path's peak allocation stays below the stock path's (the stock
    attention keeps its 4096 x 1024 score and softmax matrices per frame for the backward)"""
    past, fut = _frames(2, 4, 3, 128, 80)

    def peak(run):
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    enc, dec = _pair(npvp, AE128, 3, 9)
    s_enc, s_dec = copy.deepcopy(enc).to(DEV), copy.deepcopy(dec).to(DEV)
    s_opt = torch.optim.Adam(list(s_enc.parameters()) + list(s_dec.parameters()), lr=1e-4, betas=(0.5, 0.999))
    _stock_step(s_enc, s_dec, s_opt, past, fut)           # (Adam's state allocated before the measured step, as FlatAdamW's)
    p_stock = peak(lambda: _stock_step(s_enc, s_dec, s_opt, past, fut))
    del s_enc, s_dec, s_opt
    enc, dec = enc.to(DEV).to(memory_format=torch.channels_last), dec.to(DEV)
    npvp.prepare_trainable_autoencoder(enc, dec)
    opt = npvp.ae_optimizer(enc, dec)
    npvp.ae_train_step(enc, dec, opt, past, fut)
    p_hip = peak(lambda: npvp.ae_train_step(enc, dec, opt, past, fut))
    assert p_hip < p_stock, (p_hip, p_stock)


def test_checkpoint_after_training_loads_into_frozen_pair(npvp, tmp_path):
    enc, dec = _pair(npvp, AE64, 1, 3)
    enc, dec = enc.to(DEV).to(memory_format=torch.channels_last), dec.to(DEV)
    npvp.prepare_trainable_autoencoder(enc, dec)
    opt = npvp.ae_optimizer(enc, dec)
    past, fut = _frames(1, 2, 1, 64, 90)
    npvp.ae_train_step(enc, dec, opt, past, fut)
    path = str(tmp_path / "ae.ckpt")
    npvp.save_ae_checkpoint(path, enc, dec, opt, epoch=0, global_step=1)
    fe, fd = npvp.build_frozen_autoencoder(AE64, 1)
    assert npvp.load_lightning_checkpoint(path, None, fe, fd) == (0, 1)
    for a, b in ((fe, enc), (fd, dec)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        assert all(torch.equal(sa[k].cpu(), sb[k].cpu()) for k in sa)
    fe, fd = npvp.to_device_layout(fe, fd, DEV)
    with torch.no_grad():
        assert torch.isfinite(fd(fe(past))).all()
    # the optimiser state comes back too
    enc2, dec2 = npvp.build_autoencoder(AE64, 1)
    enc2, dec2 = enc2.to(DEV).to(memory_format=torch.channels_last), dec2.to(DEV)
    opt2 = npvp.ae_optimizer(enc2, dec2)
    assert npvp.load_ae_checkpoint(path, enc2, dec2, opt2) == (0, 1)
    assert torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v) and float(opt2.hyper[1]) == 1.0
