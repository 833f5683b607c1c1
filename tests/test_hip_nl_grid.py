"""GPU: non-local attention on any grid (npvp_nonlocal_attn_grid_fwd / _bwd, ops.nonlocal_attn_grid / _packed) against float64, and
the Stage-1 step at a frame size no config has (48x80: attentions at 24x40, 12x20, 6x10 and the odd 3x5) against the stock path
and against the reference LitAE's own two steps (tests/golden/ae_train_rect.npz).

Shapes are the smallest that reach each tail of the NL<A, V> tiles (V: QT / KT query and key tiles of the forward and dq kernels,
KB / QB key and query tiles of the dk / dv kernel):  32: 128 / 64, 128 / 16;  64: 64 / 64, 64 / 32;  128: 32 / 64, 32 / 32;
256: 16 / 16, 16 / 16."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import ae_rect_cases as RC
import golden_cases as GC
from oracle import ops as O
from test_hip_ae_train import GRAD_TOL, KERNEL_TOL, LOSS_TOL, NORM_TOL, ZERO_GRAD, _stock_step, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def npvp():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import npvp_amd
    return npvp_amd


def _attn_ref(q, k, v, H, W):
    """NonLocalAttenion2D's core: nn.MaxPool2d((2, 2), stride=2) pools floor(H/2) x floor(W/2) windows, an odd last line / column
    is in none"""
    Fr = q.shape[0]
    pool = lambda t: F.max_pool2d(t.transpose(1, 2).reshape(Fr, t.shape[-1], H, W), 2, 2).flatten(2)    # (F, d, Hp*Wp)
    att = torch.softmax(q @ pool(k), dim=-1)
    return att @ pool(v).transpose(1, 2)


def _nl_inputs(C, H, W, Fr, seed, tie=False):
    A, V = C // 8, C // 2
    q = O.seeded_randn((Fr, H * W, A), seed) * (1.5 / A ** 0.5)
    k = O.seeded_randn((Fr, H * W, A), seed + 1)
    v = O.seeded_randn((Fr, H * W, V), seed + 2)
    if tie:       # whole windows of equal values: the first element (row-major window order) must win.  Every row is inside a window.
        last = (2 * (H // 2) - 2) * W + 2 * (W // 2) - 2           # first row of the LAST window (last pooled line and column)
        k[0, 1] = k[0, 0]; v[0, 1] = v[0, 0]
        k[0, W] = k[0, 0]; v[0, W + 1] = v[0, W]
        k[1, W + 1] = k[1, W]; k[1, 1] = k[1, W]
        k[0, last + W] = k[0, last]; v[0, last + W + 1] = v[0, last + 1]
        k[1, last + 1] = k[1, last]; v[1, last + W] = v[1, last]; v[1, last + W + 1] = v[1, last]
    return q, k, v


@functools.lru_cache(maxsize=None)
def _case(C, H, W, Fr=2, tie=False):
    """inputs, upstream gradient and the float64 reference (o, dq, dk, dv) of one case: computed once, shared, never modified"""
    seed = 1000 + 7 * C + 131 * H + W
    q, k, v = _nl_inputs(C, H, W, Fr, seed, tie)
    go = O.seeded_randn((Fr, H * W, C // 2), seed + 3)
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    od = _attn_ref(qd, kd, vd, H, W)
    od.backward(go.double())
    return (q, k, v, go), (od.detach(), qd.grad, kd.grad, vd.grad)


def _run(npvp, q, k, v, go, H, W, op="nonlocal_attn_grid"):
    qg, kg, vg = (t.to(DEV).requires_grad_() for t in (q, k, v))
    og = getattr(npvp.ops, op)(qg, kg, vg, H, W)
    og.backward(go.to(DEV))
    torch.cuda.synchronize()
    return og.detach(), qg.grad, kg.grad, vg.grad


def _check(tag, got, ref):
    errs = [rel(a, b) for a, b in zip(got, ref)]
    for name, e in zip(("o", "dq", "dk", "dv"), errs):
        GC.log_err("nl_grid", f"{tag}:{name}", e)
    print(tag, " ".join(f"{n} {e:.2e}" for n, e in zip(("o", "dq", "dk", "dv"), errs)))
    for name, e in zip(("o", "dq", "dk", "dv"), errs):
        assert e < KERNEL_TOL, (tag, name, e)


def _uncovered(H, W):
    """mask [H*W] of the rows no 2x2 window covers (odd last line / column)"""
    m = torch.zeros(H, W, dtype=torch.bool)
    m[2 * (H // 2):] = True
    m[:, 2 * (W // 2):] = True
    return m.reshape(-1)


GRID_SHAPES = [
    (64, 2, 2),        # one key
    (64, 6, 6),        # HW 36 < QT, Lk 9
    (64, 7, 9),        # odd both, Lk 12
    (64, 34, 18),      # HW 612 = 4*128 + 100, Lk 153 = 2*64 + 25
    (64, 32, 32),      # tiles divide, not a config shape
    (128, 5, 6),
    (128, 12, 20),     # HW 240, Lk 60
    (128, 18, 14),     # Lk 63
    (128, 22, 24),     # HW 528 = 8*64 + 16, Lk 132
    (256, 9, 7),
    (256, 6, 10),      # Lk 15
    (256, 16, 18),     # HW 288 = 9*32: a key tail only, Lk 72
    (512, 3, 5),       # Lk 2, HW 15 < QT
    (512, 6, 10),      # HW 60 = 3*16 + 12, Lk 15
    (512, 8, 10),      # HW 80 exact, Lk 20 = 16 + 4
]


@pytest.mark.parametrize("C,H,W", GRID_SHAPES)
def test_grid_vs_float64(npvp, C, H, W):
    inp, ref = _case(C, H, W)
    got = _run(npvp, *inp, H, W)
    _check(f"{H}x{W}@{C}", got, ref)
    un = _uncovered(H, W)
    if bool(un.any()):
        assert float(got[2][:, un].abs().max()) == 0.0 and float(got[3][:, un].abs().max()) == 0.0


def test_grid_past_the_old_ceiling_vs_float64(npvp):
    """96x96 at C=64, one frame: 9 216 queries over 2 304 keys (the config grid at this width ends at 64x64)"""
    inp, ref = _case(64, 96, 96, 1)
    _check("96x96@64", _run(npvp, *inp, 96, 96), ref)


@pytest.mark.parametrize("C,H,W", [(512, 6, 10), (64, 7, 9)])
def test_grid_ties_route_as_torch(npvp, C, H, W):
    """tied windows (the first, a middle one and the last pooled line's): each window's gradient goes where torch's max_pool2d sends
    it, the tied later elements get exactly 0"""
    inp, ref = _case(C, H, W, 2, True)
    got = _run(npvp, *inp, H, W)
    _check(f"{H}x{W}@{C}:tie", got, ref)
    dk, dv = got[2].cpu(), got[3].cpu()
    assert torch.equal(dk == 0, ref[2] == 0) and torch.equal(dv == 0, ref[3] == 0)
    last = (2 * (H // 2) - 2) * W + 2 * (W // 2) - 2
    assert float(dk[0, 1].abs().max()) == 0.0 and float(dv[0, 1].abs().max()) == 0.0
    assert float(dk[0, last + W].abs().max()) == 0.0 and float(dk[0, last].abs().max()) > 0.0
    assert float(dv[1, last + W].abs().max()) == 0.0 and float(dv[1, last + W + 1].abs().max()) == 0.0
    assert float(dv[1, last].abs().max()) > 0.0


@pytest.mark.parametrize("C,H,W", [(64, 7, 9), (512, 3, 5), (256, 9, 7), (128, 5, 6)])
def test_odd_grid_writes_every_gradient_element(npvp, C, H, W):
    """the packed layout with padding columns (ld > 2A + V), the gradient buffer NaN-filled before the call: every q | k | v element
    is written (no NaN left), rows of the never-pooled line / column are exactly 0 in dk / dv, the padding columns come back 0"""
    A, V, Fr = C // 8, C // 2, 2
    (q, k, v, go), ref = _case(C, H, W)
    ld = 2 * A + V + 24
    qkv = torch.zeros(Fr * H * W, ld)
    qkv[:, :2 * A + V] = torch.cat([q.reshape(-1, A), k.reshape(-1, A), v.reshape(-1, V)], 1)
    qkv = qkv.to(DEV)
    un = _uncovered(H, W).repeat(Fr)
    # 1. the C entry points on a caller's NaN-filled buffer
    from npvp_amd._lib import check, lib
    o = torch.empty(Fr * H * W, V, device=DEV)
    lse = torch.empty(Fr * H * W, device=DEV)
    D = torch.empty(2 * Fr * H * W, device=DEV)
    dqkv = torch.full_like(qkv, float("nan"))
    g = go.reshape(-1, V).to(DEV).contiguous()
    p, d, st = qkv.data_ptr(), dqkv.data_ptr(), torch.cuda.current_stream().cuda_stream
    check(lib().npvp_nonlocal_attn_grid_fwd(p, ld, p + 4 * A, ld, p + 8 * A, ld, o.data_ptr(), V, lse.data_ptr(), Fr, H, W, A, V, st), "fwd")
    check(lib().npvp_nonlocal_attn_grid_bwd(p, ld, p + 4 * A, ld, p + 8 * A, ld, g.data_ptr(), V, lse.data_ptr(), D.data_ptr(),
                                            d, ld, d + 4 * A, ld, d + 8 * A, ld, Fr, H, W, A, V, st), "bwd")
    torch.cuda.synchronize()
    dh = dqkv.cpu()
    assert bool(torch.isfinite(dh[:, :2 * A + V]).all()) and bool(torch.isnan(dh[:, 2 * A + V:]).all())     # (padding: the op's job)
    assert bool(un.any()) and float(dh[un, A:2 * A + V].abs().max()) == 0.0
    assert rel(dh[:, :A], ref[1].reshape(-1, A)) < KERNEL_TOL
    assert rel(dh[:, A:2 * A], ref[2].reshape(-1, A)) < KERNEL_TOL and rel(dh[:, 2 * A:2 * A + V], ref[3].reshape(-1, V)) < KERNEL_TOL
    # 2. the op: the same bits, padding columns 0 (its gradient buffer very likely reuses the NaN block freed here)
    del dqkv
    leaf = qkv.clone().requires_grad_()
    og = npvp.ops.nonlocal_attn_grid_packed(leaf, Fr, H, W, A, V)
    assert torch.equal(og, o)
    og.backward(g)
    gh = leaf.grad.cpu()
    assert torch.equal(gh[:, :2 * A + V], dh[:, :2 * A + V])
    assert float(gh[:, 2 * A + V:].abs().max()) == 0.0 and float(gh[un, A:2 * A + V].abs().max()) == 0.0


@pytest.mark.parametrize("C,S", [(512, 8), (64, 64)])
def test_config_shapes_run_the_old_kernels(npvp, C, S):
    """a shape the existing entry points accept is handed to them: outputs and the three gradients are the same bits"""
    A, V = C // 8, C // 2
    q = O.seeded_randn((1, S * S, A), 300 + C) * (1.5 / A ** 0.5)
    k, v, go = O.seeded_randn((1, S * S, A), 301 + C), O.seeded_randn((1, S * S, V), 302 + C), O.seeded_randn((1, S * S, V), 303 + C)
    a = _run(npvp, q, k, v, go, S, S, "nonlocal_attn_grid")
    b = _run(npvp, q, k, v, go, S, S, "nonlocal_attn")
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i


@pytest.mark.parametrize("C,H,W", [(64, 34, 18), (512, 3, 5)])
def test_grid_kernels_are_bit_reproducible(npvp, C, H, W):
    inp, _ = _case(C, H, W)
    a, b = _run(npvp, *inp, H, W), _run(npvp, *inp, H, W)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i


# ------------------------------------------------------------------------------------------------------ the training step
def _pair(npvp, seed):
    enc, dec = npvp.build_autoencoder(RC.AE, RC.CI)
    O.key_hashed_fill(npvp.AEPair(enc, dec), seed)
    return enc, dec


def _frames(seed):
    x = torch.tanh(O.seeded_randn((RC.B, RC.T, RC.CI, RC.H, RC.W), seed))
    return x[:, : RC.T // 2].contiguous().to(DEV), x[:, RC.T // 2:].contiguous().to(DEV)


@pytest.fixture(scope="module")
def trained(npvp):
    """3 steps of the HIP path and of the stock path at 48x80 from the same weights and frames (as
    test_hip_ae_train.py::test_ae_train_step_matches_stock): what the step, validation and checkpoint tests below look at"""
    enc, dec = _pair(npvp, 7)
    s_enc, s_dec = copy.deepcopy(enc).to(DEV), copy.deepcopy(dec).to(DEV)
    enc, dec = enc.to(DEV).to(memory_format=torch.channels_last), dec.to(DEV)
    npvp.prepare_trainable_autoencoder(enc, dec)
    opt = npvp.ae_optimizer(enc, dec, lr=1e-4)
    s_opt = torch.optim.Adam(list(s_enc.parameters()) + list(s_dec.parameters()), lr=1e-4, betas=(0.5, 0.999))
    s_pair = npvp.AEPair(s_enc, s_dec)
    losses, grads = [], None
    for step in range(3):
        past, fut = _frames(60 + step)
        lh = npvp.ae_train_step(enc, dec, opt, past, fut)
        ls = _stock_step(s_enc, s_dec, s_opt, past, fut)
        losses.append((float(lh), float(ls)))
        if step == 0:
            grads = [(n, p.grad.detach().clone(), q.grad.detach().clone())
                     for (n, p), (_, q) in zip(opt.ae_pair.named_parameters(), s_pair.named_parameters())]
    return dict(enc=enc, dec=dec, opt=opt, s_enc=s_enc, s_dec=s_dec, s_pair=s_pair, losses=losses, grads=grads)


def test_ae_train_step_rect_matches_stock(npvp, trained):
    """losses, gradients of step 1, parameters and BatchNorm running statistics after step 3; that test's bounds"""
    for step, (lh, ls) in enumerate(trained["losses"]):
        assert abs(lh - ls) <= LOSS_TOL * abs(ls), (step, lh, ls)
    hg, sg = [], []
    for n, g, s in trained["grads"]:
        hg.append(g.reshape(-1)); sg.append(s.reshape(-1))
        if n.endswith(ZERO_GRAD):
            assert float(g.abs().max()) < 1e-6 and float(s.abs().max()) < 1e-6
            continue
        nh, ns = float(g.double().norm()), float(s.double().norm())
        GC.log_err("nl_grid", f"step-vs-stock:norm:{n}", abs(nh - ns) / ns)
        assert ns > 0.0, n
        assert abs(nh - ns) <= NORM_TOL * ns, (n, nh, ns)
    e = rel(torch.cat(hg), torch.cat(sg))
    GC.log_err("nl_grid", "step-vs-stock:grad", e)
    assert e < GRAD_TOL
    hs, ss = trained["opt"].ae_pair.state_dict(), trained["s_pair"].state_dict()
    assert list(hs) == list(ss)
    for kk in hs:
        if kk.endswith(ZERO_GRAD):
            continue
        if kk.endswith("num_batches_tracked"):
            assert int(hs[kk]) == int(ss[kk]) == 3
        else:
            assert rel(hs[kk], ss[kk]) < GRAD_TOL, (kk, rel(hs[kk], ss[kk]))


def test_ae_val_step_rect_matches_stock(npvp, trained):
    enc, dec, s_enc, s_dec = (trained[k] for k in ("enc", "dec", "s_enc", "s_dec"))
    past, fut = _frames(70)
    lv, rec = npvp.ae_val_step(enc, dec, past, fut)
    s_enc.eval(); s_dec.eval()
    try:
        with torch.no_grad():
            x = torch.cat([past, fut], 1)
            lvs = (s_dec(s_enc(x)) - x).abs().mean()
    finally:
        s_enc.train(); s_dec.train()
    assert abs(float(lv) - float(lvs)) <= LOSS_TOL * abs(float(lvs)) and enc.training and dec.training
    assert rec.shape[-2:] == (RC.H, RC.W)


def test_checkpoint_after_rect_training_loads_into_frozen_pair(npvp, trained, tmp_path):
    enc, dec, opt = (trained[k] for k in ("enc", "dec", "opt"))
    path = str(tmp_path / "ae.ckpt")
    npvp.save_ae_checkpoint(path, enc, dec, opt, epoch=0, global_step=3)
    fe, fd = npvp.build_frozen_autoencoder(RC.AE, RC.CI)
    assert npvp.load_lightning_checkpoint(path, None, fe, fd) == (0, 3)
    for a, b in ((fe, enc), (fd, dec)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        assert all(torch.equal(sa[k].cpu(), sb[k].cpu()) for k in sa)
    fe, fd = fe.to(DEV).eval(), fd.to(DEV).eval()            # the stock modules' own eval forward
    with torch.no_grad():
        y = fd(fe(_frames(71)[0]))
    assert y.shape[-2:] == (RC.H, RC.W) and bool(torch.isfinite(y).all())


def test_ae_train_step_rect_vs_reference_fixture(npvp):
    """two steps of ae_train_step at 48x80 against the reference LitAE's own two steps (tests/golden/ae_train_rect.npz): losses,
    per-parameter gradient norms and gradient heads of step 1, BatchNorm running statistics after step 1, parameter heads after
    steps 1 and 2; bounds as in test_hip_ae_train.py::test_ae_train_step_vs_reference_fixture"""
    gold = GC.load(RC.NAME)
    torch.manual_seed(0)
    enc, dec = npvp.build_autoencoder(RC.AE, RC.CI)
    RC.fill(npvp.AEPair(enc, dec))
    enc, dec = enc.to(DEV).to(memory_format=torch.channels_last), dec.to(DEV)
    npvp.prepare_trainable_autoencoder(enc, dec)
    opt = npvp.ae_optimizer(enc, dec, lr=RC.LR)
    assert list(RC.param_names(opt.ae_pair)) == list(gold["param_names"])
    assert list(RC.state_keys(opt.ae_pair)) == list(gold["state_keys"])
    res = RC.record(opt.ae_pair, lambda p, f: npvp.ae_train_step(enc, dec, opt, p, f), DEV)
    for k in ("loss_0", "loss_1"):
        GC.log_err("nl_grid", f"step-vs-fixture:{k}", abs(float(res[k]) - float(gold[k])) / abs(float(gold[k])))
        assert abs(float(res[k]) - float(gold[k])) <= LOSS_TOL * abs(float(gold[k])), (k, float(res[k]), float(gold[k]))
    keep = [i for i, n in enumerate(gold["param_names"]) if not str(n).endswith(ZERO_GRAD)]
    worst = (0.0, "")
    for i, n in enumerate(gold["param_names"]):
        nh, ng = float(res["grad_norm"][i]), float(gold["grad_norm"][i])
        if i in keep:
            worst = max(worst, (abs(nh - ng) / ng, str(n)))
    GC.log_err("nl_grid", f"step-vs-fixture:worst-norm:{worst[1]}", worst[0])
    print("worst per-tensor gradient norm deviation", worst)
    e = rel(res["grad_head"][keep], torch.as_tensor(gold["grad_head"][keep]))
    GC.log_err("nl_grid", "step-vs-fixture:grad_head", e)
    for i, n in enumerate(gold["param_names"]):
        nh, ng = float(res["grad_norm"][i]), float(gold["grad_norm"][i])
        if i in keep:
            assert abs(nh - ng) <= NORM_TOL * ng, (str(n), nh, ng)
        else:
            assert nh < 1e-6 and ng < 1e-6, (str(n), nh, ng)
    assert e < GRAD_TOL
    assert rel(res["running"], torch.as_tensor(gold["running"])) < 1e-3         # forward only: MIOpen vs CPU convolutions
    for k in ("param_head_0", "param_head_1"):
        for i in keep:
            assert rel(res[k][i], torch.as_tensor(gold[k][i])) < GRAD_TOL, (k, str(gold["param_names"][i]))
