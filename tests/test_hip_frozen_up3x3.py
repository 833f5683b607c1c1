"""GPU: the frozen decoder's opt-in transposed 3 x 3 convolution route (to_device_layout(..., up3x3="hip")): the kernel
npvp_convt3x3s2_f16 against the float64 reference of tests/frozen_up3x3_cases.py at the f16x3 bars of tests/test_hip_ops.py (written
exactly once, nothing behind y, bit-identical between launches, y_amax filled), the op's input gradient, slot hand-over, launch counts
and argument checks, one routed ConvTranspose2d + BatchNorm + ReLU group against its float64 restatement, two whole decoders against
the stock route (forward and input gradient), and what the routed forward saves or leaves alone.  NPVP_ERR_LOG=<file> appends the
measured errors.

Gradients through ReLU: the float64 reference takes its mask from the routed forward's OWN output y (a unit within rounding of zero
may flip between two evaluations - see the comment at tests/test_hip_golden.py::test_frozen_autoencoder); the forward tests bound y."""
import pytest
import torch
import torch.nn.functional as F

import frozen_up3x3_cases as UC
from oracle import ops as O
from test_hip_ops import ROW_TOL, close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL, TAIL = -12345.5, 4096
AE_SMMNIST = dict(ngf=64, n_downsampling=3, num_res_blocks=2, learn_3d=False, out_layer='Sigmoid')   # configs/config_SMMNIST_VFP_NPVP-S.yaml
AE_NGF32 = dict(ngf=32, n_downsampling=4, num_res_blocks=1, learn_3d=False, out_layer='Tanh')        # the last upsampling is 64 -> 32: stock


@pytest.fixture(scope="module")
def npvp():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import npvp_amd
    return npvp_amd


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rows(t):
    """(F, C, H, W) -> the kernel's [F H W][C] matrix (a contiguous copy)"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def _act_grad64(y, act):
    """d act / d pre-activation in float64, through the OUTPUT y (the own-mask rule for ReLU)"""
    y = y.detach().double().cpu()
    return {"none": torch.ones_like(y), "relu": (y > 0).double(), "tanh": 1 - y * y, "sigmoid": y * (1 - y)}[act]


# ------------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("case", UC.KERNEL_CASES, ids=UC.case_id)
def test_convt3x3s2_kernel_vs_float64(npvp, case):
    Ci, Co, H, W, Fr, act = case
    L = npvp._lib.lib()
    ins = UC.inputs(case)
    ref = _rows(UC.ref64(case, ins=ins))
    M = Fr * 4 * H * W
    assert ref.shape == (M, Co)
    x = _rows(ins["x"]).to(DEV)
    w = ins["w"].to(DEV)
    planes = torch.empty(L.npvp_convt3x3s2_planes_bytes(Ci, Co) // 2, dtype=torch.float16, device=DEV)
    assert planes.numel() == 2 * 9 * Ci * Co
    w_slot = torch.zeros(512, device=DEV)
    assert L.npvp_convt3x3s2_planes(w.data_ptr(), Ci, Co, planes.data_ptr(), w_slot.data_ptr(), _stream()) == 0, L.npvp_last_error()
    bias = ins["bias"].to(DEV)
    x_slot = torch.zeros(512, device=DEV)
    assert L.npvp_amax(x.data_ptr(), Fr * H * W, Ci, Ci, x_slot.data_ptr(), _stream()) == 0
    assert float(w_slot.max()) == float(ins["w"].abs().max()) and float(x_slot.max()) == float(ins["x"].abs().max())

    def launch(want_amax):
        buf = torch.full((M * Co + TAIL,), SENTINEL, device=DEV)
        y_slot = torch.zeros(512, device=DEV) if want_amax else None
        rc = L.npvp_convt3x3s2_f16(x.data_ptr(), planes.data_ptr(), bias.data_ptr(), buf.data_ptr(), Fr, H, W, Ci, Co, UC.ACT[act],
                                   x_slot.data_ptr(), w_slot.data_ptr(), y_slot.data_ptr() if want_amax else None, None, 0, _stream())
        assert rc == 0, L.npvp_last_error()
        torch.cuda.synchronize()
        assert bool((buf[M * Co:] == SENTINEL).all()), "the kernel wrote behind y"
        return buf[:M * Co].view(M, Co), y_slot

    y, y_slot = launch(True)
    y2, _ = launch(False)
    assert torch.equal(y, y2), "two launches differ"
    assert not bool((y == SENTINEL).any()), "an element of y was left unwritten"
    m, sv = float(y.abs().max()), float(y_slot.max())
    assert m <= sv < 2 * m, (m, sv)
    e = UC.rel(y, ref)
    from golden_cases import max_row_rel_err
    UC.log_line(f"convt3x3s2[{UC.case_id(case)}] rows {M}: rel-L2 {e:.3e}, worst row {max_row_rel_err(y.cpu(), ref.float()):.3e} "
                f"(bars {UC.F16X3_TOL:.0e} / {ROW_TOL:.0e})")
    close(y, ref, tol=UC.F16X3_TOL, what=UC.case_id(case))


# ----------------------------------------------------------------------------------------------------------------------- the op
@pytest.mark.parametrize("case,act", UC.GRAD_CASES, ids=[f"{UC.case_id(c)}_as_{a}" for c, a in UC.GRAD_CASES])
def test_op_forward_and_input_gradient_vs_float64(npvp, case, act):
    """ops.convt3x3s2_packed -> a second routed layer, with the C calls counted: forward = one npvp_amax pass for the untagged input +
    one launch, the layer behind it no pass; backward of the first = act_bwd (when there is an activation), amax, one
    npvp_conv3x3s2_f16.  dx against float64 with the mask / derivative taken from the routed forward's own y."""
    L, ops = npvp._lib.lib(), npvp.ops
    Ci, Co, H, W, Fr, _ = case
    code = UC.ACT[act]
    ins = UC.inputs(case)
    x = ins["x"].to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
    bias = ins["bias"].to(DEV)
    planes = ops.convt3x3s2_planes(ins["w"].to(DEV))
    w1 = O.seeded_randn((Co, 64, 3, 3), 2990) * (9 * Co / 4) ** -0.5
    b1 = O.seeded_randn((64,), 2991)
    planes1 = ops.convt3x3s2_planes(w1.to(DEV))
    g = O.seeded_randn((Fr, Co, 2 * H, 2 * W), 2992)
    names = ("npvp_amax", "npvp_convt3x3s2_f16", "npvp_conv3x3s2_f16", "npvp_act_bwd")
    real = {n: getattr(L, n) for n in names}
    calls = []
    count = lambda name: lambda *a: calls.append((name, len(a))) or real[name](*a)
    try:
        for n in names:
            setattr(L, n, count(n))
        y = ops.convt3x3s2_packed(x, planes, bias, code)
        assert calls == [("npvp_amax", 6), ("npvp_convt3x3s2_f16", 16)], calls
        del calls[:]
        with torch.no_grad():
            z = ops.convt3x3s2_packed(y, planes1, b1.to(DEV), 1)
        assert calls == [("npvp_convt3x3s2_f16", 16)], calls
        del calls[:]
        (dx,) = torch.autograd.grad(y, x, g.to(DEV))
        assert calls == ([("npvp_act_bwd", 6)] if code else []) + [("npvp_amax", 6), ("npvp_conv3x3s2_f16", 17)], calls
    finally:
        for n, f in real.items():
            setattr(L, n, f)
    torch.cuda.synchronize()
    assert y.shape == (Fr, Co, 2 * H, 2 * W) and y.is_contiguous(memory_format=torch.channels_last)
    assert dx.shape == (Fr, Ci, H, W) and dx.is_contiguous(memory_format=torch.channels_last)
    pre = UC.convt64(ins["x"], ins["w"]) + ins["bias"].double().view(1, Co, 1, 1)
    ref = UC.act64(pre, act)
    ey = UC.rel(y, ref)
    slot = ops.amax_of(y.permute(0, 2, 3, 1).reshape(-1, Co))
    assert slot is y._npvp_amax[0] and slot is y._base._npvp_amax[0] and slot.read() == float(y.detach().abs().max())
    zref = (UC.convt64(ref, w1) + b1.double().view(1, -1, 1, 1)).clamp_min(0)
    ez = UC.rel(z, zref)
    dref = F.conv2d(g.double() * _act_grad64(y, act), ins["w"].double(), None, 2, 1)
    ed = UC.rel(dx, dref)
    UC.log_line(f"convt3x3s2_packed[{UC.case_id(case)} as {act}]: y {ey:.3e}, second layer {ez:.3e}, dx {ed:.3e} (bar {UC.F16X3_TOL:.0e})")
    assert ey < UC.F16X3_TOL and ez < UC.F16X3_TOL and ed < UC.F16X3_TOL, (ey, ez, ed)


def test_op_checks_its_arguments(npvp):
    ops = npvp.ops
    case = UC.KERNEL_CASES[2]
    Ci, Co, H, W, Fr, act = case
    ins = UC.inputs(case)
    x = ins["x"].to(DEV).contiguous(memory_format=torch.channels_last)
    bias = ins["bias"].to(DEV)
    planes = ops.convt3x3s2_planes(ins["w"].to(DEV))
    with pytest.raises(RuntimeError, match="channels-last"):
        ops.convt3x3s2_packed(ins["x"].to(DEV), planes, bias)
    with pytest.raises(RuntimeError, match="planes do not belong"):
        ops.convt3x3s2_packed(x, planes._replace(fwd=planes.fwd[:-8]), bias)
    with pytest.raises(RuntimeError, match="planes do not belong"):
        ops.convt3x3s2_packed(x, planes._replace(bwd=planes.bwd[:-8]), bias)
    with pytest.raises(RuntimeError, match="planes do not belong"):
        ops.convt3x3s2_packed(x[:, :64], planes, bias)
    with pytest.raises(RuntimeError, match="multiples of 64"):
        ops.convt3x3s2_packed(x, planes, bias[:32])
    with pytest.raises(RuntimeError, match="multiples of 64"):
        ops.convt3x3s2_planes(torch.zeros(32, 64, 3, 3, device=DEV))
    with pytest.raises(RuntimeError, match="multiples of 64"):
        ops.convt3x3s2_planes(torch.zeros(64, 32, 3, 3, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.convt3x3s2_packed(x.cpu(), planes, bias)


# ------------------------------------------------------------------------------------------------------------------ the modules
def test_routed_upsampling_group_vs_float64(npvp):
    """ConvTranspose2d(256, 128, 3, stride 2, padding 1, output_padding 1) -> BatchNorm2d -> ReLU (eval mode) folded and routed, against
    the unfused modules in float64: forward, and the input gradient with the ReLU mask of the routed forward's own output"""
    import copy
    import torch.nn as nn
    from npvp_amd.models.ResNetAutoEncoder import _fold_sequential, _route_up3x3
    seq = nn.Sequential(nn.ConvTranspose2d(UC.MODULE_CIN, UC.MODULE_COUT, 3, stride=2, padding=1, output_padding=1, bias=False),
                        nn.BatchNorm2d(UC.MODULE_COUT), nn.ReLU(True)).eval()
    O.key_hashed_fill(seq, 2821)
    ref_mod = copy.deepcopy(seq).double()
    with torch.no_grad():
        folded = _fold_sequential(seq.to(DEV).to(memory_format=torch.channels_last))
    _route_up3x3(list(folded))
    assert folded[0].up3x3 and folded[0]._npvp_planes.is_cuda and folded[0]._npvp_bwd_planes.is_cuda and folded[0].act == 1
    x = O.seeded_randn((UC.MODULE_FRAMES, UC.MODULE_CIN, UC.MODULE_GRID, UC.MODULE_GRID), 2830)
    g = O.seeded_randn((UC.MODULE_FRAMES, UC.MODULE_COUT, 2 * UC.MODULE_GRID, 2 * UC.MODULE_GRID), 2831)
    L = npvp._lib.lib()
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
    n0 = L.npvp_launch_count()
    out = folded(xd)
    assert L.npvp_launch_count() - n0 == 2, "one npvp_amax pass over the untagged input and the convolution"
    (dx,) = torch.autograd.grad(out, xd, g.to(DEV))
    assert L.npvp_launch_count() - n0 == 5, "act_bwd, amax and the stride-2 convolution"
    # float64: the unfused modules up to the BatchNorm, then the ReLU with the routed forward's own mask
    x64 = x.double().requires_grad_()
    pre = ref_mod[1](ref_mod[0](x64))
    ref = pre.clamp_min(0)
    (dref,) = torch.autograd.grad(pre, x64, g.double() * _act_grad64(out, "relu"))
    e, ed = UC.rel(out, ref), UC.rel(dx, dref)
    UC.log_line(f"up3x3 hip group {UC.MODULE_CIN} -> {UC.MODULE_COUT} grid {UC.MODULE_GRID}: forward rel-L2 {e:.3e}, input gradient "
                f"{ed:.3e} (bar {UC.BAR:.0e})")
    assert out.shape == ref.shape and dx.shape == x.shape and float(ref.detach().abs().max()) > 0 and float(dref.abs().max()) > 0
    assert e < UC.BAR and ed < UC.BAR, (e, ed)


@pytest.fixture(scope="module")
def decoders(npvp):
    """(AE name) -> {route: fused decoder} on the same weights, and the 4 frames of 8 x 8 features they decode"""
    out = {}
    for name, AE, ch in (("smmnist", AE_SMMNIST, 1), ("ngf32x4", AE_NGF32, 3)):
        decs = {}
        for route in ("stock", "hip"):
            enc, dec = npvp.build_frozen_autoencoder(AE, ch)
            O.key_hashed_fill(dec, 2842)
            decs[route] = npvp.to_device_layout(enc, dec, DEV, up3x3=route)[1]
        C = AE["ngf"] << AE["n_downsampling"]
        feats = O.seeded_randn((2, 2, C, 8, 8), 2843).clamp_min(0).to(DEV)          # (the encoder's features are post-ReLU)
        out[name] = (decs, feats, AE, ch)
    return out


@pytest.mark.parametrize("name", ["smmnist", "ngf32x4"])
def test_whole_decoder_hip_vs_stock(npvp, decoders, name):
    """4 frames of 8 x 8 features through the decoder: forward at BAR, the input gradient at the project's bound for gradients through
    ReLU chains; three transposed convolutions are routed in both (all three, and three of four)"""
    decs, feats, AE, ch = decoders[name]
    assert sum(getattr(m, "up3x3", False) is True for m in decs["hip"].model) == 3
    assert not any(getattr(m, "up3x3", False) for m in decs["stock"].model) and decs["hip"].up3x3 and not decs["stock"].up3x3
    side = 8 << AE["n_downsampling"]
    gy = O.seeded_randn((2, 2, ch, side, side), 2844).to(DEV)
    res = {}
    for route, dec in decs.items():
        f = feats.clone().requires_grad_()
        y = dec(f)
        (gf,) = torch.autograd.grad(y, f, gy)
        res[route] = (y.detach(), gf)
    ys, gs = res["stock"]
    yh, gh = res["hip"]
    assert ys.shape == yh.shape == (2, 2, ch, side, side) and gh.shape == gs.shape == feats.shape
    assert float(ys.abs().max()) > 0 and float(gs.abs().max()) > 0
    e, eg = UC.rel(yh, ys), UC.rel(gh, gs)
    UC.log_line(f"decoder ngf {AE['ngf']} / {AE['n_downsampling']} upsamplings, 4 frames of 8x8 features: up3x3 hip vs stock forward rel-L2 "
                f"{e:.3e} (bar {UC.BAR:.0e}), input gradient {eg:.3e} (bar {UC.GRAD_BAR:.0e})")
    assert e < UC.BAR and eg < UC.GRAD_BAR, (e, eg)


def test_routed_decoder_saves_nothing_under_no_grad(npvp, decoders, monkeypatch):
    decs, feats, AE, ch = decoders["smmnist"]
    saved = []
    real = npvp.ops._ConvT3x3S2.forward

    class Spy:
        def __init__(self, ctx):
            object.__setattr__(self, "_ctx", ctx)

        def save_for_backward(self, *ts):
            saved.append(len(ts))
            self._ctx.save_for_backward(*ts)

        def __getattr__(self, k):
            return getattr(self._ctx, k)

        def __setattr__(self, k, v):
            setattr(self._ctx, k, v)
    monkeypatch.setattr(npvp.ops._ConvT3x3S2, "forward", staticmethod(lambda ctx, *a: real(Spy(ctx), *a)))
    with torch.no_grad():
        y = decs["hip"](feats)
    assert not saved and not y.requires_grad and y.grad_fn is None
    with torch.no_grad():
        y2 = decs["hip"](feats.clone().requires_grad_())
    assert not saved and not y2.requires_grad
    y3 = decs["hip"](feats.clone().requires_grad_())
    assert saved == [4, 4, 4] and y3.requires_grad
    del saved[:]
    decs["hip"](feats)                                   # grad mode on, nothing requires grad: nothing to save either
    assert not saved
    # the routed kernel gives the same bits whether or not its output is saved
    m, x = decs["hip"].model[0], feats.flatten(0, 1).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        a = m(x)
    assert torch.equal(a, m(x.clone().requires_grad_()).detach()) and saved == [4]


def test_routed_module_leaves_nchw_on_stock(npvp, decoders, monkeypatch):
    """an NCHW-contiguous input at a routed FoldedConvAct: the stock forward (F.conv_transpose2d + one npvp_bias_act pass), no copy to
    channels-last, the kernel not called; within BAR of the routed forward of the same frames"""
    decs, feats, AE, ch = decoders["smmnist"]
    L = npvp._lib.lib()
    m = decs["hip"].model[0]
    x = feats.flatten(0, 1)
    assert m.up3x3 and x.is_contiguous()
    taken = []
    packed = npvp.ops.convt3x3s2_packed
    monkeypatch.setattr(npvp.ops, "convt3x3s2_packed", lambda *a, **k: (taken.append(1), packed(*a, **k))[1])
    real = F.conv_transpose2d
    convs = []

    def convt(inp, *a):
        convs.append((tuple(inp.shape), inp.is_contiguous()))
        return real(inp, *a)
    monkeypatch.setattr(torch.nn.functional, "conv_transpose2d", convt)
    with torch.no_grad():
        n0 = L.npvp_launch_count()
        y = m(x)
        assert L.npvp_launch_count() - n0 == 1 and not taken and convs == [((4, 512, 8, 8), True)]
        yh = m(x.contiguous(memory_format=torch.channels_last))
        assert len(taken) == 1 and len(convs) == 1
    assert y.shape == yh.shape == (4, 256, 16, 16) and UC.rel(yh, y) < UC.BAR
