"""GPU: the frozen decoder's opt-in 7 x 7 tail route (to_device_layout(..., tail7x7="hip"), csrc/conv7x7.hip): the forward kernel
npvp_tail7x7_f16 and the input-gradient kernel npvp_tail7x7_dgrad_f16 against the float64 reference of tests/frozen_tail7x7_cases.py
at the f16x3 bars of tests/test_hip_ops.py (written exactly once, nothing behind the output, bit-identical between launches), the op
ops.tail7x7_packed (forward, input gradient, slot hand-over, C calls counted, layouts, refusals) and two whole decoders under all
four (up3x3, tail7x7) combinations against the stock decoder.  NPVP_ERR_LOG=<file> appends the measured errors.

Gradients through ReLU (the whole decoders): a unit within rounding of zero may flip between two evaluations - see the comment at
tests/test_hip_golden.py::test_frozen_autoencoder and tests/test_hip_frozen_up3x3.py; the feature gradient is held to GRAD_BAR, the
project's bound for gradients through ReLU chains, and the frames to BAR.  The op's own gradient test takes the activation derivative
from the routed forward's own y."""
import pytest
import torch

import frozen_tail7x7_cases as TC
from oracle import ops as O
from test_hip_ops import ROW_TOL, close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL, TAIL = -12345.5, 4096
AE_NGF64 = dict(ngf=64, n_downsampling=3, num_res_blocks=2, learn_3d=False, out_layer='Sigmoid')     # configs/config_SMMNIST_VFP_NPVP-S.yaml
AE_NGF32 = dict(ngf=32, n_downsampling=4, num_res_blocks=1, learn_3d=False, out_layer='Tanh')        # the last upsampling is 64 -> 32: stock


@pytest.fixture(scope="module")
def npvp():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import npvp_amd
    return npvp_amd


@pytest.fixture(scope="module")
def refs():
    """case -> (inputs, float64 y, float64 dx with the reference's own activation derivative): computed once, never changed"""
    out = {}
    for c in TC.KERNEL_CASES:
        ins = TC.inputs(c)
        out[c] = (ins, TC.ref64(c, ins=ins))
    return out


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cl(t):
    """(F, C, H, W) -> the kernel's channels-last memory [F][H][W][C] as a contiguous tensor"""
    return t.permute(0, 2, 3, 1).contiguous()


def _planes(L, ins, Ci, Co):
    w = ins["w"].to(DEV)
    n = L.npvp_tail7x7_planes_bytes(Ci, Co) // 2
    assert n == 2 * 7 * Ci * 32
    fwd = torch.empty(n, dtype=torch.float16, device=DEV)
    bwd = torch.empty(n, dtype=torch.float16, device=DEV)
    w_slot = torch.zeros(512, device=DEV)
    assert L.npvp_tail7x7_planes(w.data_ptr(), Ci, Co, fwd.data_ptr(), w_slot.data_ptr(), _stream()) == 0, L.npvp_last_error()
    assert L.npvp_tail7x7_dgrad_planes(w.data_ptr(), Ci, Co, bwd.data_ptr(), w_slot.data_ptr(), _stream()) == 0, L.npvp_last_error()
    assert float(w_slot.max()) == float(ins["w"].abs().max())
    return fwd, bwd, w_slot


# ------------------------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("case", TC.KERNEL_CASES, ids=TC.case_id)
def test_tail7x7_forward_kernel_vs_float64(npvp, refs, case):
    Ci, Co, H, W, Fr, act = case
    L = npvp._lib.lib()
    ins, ref = refs[case]
    n = Fr * Co * H * W
    x = _cl(ins["x"]).to(DEV)
    fwd, _, w_slot = _planes(L, ins, Ci, Co)
    bias = ins["bias"].to(DEV)
    x_slot = torch.zeros(512, device=DEV)
    assert L.npvp_amax(x.data_ptr(), Fr * H * W, Ci, Ci, x_slot.data_ptr(), _stream()) == 0
    assert float(x_slot.max()) == float(ins["x"].abs().max())

    def launch():
        buf = torch.full((n + TAIL,), SENTINEL, device=DEV)
        rc = L.npvp_tail7x7_f16(x.data_ptr(), fwd.data_ptr(), bias.data_ptr(), buf.data_ptr(), Fr, H, W, Ci, Co, TC.ACT[act],
                                x_slot.data_ptr(), w_slot.data_ptr(), None, 0, _stream())
        assert rc == 0, L.npvp_last_error()
        torch.cuda.synchronize()
        assert bool((buf[n:] == SENTINEL).all()), "the kernel wrote behind y"
        return buf[:n].view(Fr, Co, H, W)

    y, y2 = launch(), launch()
    assert torch.equal(y, y2), "two launches differ"
    assert not bool((y == SENTINEL).any()), "an element of y was left unwritten"
    from golden_cases import max_row_rel_err
    TC.log_line(f"tail7x7[{TC.case_id(case)}] forward: rel-L2 {TC.rel(y, ref):.3e}, worst row {max_row_rel_err(y.cpu(), ref.float()):.3e} "
                f"(bars {TC.F16X3_TOL:.0e} / {ROW_TOL:.0e})")
    close(y, ref, tol=TC.F16X3_TOL, what=TC.case_id(case))


@pytest.mark.parametrize("case", TC.KERNEL_CASES, ids=TC.case_id)
def test_tail7x7_dgrad_kernel_vs_float64(npvp, refs, case):
    """dz = g * act'(reference y) in float64, rounded to fp32 -> the kernel -> dx [F][H][W][C_in] against autograd of pad + conv"""
    Ci, Co, H, W, Fr, act = case
    L = npvp._lib.lib()
    ins, yref = refs[case]
    dz = (ins["g"].double() * TC.act_grad64(yref, act)).float()
    x64 = ins["x"].double().requires_grad_()
    (dref,) = torch.autograd.grad(TC.pre64(case, ins, x64), x64, dz.double())
    dref = _cl(dref)
    _, bwd, w_slot = _planes(L, ins, Ci, Co)
    n, npad = dz.numel(), (dz.numel() + 3) // 4 * 4
    dzd = torch.zeros(npad, device=DEV)
    dzd[:n] = dz.to(DEV).view(-1)
    s = torch.zeros(512, device=DEV)
    assert L.npvp_amax(dzd.data_ptr(), 1, npad, npad, s.data_ptr(), _stream()) == 0
    M = Fr * H * W

    def launch():
        buf = torch.full((M * Ci + TAIL,), SENTINEL, device=DEV)
        rc = L.npvp_tail7x7_dgrad_f16(dzd.data_ptr(), bwd.data_ptr(), buf.data_ptr(), Fr, H, W, Ci, Co, s.data_ptr(), w_slot.data_ptr(),
                                      None, 0, _stream())
        assert rc == 0, L.npvp_last_error()
        torch.cuda.synchronize()
        assert bool((buf[M * Ci:] == SENTINEL).all()), "the kernel wrote behind dx"
        return buf[:M * Ci].view(Fr, H, W, Ci)

    dx, dx2 = launch(), launch()
    assert torch.equal(dx, dx2), "two launches differ"
    assert not bool((dx == SENTINEL).any()), "an element of dx was left unwritten"
    from golden_cases import max_row_rel_err
    TC.log_line(f"tail7x7[{TC.case_id(case)}] input gradient: rel-L2 {TC.rel(dx, dref):.3e}, worst row "
                f"{max_row_rel_err(dx.cpu(), dref.float()):.3e} (bars {TC.F16X3_TOL:.0e} / {ROW_TOL:.0e})")
    close(dx, dref, tol=TC.F16X3_TOL, what=TC.case_id(case))


# ----------------------------------------------------------------------------------------------------------------------- the op
@pytest.mark.parametrize("case", [TC.KERNEL_CASES[0], TC.KERNEL_CASES[2], TC.KERNEL_CASES[3]], ids=TC.case_id)
def test_op_forward_and_input_gradient_vs_float64(npvp, refs, case):
    """ops.tail7x7_packed on an untagged input: one npvp_amax pass plus one launch; backward: act_bwd (absent for act = none), amax,
    dgrad.  y against float64, dx against float64 with the activation derivative taken from the routed forward's own y."""
    L, ops = npvp._lib.lib(), npvp.ops
    Ci, Co, H, W, Fr, act = case
    code = TC.ACT[act]
    ins, ref = refs[case]
    x = ins["x"].to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
    bias = ins["bias"].to(DEV)
    planes = ops.tail7x7_planes(ins["w"].to(DEV))
    names = ("npvp_amax", "npvp_tail7x7_f16", "npvp_tail7x7_dgrad_f16", "npvp_act_bwd")
    real = {n: getattr(L, n) for n in names}
    calls = []
    count = lambda name: lambda *a: calls.append((name, len(a))) or real[name](*a)
    try:
        for n in names:
            setattr(L, n, count(n))
        y = ops.tail7x7_packed(x, planes, bias, code)
        assert calls == [("npvp_amax", 6), ("npvp_tail7x7_f16", 15)], calls
        del calls[:]
        (dx,) = torch.autograd.grad(y, x, ins["g"].to(DEV))
        assert calls == ([("npvp_act_bwd", 6)] if code else []) + [("npvp_amax", 6), ("npvp_tail7x7_dgrad_f16", 13)], calls
    finally:
        for n, f in real.items():
            setattr(L, n, f)
    torch.cuda.synchronize()
    assert y.shape == (Fr, Co, H, W) and y.is_contiguous(), "the frames come out in contiguous NCHW"
    assert dx.shape == (Fr, Ci, H, W) and dx.permute(0, 2, 3, 1).is_contiguous(), "dx is channels-last"
    dref = TC.dgrad64(case, ins, y=y)
    ey, ed = TC.rel(y, ref), TC.rel(dx, dref)
    TC.log_line(f"tail7x7_packed[{TC.case_id(case)}]: y {ey:.3e}, dx {ed:.3e} (bar {TC.F16X3_TOL:.0e})")
    assert ey < TC.F16X3_TOL and ed < TC.F16X3_TOL, (ey, ed)


def test_op_behind_a_routed_upsampling_needs_no_amax_pass(npvp):
    """convt3x3s2_packed (128 -> 64) hands its amax slot to the tail: one launch, no npvp_amax pass; against float64 at BAR (two layers)"""
    import torch.nn.functional as F
    L, ops = npvp._lib.lib(), npvp.ops
    x = O.seeded_randn((2, 128, 4, 4), 3170)
    wt = O.seeded_randn((128, 64, 3, 3), 3171) * (9 * 128 / 4) ** -0.5
    bt = O.seeded_randn((64,), 3172)
    w = O.seeded_randn((3, 64, 7, 7), 3173) * (49 * 64) ** -0.5
    b = O.seeded_randn((3,), 3174)
    up = ops.convt3x3s2_planes(wt.to(DEV))
    planes = ops.tail7x7_planes(w.to(DEV))
    names = ("npvp_amax", "npvp_tail7x7_f16")
    real = {n: getattr(L, n) for n in names}
    calls = []
    count = lambda name: lambda *a: calls.append(name) or real[name](*a)
    with torch.no_grad():
        mid = ops.convt3x3s2_packed(x.to(DEV).contiguous(memory_format=torch.channels_last), up, bt.to(DEV), 1)
        try:
            for n in names:
                setattr(L, n, count(n))
            y = ops.tail7x7_packed(mid, planes, b.to(DEV), 2)
        finally:
            for n, f in real.items():
                setattr(L, n, f)
    assert calls == ["npvp_tail7x7_f16"], calls
    mid64 = (F.conv_transpose2d(x.double(), wt.double(), None, 2, 1, 1) + bt.double().view(1, -1, 1, 1)).clamp_min(0)
    ref = torch.tanh(F.conv2d(F.pad(mid64, (3, 3, 3, 3), "reflect"), w.double()) + b.double().view(1, -1, 1, 1))
    e = TC.rel(y, ref)
    TC.log_line(f"tail7x7_packed behind convt3x3s2_packed: y {e:.3e} (bar {TC.F16X3_TOL:.0e})")
    assert y.shape == (2, 3, 8, 8) and y.is_contiguous() and e < TC.F16X3_TOL, e


def test_op_checks_its_arguments(npvp):
    ops = npvp.ops
    case = TC.KERNEL_CASES[2]
    ins = TC.inputs(case)
    x = ins["x"].to(DEV).contiguous(memory_format=torch.channels_last)
    bias = ins["bias"].to(DEV)
    planes = ops.tail7x7_planes(ins["w"].to(DEV))
    with pytest.raises(RuntimeError, match="channels-last"):
        ops.tail7x7_packed(ins["x"].to(DEV), planes, bias, 2)
    with pytest.raises(RuntimeError, match="planes do not belong"):
        ops.tail7x7_packed(x, planes._replace(fwd=planes.fwd[:-8]), bias, 2)
    with pytest.raises(RuntimeError, match="planes do not belong"):
        ops.tail7x7_packed(x, planes._replace(bwd=planes.bwd[:-8]), bias, 2)
    with pytest.raises(RuntimeError, match="at least 4"):
        ops.tail7x7_packed(x[:, :, :3].contiguous(memory_format=torch.channels_last), planes, bias, 2)
    with pytest.raises(RuntimeError, match="at least 4"):
        ops.tail7x7_packed(x[:, :, :, :3].contiguous(memory_format=torch.channels_last), planes, bias, 2)
    with pytest.raises(RuntimeError, match="act is 0"):
        ops.tail7x7_packed(x, planes, bias, 1)
    with pytest.raises(RuntimeError, match="1 <= C_out <= 4"):
        ops.tail7x7_packed(x, planes, torch.zeros(5, device=DEV), 2)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ops.tail7x7_planes(torch.zeros(3, 48, 7, 7, device=DEV))
    with pytest.raises(RuntimeError, match="1 <= C_out <= 4"):
        ops.tail7x7_planes(torch.zeros(5, 64, 7, 7, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tail7x7_packed(x.cpu(), planes, bias, 2)


# ------------------------------------------------------------------------------------------------------------- whole decoders
ROUTES = (("stock", "stock"), ("hip", "stock"), ("stock", "hip"), ("hip", "hip"))


@pytest.fixture(scope="module")
def decoders(npvp):
    """(AE name) -> {(up3x3, tail7x7): fused decoder} on the same weights, and the 2 frames of 2 x 2 features they decode"""
    out = {}
    for name, AE, ch in (("ngf64x3", AE_NGF64, 1), ("ngf32x4", AE_NGF32, 3)):
        decs = {}
        for up, tail in ROUTES:
            enc, dec = npvp.build_frozen_autoencoder(AE, ch)
            O.key_hashed_fill(dec, 3142)
            decs[(up, tail)] = npvp.to_device_layout(enc, dec, DEV, up3x3=up, tail7x7=tail)[1]
        C = AE["ngf"] << AE["n_downsampling"]
        feats = O.seeded_randn((1, 2, C, 2, 2), 3143).clamp_min(0).to(DEV)          # (the encoder's features are post-ReLU)
        out[name] = (decs, feats, AE, ch)
    return out


@pytest.mark.parametrize("name", ["ngf64x3", "ngf32x4"])
def test_whole_decoder_every_route_combination_vs_stock(npvp, decoders, name):
    decs, feats, AE, ch = decoders[name]
    for (up, tail), dec in decs.items():
        assert [m.tail7x7 for m in dec.model] == [False] * AE["n_downsampling"] + [tail == "hip"] and dec.tail7x7 == (tail == "hip")
        assert sum(m.up3x3 for m in dec.model) == (3 if up == "hip" else 0)
    side = 2 << AE["n_downsampling"]
    gy = O.seeded_randn((1, 2, ch, side, side), 3144).to(DEV)
    res = {}
    for route, dec in decs.items():
        f = feats.clone().requires_grad_()
        y = dec(f)
        (gf,) = torch.autograd.grad(y, f, gy)
        assert y.is_contiguous(), route
        res[route] = (y.detach(), gf)
    ys, gs = res[("stock", "stock")]
    assert ys.shape == (1, 2, ch, side, side) and float(ys.abs().max()) > 0 and float(gs.abs().max()) > 0
    bad = []
    for route in ROUTES[1:]:
        yh, gh = res[route]
        assert yh.shape == ys.shape and gh.shape == gs.shape == feats.shape
        e, eg = TC.rel(yh, ys), TC.rel(gh, gs)
        TC.log_line(f"decoder ngf {AE['ngf']} / {AE['n_downsampling']} upsamplings, 2 frames of 2x2 features, up3x3={route[0]} "
                    f"tail7x7={route[1]} vs stock: forward rel-L2 {e:.3e} (bar {TC.BAR:.0e}), feature gradient {eg:.3e} "
                    f"(bar {TC.GRAD_BAR:.0e})")
        if not (e < TC.BAR and eg < TC.GRAD_BAR):
            bad.append((route, e, eg))
    assert not bad, bad


def test_routed_decoder_layouts(npvp, decoders, monkeypatch):
    """ngf = 64, both routes: no copy back to NCHW remains (the tail takes the channels-last tensor of the last routed upsampling);
    up3x3 = stock: the tail's input is the one channels-last copy the decoder makes"""
    decs, feats, AE, ch = decoders["ngf64x3"]
    seen = []
    packed = npvp.ops.tail7x7_packed
    monkeypatch.setattr(npvp.ops, "tail7x7_packed", lambda x, *a: (seen.append((x._base is not None, x.permute(0, 2, 3, 1).is_contiguous())),
                                                                    packed(x, *a))[1])
    with torch.no_grad():
        decs[("hip", "hip")](feats)
        decs[("stock", "hip")](feats)
    assert seen == [(True, True), (False, True)], seen
