"""GPU: the frozen encoder's opt-in 7 x 7 stem route (to_device_layout(..., stem7x7="hip"), csrc/conv7x7.hip): the kernel
npvp_stem7x7_f16 against the float64 reference of tests/frozen_stem7x7_cases.py at the f16x3 bars of tests/test_hip_ops.py (written
exactly once, nothing behind the output, bit-identical between launches, the output's amax slot), the op ops.stem7x7_packed (C calls
counted, slot hand-over to the routed downsampling convolution, layouts, refusals) and two whole encoders against the stock pair.
NPVP_ERR_LOG=<file> appends the measured errors."""
import pytest
import torch

import frozen_stem7x7_cases as SC
from oracle import ops as O
from test_hip_ops import ROW_TOL, close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL, TAIL = -12345.5, 4096
AE_NGF64 = dict(ngf=64, n_downsampling=3, num_res_blocks=2, learn_3d=False, out_layer='Sigmoid')     # configs/config_SMMNIST_VFP_NPVP-S.yaml
AE_NGF32 = dict(ngf=32, n_downsampling=4, num_res_blocks=1, learn_3d=False, out_layer='Tanh')
OTHERS_STOCK = dict(attn2d="stock", conv3x3="stock", down3x3="stock")
OTHERS_HIP = dict(attn2d="hip", conv3x3="hip", down3x3="hip")


@pytest.fixture(scope="module")
def npvp():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import npvp_amd
    return npvp_amd


@pytest.fixture(scope="module")
def refs():
    """case -> (inputs, float64 y): computed once, never changed"""
    out = {}
    for c in SC.KERNEL_CASES:
        ins = SC.inputs(c)
        out[c] = (ins, SC.ref64(c, ins=ins))
    return out


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _padded4(t):
    """the planar memory of t on the device behind a zero tail up to a multiple of 4 floats (npvp_amax reads float4s)"""
    n = t.numel()
    buf = torch.zeros((n + 3) // 4 * 4, device=DEV)
    buf[:n] = t.to(DEV).reshape(-1)
    return buf


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("case", SC.KERNEL_CASES, ids=SC.case_id)
def test_stem7x7_kernel_vs_float64(npvp, refs, case):
    Ci, Co, H, W, Fr, act = case
    L = npvp._lib.lib()
    ins, ref = refs[case]
    ref_cl = ref.permute(0, 2, 3, 1).contiguous()
    n = Fr * H * W * Co
    x = _padded4(ins["x"])
    w = ins["w"].to(DEV)
    halves = L.npvp_stem7x7_planes_bytes(Ci, Co) // 2
    assert halves == 2 * (-(-49 * Ci // 32) * 32) * Co
    planes = torch.empty(halves, dtype=torch.float16, device=DEV)
    w_slot = torch.full((512,), 7.0, device=DEV)                      # (stale on purpose: the entry point zeroes and recomputes it)
    assert L.npvp_stem7x7_planes(w.data_ptr(), Ci, Co, planes.data_ptr(), w_slot.data_ptr(), _stream()) == 0, L.npvp_last_error()
    assert float(w_slot.max()) == float(ins["w"].abs().max())
    bias = ins["bias"].to(DEV)
    x_slot = torch.zeros(512, device=DEV)
    assert L.npvp_amax(x.data_ptr(), 1, x.numel(), x.numel(), x_slot.data_ptr(), _stream()) == 0
    assert float(x_slot.max()) == float(ins["x"].abs().max())

    def launch(with_slot=True):
        buf = torch.full((n + TAIL,), SENTINEL, device=DEV)
        y_slot = torch.zeros(512, device=DEV) if with_slot else None
        rc = L.npvp_stem7x7_f16(x.data_ptr(), planes.data_ptr(), bias.data_ptr(), buf.data_ptr(), Fr, H, W, Ci, Co, SC.ACT[act],
                                x_slot.data_ptr(), w_slot.data_ptr(), y_slot.data_ptr() if with_slot else None, None, 0, _stream())
        assert rc == 0, L.npvp_last_error()
        torch.cuda.synchronize()
        assert bool((buf[n:] == SENTINEL).all()), "the kernel wrote behind y"
        return buf[:n].view(Fr, H, W, Co), y_slot

    (y, y_slot), (y2, _), (y3, _) = launch(), launch(), launch(False)
    assert torch.equal(y, y2), "two launches differ"
    assert torch.equal(y, y3), "y differs without an amax slot"
    assert not bool((y == SENTINEL).any()), "an element of y was left unwritten"
    assert float(y_slot.max()) == float(y.abs().max()), "the slot holds the bound of the stored values"
    from golden_cases import max_row_rel_err
    SC.log_line(f"stem7x7[{SC.case_id(case)}]: rel-L2 {SC.rel(y, ref_cl):.3e}, worst row {max_row_rel_err(y.cpu(), ref_cl.float()):.3e} "
                f"(bars {SC.F16X3_TOL:.0e} / {ROW_TOL:.0e})")
    close(y, ref_cl, tol=SC.F16X3_TOL, what=SC.case_id(case))


# ----------------------------------------------------------------------------------------------------------------------- the op
def _counting(L, names, calls):
    real = {n: getattr(L, n) for n in names}
    for n in names:
        setattr(L, n, (lambda name: lambda *a: calls.append((name, len(a))) or real[name](*a))(n))
    return real


@pytest.mark.parametrize("case", [SC.KERNEL_CASES[0], SC.KERNEL_CASES[1], SC.KERNEL_CASES[6]], ids=SC.case_id)
def test_op_counts_its_calls_and_hands_its_slot_on(npvp, refs, case):
    """untagged input: one npvp_amax pass and the launch; tagged input: the launch alone; conv3x3s2_packed behind it: no npvp_amax pass"""
    L, ops = npvp._lib.lib(), npvp.ops
    Ci, Co, H, W, Fr, act = case
    ins, ref = refs[case]
    x = ins["x"].to(DEV)
    bias = ins["bias"].to(DEV)
    planes, w_slot = ops.stem7x7_planes(ins["w"].to(DEV))
    w1 = (O.seeded_randn((64, Co, 3, 3), 3380) * (9 * Co) ** -0.5).to(DEV)
    b1 = O.seeded_randn((64,), 3381).to(DEV)
    planes1, w1_slot = ops.conv3x3s2_planes(w1)
    names = ("npvp_amax", "npvp_stem7x7_f16", "npvp_conv3x3s2_f16")
    calls = []
    real = _counting(L, names, calls)
    try:
        with torch.no_grad():
            y = ops.stem7x7_packed(x, planes, w_slot, bias, SC.ACT[act])
            assert calls == [("npvp_amax", 6), ("npvp_stem7x7_f16", 16)], calls
            del calls[:]
            z = ops.conv3x3s2_packed(y, planes1, w1_slot, b1, 1)
            assert calls == [("npvp_conv3x3s2_f16", 17)], calls
            del calls[:]
            xt = x.clone()
            ops.tag_amax(xt, ops.amax_of(xt.view(1, -1)))
            del calls[:]
            yt = ops.stem7x7_packed(xt, planes, w_slot, bias, SC.ACT[act])
            assert calls == [("npvp_stem7x7_f16", 16)], calls
            # the encoder's own call: the frames are a VIEW (N, T flattened) of a tensor whose producer tagged it
            x5 = torch.empty((1,) + tuple(x.shape), device=DEV).copy_(x)
            ops.tag_amax(x5, ops.amax_of(xt.view(1, -1)))
            del calls[:]
            yv = ops.stem7x7_packed(x5.flatten(0, 1), planes, w_slot, bias, SC.ACT[act])
            assert x5.flatten(0, 1)._base is x5 and calls == [("npvp_stem7x7_f16", 16)], calls
            assert torch.equal(yv, yt)
    finally:
        for n, f in real.items():
            setattr(L, n, f)
    torch.cuda.synchronize()
    assert y.shape == (Fr, Co, H, W) and y.is_contiguous(memory_format=torch.channels_last) and torch.equal(y, yt)
    e = SC.rel(y, ref)
    slot = ops.amax_of(y.permute(0, 2, 3, 1).reshape(-1, Co))
    assert slot is y._npvp_amax[0] and slot is y._base._npvp_amax[0] and slot.read() == float(y.abs().max())
    zref = (torch.nn.functional.conv2d(ref, w1.double().cpu(), stride=2, padding=1) + b1.double().cpu().view(1, -1, 1, 1)).clamp_min(0)
    ez = SC.rel(z, zref)
    SC.log_line(f"stem7x7_packed[{SC.case_id(case)}]: y {e:.3e} (bar {SC.F16X3_TOL:.0e}), conv3x3s2_packed behind it {ez:.3e} (bar {SC.BAR:.0e})")
    assert e < SC.F16X3_TOL and ez < SC.BAR, (e, ez)
    assert not hasattr(ops.stem7x7_packed(x, planes, w_slot, bias, SC.ACT[act], want_amax=False), "_npvp_amax")


def test_op_on_an_element_count_that_is_no_multiple_of_four(npvp, refs):
    """3 x 3 x 5 x 9 = 405 floats: the bound of the last float comes from a second npvp_amax pass over a padded copy of it"""
    ops = npvp.ops
    case = SC.KERNEL_CASES[2]
    ins, ref = refs[case]
    x = ins["x"].clone()
    x.view(-1)[-1] = 9.0                                              # the largest value is the ragged tail's
    planes, w_slot = ops.stem7x7_planes(ins["w"].to(DEV))
    ref9 = SC.ref64(case, ins=dict(ins, x=x))
    with torch.no_grad():
        y = ops.stem7x7_packed(x.to(DEV), planes, w_slot, ins["bias"].to(DEV), 1)
    assert SC.rel(y, ref9) < SC.F16X3_TOL


def test_op_checks_its_arguments(npvp):
    ops = npvp.ops
    case = SC.KERNEL_CASES[6]
    ins = SC.inputs(case)
    x = ins["x"].to(DEV)
    bias = ins["bias"].to(DEV)
    planes, w_slot = ops.stem7x7_planes(ins["w"].to(DEV))
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="planar"):
            ops.stem7x7_packed(x.contiguous(memory_format=torch.channels_last), planes, w_slot, bias)
        with pytest.raises(RuntimeError, match="planar"):
            ops.stem7x7_packed(x[:, :, ::2], planes, w_slot, bias)
        with pytest.raises(RuntimeError, match="at least 4"):
            ops.stem7x7_packed(x[:, :, :3].contiguous(), planes, w_slot, bias)
        with pytest.raises(RuntimeError, match="at least 4"):
            ops.stem7x7_packed(x[:, :, :, :3].contiguous(), planes, w_slot, bias)
        with pytest.raises(RuntimeError, match="16-byte boundary"):
            ops.stem7x7_packed(torch.zeros(x.numel() + 1, device=DEV)[1:].view(x.shape), planes, w_slot, bias)
        with pytest.raises(RuntimeError, match="act is 0"):
            ops.stem7x7_packed(x, planes, w_slot, bias, 2)
        with pytest.raises(RuntimeError, match="planes do not belong"):
            ops.stem7x7_packed(x, planes[:-8], w_slot, bias)
        with pytest.raises(RuntimeError, match="multiple of 32"):
            ops.stem7x7_packed(x, planes, w_slot, torch.zeros(48, device=DEV))
        with pytest.raises(RuntimeError, match="1 <= C_in <= 4"):
            ops.stem7x7_planes(torch.zeros(64, 5, 7, 7, device=DEV))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.stem7x7_packed(x.cpu(), planes, w_slot, bias)
    with pytest.raises(NotImplementedError, match="forward only"):
        ops.stem7x7_packed(x.clone().requires_grad_(), planes, w_slot, bias)
    assert ops.STEM7X7_ACTS == (0, 1) and ops.stem7x7_takes(1, 64) and ops.stem7x7_takes(3, 32) and not ops.stem7x7_takes(64, 3)


# ------------------------------------------------------------------------------------------------------------- whole encoders
@pytest.mark.parametrize("AE,ch,side,feat", [(AE_NGF64, 1, 16, (512, 2, 2)), (AE_NGF32, 3, 32, (512, 2, 2))], ids=["ngf64x3", "ngf32x4"])
def test_whole_encoder_hip_vs_stock(npvp, AE, ch, side, feat):
    """2 x 2 frames through the encoder: stem7x7="hip" against the stock pair, with every other route stock and with every other route hip"""
    x = torch.rand(2, 2, ch, side, side, generator=torch.Generator().manual_seed(3341)).to(DEV)
    feats = {}
    for key, routes in (("stock", dict(OTHERS_STOCK)), ("stem", dict(OTHERS_STOCK, stem7x7="hip")), ("all", dict(OTHERS_HIP, stem7x7="hip"))):
        enc, dec = npvp.build_frozen_autoencoder(AE, ch)
        O.key_hashed_fill(enc, 3342)
        enc, _ = npvp.to_device_layout(enc, dec, DEV, **routes)
        routed = [n for n, m in enc.named_modules() if getattr(m, "stem7x7", False)]
        assert routed == ([] if key == "stock" else ["block0.0"])
        with torch.no_grad():
            feats[key] = enc(x)
    assert feats["stock"].shape == (2, 2) + feat and float(feats["stock"].abs().max()) > 0
    for key in ("stem", "all"):
        e = SC.rel(feats[key], feats["stock"])
        SC.log_line(f"encoder ngf {AE['ngf']} / {AE['n_downsampling']} downsamplings, 4 frames of {side}x{side}x{ch}: stem7x7 hip, the other "
                    f"routes {'hip' if key == 'all' else 'stock'}, vs stock rel-L2 {e:.3e} (bar {SC.BAR:.0e})")
        assert e < SC.BAR, (key, e)


def test_routed_stem_refuses_grad_and_leaves_channels_last_on_stock(npvp, monkeypatch):
    enc, dec = npvp.build_frozen_autoencoder(AE_NGF32, 3)
    O.key_hashed_fill(enc, 3342)
    enc, _ = npvp.to_device_layout(enc, dec, DEV, stem7x7="hip")
    L = npvp._lib.lib()
    stem = enc.block0
    x = O.seeded_randn((2, 3, 8, 12), 3350).to(DEV)
    n0 = L.npvp_launch_count()
    with pytest.raises(NotImplementedError, match='stem7x7="hip".*inference-only'):
        stem(x.clone().requires_grad_())
    assert L.npvp_launch_count() == n0
    taken = []
    packed = npvp.ops.stem7x7_packed
    monkeypatch.setattr(npvp.ops, "stem7x7_packed", lambda *a, **k: (taken.append(1), packed(*a, **k))[1])
    with torch.no_grad():
        y = stem(x)
        assert y.shape == (2, 32, 8, 12) and y.is_contiguous(memory_format=torch.channels_last) and len(taken) == 1
        xcl = x.contiguous(memory_format=torch.channels_last)
        ycl = stem(xcl)                                               # channels-last, C_in = 3: the stock forward, no copy to planar
        assert len(taken) == 1, "the kernel was called on channels-last frames"
        try:
            stem[0].stem7x7 = False
            want = stem(x)
        finally:
            stem[0].stem7x7 = True
        e, es = SC.rel(y, want), SC.rel(ycl, want)
        SC.log_line(f"stem ngf 32, 2 frames of 8x12x3: hip vs stock {e:.3e}, channels-last input (stock forward) vs stock {es:.3e} (bar {SC.BAR:.0e})")
        assert e < SC.BAR and es < SC.BAR, (e, es)
