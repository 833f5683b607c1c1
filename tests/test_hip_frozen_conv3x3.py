"""GPU: the frozen encoder's opt-in 3 x 3 convolution route (to_device_layout(..., conv3x3="hip")): the implicit-GEMM kernel
npvp_conv3x3_f16 against the float64 reference of tests/frozen_conv3x3_cases.py at the f16x3 bars of tests/test_hip_ops.py (written
exactly once, bit-identical between launches, y_amax filled), one routed Factorized3DConvAttn and one routed ResnetBlock against their
float64 restatement, the whole SM-MNIST-sized encoder against the stock route, and what the routed forward refuses or leaves alone.
NPVP_ERR_LOG=<file> appends the measured errors."""
import copy

import pytest
import torch

import frozen_conv3x3_cases as CC
from oracle import ops as O
from test_hip_ops import ROW_TOL, close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL, TAIL = -12345.5, 4096
AE_BLOCKS = dict(ngf=64, n_downsampling=3, num_res_blocks=1, learn_3d=False, out_layer='Tanh')       # C = 512 behind three downsamplings
AE_SMMNIST = dict(ngf=64, n_downsampling=3, num_res_blocks=2, learn_3d=False, out_layer='Sigmoid')   # configs/config_SMMNIST_VFP_NPVP-S.yaml


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


# ------------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("case", CC.KERNEL_CASES, ids=CC.case_id)
def test_conv3x3_kernel_vs_float64(npvp, case):
    Ci, Co, H, W, Fr, pad, act, res = case
    L, ops = npvp._lib.lib(), npvp.ops
    ins = CC.inputs(case)
    ref = _rows(CC.ref64(case, ins=ins))
    M = CC.rows(case)
    x = _rows(ins["x"]).to(DEV)
    planes, w_slot = ops.conv3x3_planes(ins["w"].to(DEV))
    assert planes.numel() * 2 == L.npvp_conv3x3_planes_bytes(Ci, Co)
    bias = ins["bias"].to(DEV)
    r = _rows(ins["res"]).to(DEV) if res else None
    x_slot = torch.zeros(512, device=DEV)
    assert L.npvp_amax(x.data_ptr(), M, Ci, Ci, x_slot.data_ptr(), _stream()) == 0
    assert float(w_slot.max()) == float(ins["w"].abs().max()) and float(x_slot.max()) == float(ins["x"].abs().max())

    def launch(want_amax):
        buf = torch.full((M * Co + TAIL,), SENTINEL, device=DEV)
        y_slot = torch.zeros(512, device=DEV) if want_amax else None
        rc = L.npvp_conv3x3_f16(x.data_ptr(), planes.data_ptr(), bias.data_ptr(), r.data_ptr() if res else None, buf.data_ptr(), Fr, H, W,
                                Ci, Co, CC.PAD_MODE[pad], CC.ACT[act], x_slot.data_ptr(), w_slot.data_ptr(),
                                y_slot.data_ptr() if want_amax else None, None, 0, _stream())
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
    e = CC.rel(y, ref)
    from golden_cases import max_row_rel_err
    CC.log_line(f"conv3x3[{CC.case_id(case)}] M {M}: rel-L2 {e:.3e}, worst row {max_row_rel_err(y.cpu(), ref.float()):.3e} "
                f"(bars {CC.F16X3_TOL:.0e} / {ROW_TOL:.0e})")
    close(y, ref, tol=CC.F16X3_TOL, what=CC.case_id(case))


def test_op_attaches_the_slot_and_checks_its_arguments(npvp):
    ops = npvp.ops
    case = CC.KERNEL_CASES[6]
    Ci, Co, H, W, Fr, pad, act, res = case
    ins = CC.inputs(case)
    x = ins["x"].to(DEV).contiguous(memory_format=torch.channels_last)
    r = ins["res"].to(DEV).contiguous(memory_format=torch.channels_last)
    planes, w_slot = ops.conv3x3_planes(ins["w"].to(DEV))
    y = ops.conv3x3_packed(x, planes, w_slot, ins["bias"].to(DEV), pad, CC.ACT[act], r)
    assert y.shape == (Fr, Co, H, W) and y.is_contiguous(memory_format=torch.channels_last)
    assert CC.rel(y, CC.ref64(case, ins=ins)) < CC.F16X3_TOL
    slot = ops.amax_of(y.permute(0, 2, 3, 1).reshape(-1, Co))
    assert slot is y._npvp_amax[0] and slot.read() == float(y.abs().max())
    with pytest.raises(RuntimeError, match="channels-last"):
        ops.conv3x3_packed(ins["x"].to(DEV), planes, w_slot, ins["bias"].to(DEV), pad)
    with pytest.raises(NotImplementedError, match="forward only"):
        ops.conv3x3_packed(x.clone().requires_grad_(), planes, w_slot, ins["bias"].to(DEV), pad)


# ------------------------------------------------------------------------------------------------------------------ the modules
@pytest.fixture(scope="module")
def blocks(npvp):
    """(unfused CPU encoder, the same encoder fused on the device under conv3x3="hip")"""
    enc, dec = npvp.build_frozen_autoencoder(AE_BLOCKS, 1)
    O.key_hashed_fill(enc, 821)
    raw = copy.deepcopy(enc)
    hip, _ = npvp.to_device_layout(enc, dec, DEV, conv3x3="hip")
    return raw, hip


@pytest.mark.parametrize("name", ["res_3dConvAttn_0", "res_conv_0"])
def test_routed_block_vs_float64(npvp, blocks, name):
    """one Factorized3DConvAttn(512) at 8 x 8 (spatial_conv: zero padding, ReLU, skip) and one ResnetBlock(512) (two reflection-padded
    convolutions, the second with the skip) of a fused pair against the unfused module in float64"""
    raw, hip = blocks
    x = O.seeded_randn((CC.MODULE_FRAMES, CC.MODULE_C, CC.MODULE_GRID, CC.MODULE_GRID), 830)
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    L = npvp._lib.lib()
    mod, ref_mod = getattr(hip, name), copy.deepcopy(getattr(raw, name)).double()
    convs = [mod.spatial_conv] if name.startswith("res_3d") else list(mod.conv_block)
    assert all(c.conv3x3_pad is not None and c._npvp_planes is not None and c._npvp_planes.is_cuda for c in convs)
    n0 = L.npvp_launch_count()
    with torch.no_grad():
        if name.startswith("res_3d"):
            out, ref = mod(xd, 1), ref_mod(x.double(), 1)
        else:
            out, ref = mod(xd), ref_mod(x.double())
    assert L.npvp_launch_count() - n0 >= len(convs)
    e = CC.rel(out.cpu().double() - x.double(), ref - x.double())
    CC.log_line(f"conv3x3 hip {name} C {CC.MODULE_C} grid {CC.MODULE_GRID}: branch rel-L2 {e:.3e} (bar {CC.BAR:.0e})")
    assert out.shape == x.shape and e < CC.BAR, e


def test_whole_encoder_hip_vs_stock(npvp):
    """the SM-MNIST-sized encoder on 2 x 2 frames of 64 x 64: conv3x3="hip" against "stock" at the frozen pair's bar"""
    x = torch.rand(2, 2, 1, 64, 64, generator=torch.Generator().manual_seed(841)).to(DEV)
    feats = {}
    for route in ("stock", "hip"):
        enc, dec = npvp.build_frozen_autoencoder(AE_SMMNIST, 1)
        O.key_hashed_fill(enc, 842)
        enc, _ = npvp.to_device_layout(enc, dec, DEV, conv3x3=route)
        routed = [m for m in enc.modules() if getattr(m, "conv3x3_pad", None) is not None]
        assert len(routed) == (8 if route == "hip" else 0)
        with torch.no_grad():
            feats[route] = enc(x)
    e = CC.rel(feats["hip"], feats["stock"])
    CC.log_line(f"SM-MNIST encoder, 4 frames: conv3x3 hip vs stock rel-L2 {e:.3e} (bar {CC.BAR:.0e})")
    assert feats["hip"].shape == (2, 2, 512, 8, 8) and float(feats["stock"].abs().max()) > 0 and e < CC.BAR, e


def test_routed_forward_refuses_grad_and_leaves_nchw_on_stock(npvp, blocks, monkeypatch):
    raw, hip = blocks
    L = npvp._lib.lib()
    blk = hip.res_conv_0
    x = O.seeded_randn((1, 512, 4, 6), 850).to(DEV)
    xg = x.contiguous(memory_format=torch.channels_last).requires_grad_()
    n0 = L.npvp_launch_count()
    with pytest.raises(NotImplementedError, match='conv3x3="hip"'):
        blk(xg)
    assert L.npvp_launch_count() == n0
    taken = []
    packed = npvp.ops.conv3x3_packed
    monkeypatch.setattr(npvp.ops, "conv3x3_packed", lambda *a, **k: (taken.append(1), packed(*a, **k))[1])
    with torch.no_grad():
        assert torch.isfinite(blk(xg)).all() and len(taken) == 2
        # NCHW-contiguous: the stock forward (F.conv2d + two npvp_bias_act passes), no copy to channels-last, the kernel not called -
        # bit for bit what the same module gives with its routing switched off.  MIOpen's kernels for this mixed layout (NCHW frames,
        # channels-last weights) do not repeat their own bits from call to call (logged below), so for the comparison F.conv2d is a
        # deterministic stand-in (float64 on the host): everything around it is the code under test.
        rep = torch.equal(blk(x), blk(x))
        CC.log_line(f"NCHW input: two stock forwards through MIOpen give the same bits: {rep}")
        real = torch.nn.functional.conv2d
        convs = []

        def conv2d64(inp, w, *a):
            convs.append((tuple(inp.shape), inp.is_contiguous(), tuple(a)))
            return real(inp.double().cpu(), w.double().cpu(), *a).float().to(inp.device).contiguous(memory_format=torch.channels_last)
        monkeypatch.setattr(torch.nn.functional, "conv2d", conv2d64)
        del taken[:]
        n0 = L.npvp_launch_count()
        y = blk(x)
        assert L.npvp_launch_count() - n0 == 2 and not taken and len(convs) == 2 and convs[0][:2] == ((1, 512, 6, 8), True)
        marks = [(c, c.conv3x3_pad) for c in blk.conv_block]
        try:
            for c, _ in marks:
                c.conv3x3_pad = None
            want = blk(x)
        finally:
            for c, p in marks:
                c.conv3x3_pad = p
        assert convs[2:] == convs[:2] and torch.equal(y, want)
        monkeypatch.setattr(torch.nn.functional, "conv2d", real)
        stock, _ = npvp.to_device_layout(copy.deepcopy(raw), npvp.build_frozen_autoencoder(AE_BLOCKS, 1)[1], DEV)
        CC.log_line(f"NCHW input: routed module vs a stock-fused twin rel-L2 {CC.rel(y, stock.res_conv_0(x)):.3e}")
