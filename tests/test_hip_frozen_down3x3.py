"""GPU: the frozen encoder's opt-in stride-2 3 x 3 convolution route (to_device_layout(..., down3x3="hip")): the kernel
npvp_conv3x3s2_f16 against the float64 reference of tests/frozen_down3x3_cases.py at the f16x3 bars of tests/test_hip_ops.py (written
exactly once, nothing behind y, bit-identical between launches, y_amax filled), the op's slot hand-over and argument checks, one routed
block2_conv-shaped FoldedConvAct against its float64 restatement, two whole encoders against the stock route, and what the routed
forward refuses or leaves alone.  NPVP_ERR_LOG=<file> appends the measured errors."""
import pytest
import torch

import frozen_down3x3_cases as DC
from oracle import ops as O
from test_hip_ops import ROW_TOL, close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL, TAIL = -12345.5, 4096
AE_SMMNIST = dict(ngf=64, n_downsampling=3, num_res_blocks=2, learn_3d=False, out_layer='Sigmoid')   # configs/config_SMMNIST_VFP_NPVP-S.yaml
AE_NGF32 = dict(ngf=32, n_downsampling=4, num_res_blocks=1, learn_3d=False, out_layer='Tanh')        # block1: C_in = 32
ALL_STOCK = dict(attn2d="stock", conv3x3="stock", down3x3="stock")
ALL_HIP = dict(attn2d="hip", conv3x3="hip", down3x3="hip")
DOWN_ONLY = dict(attn2d="stock", conv3x3="stock", down3x3="hip")


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
@pytest.mark.parametrize("case", DC.KERNEL_CASES, ids=DC.case_id)
def test_conv3x3s2_kernel_vs_float64(npvp, case):
    Ci, Co, H, W, Fr, act, res = case
    L, ops = npvp._lib.lib(), npvp.ops
    ins = DC.inputs(case)
    ref = _rows(DC.ref64(case, ins=ins))
    M = DC.rows(case)
    assert ref.shape == (M, Co)
    x = _rows(ins["x"]).to(DEV)
    planes, w_slot = ops.conv3x3s2_planes(ins["w"].to(DEV))
    assert planes.numel() * 2 == L.npvp_conv3x3s2_planes_bytes(Ci, Co)
    bias = ins["bias"].to(DEV)
    r = _rows(ins["res"]).to(DEV) if res else None
    x_slot = torch.zeros(512, device=DEV)
    assert L.npvp_amax(x.data_ptr(), Fr * H * W, Ci, Ci, x_slot.data_ptr(), _stream()) == 0
    assert float(w_slot.max()) == float(ins["w"].abs().max()) and float(x_slot.max()) == float(ins["x"].abs().max())

    def launch(want_amax):
        buf = torch.full((M * Co + TAIL,), SENTINEL, device=DEV)
        y_slot = torch.zeros(512, device=DEV) if want_amax else None
        rc = L.npvp_conv3x3s2_f16(x.data_ptr(), planes.data_ptr(), bias.data_ptr(), r.data_ptr() if res else None, buf.data_ptr(), Fr, H, W,
                                  Ci, Co, DC.ACT[act], x_slot.data_ptr(), w_slot.data_ptr(), y_slot.data_ptr() if want_amax else None,
                                  None, 0, _stream())
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
    e = DC.rel(y, ref)
    from golden_cases import max_row_rel_err
    DC.log_line(f"conv3x3s2[{DC.case_id(case)}] M {M}: rel-L2 {e:.3e}, worst row {max_row_rel_err(y.cpu(), ref.float()):.3e} "
                f"(bars {DC.F16X3_TOL:.0e} / {ROW_TOL:.0e})")
    close(y, ref, tol=DC.F16X3_TOL, what=DC.case_id(case))


def test_op_hands_its_slot_to_the_next_convolution_and_checks_its_arguments(npvp):
    """conv3x3s2_packed -> conv3x3_packed: the first op makes one npvp_amax launch for its untagged input, the second none - it finds the
    slot the first attached to its result"""
    L, ops = npvp._lib.lib(), npvp.ops
    case = DC.KERNEL_CASES[1]
    Ci, Co, H, W, Fr, act, res = case
    Ho, Wo = DC.out_extent(H), DC.out_extent(W)
    ins = DC.inputs(case)
    x = ins["x"].to(DEV).contiguous(memory_format=torch.channels_last)
    bias = ins["bias"].to(DEV)
    planes, w_slot = ops.conv3x3s2_planes(ins["w"].to(DEV))
    w1 = (O.seeded_randn((Co, Co, 3, 3), 1990) * (9 * Co) ** -0.5).to(DEV)
    b1 = O.seeded_randn((Co,), 1991).to(DEV)
    planes1, w1_slot = ops.conv3x3_planes(w1)
    names = ("npvp_amax", "npvp_conv3x3s2_f16", "npvp_conv3x3_f16")
    real = {n: getattr(L, n) for n in names}
    calls = []
    count = lambda name: lambda *a: calls.append((name, len(a))) or real[name](*a)
    try:
        for n in names:
            setattr(L, n, count(n))
        y = ops.conv3x3s2_packed(x, planes, w_slot, bias, DC.ACT[act])
        assert calls == [("npvp_amax", 6), ("npvp_conv3x3s2_f16", 17)], calls
        del calls[:]
        z = ops.conv3x3_packed(y, planes1, w1_slot, b1, "zero", 1, y)
        assert calls == [("npvp_conv3x3_f16", 18)], calls
    finally:
        for n, f in real.items():
            setattr(L, n, f)
    torch.cuda.synchronize()
    assert y.shape == (Fr, Co, Ho, Wo) and y.is_contiguous(memory_format=torch.channels_last)
    ref = DC.ref64(case, ins=ins)
    assert DC.rel(y, ref) < DC.F16X3_TOL
    slot = ops.amax_of(y.permute(0, 2, 3, 1).reshape(-1, Co))
    assert slot is y._npvp_amax[0] and slot is y._base._npvp_amax[0] and slot.read() == float(y.abs().max())
    zref = torch.nn.functional.conv2d(ref, w1.double().cpu(), padding=1) + b1.double().cpu().view(1, -1, 1, 1)
    assert DC.rel(z, zref.clamp_min(0) + ref) < DC.F16X3_TOL
    assert not hasattr(ops.conv3x3s2_packed(x, planes, w_slot, bias, 1, want_amax=False), "_npvp_amax")
    with pytest.raises(RuntimeError, match="channels-last"):
        ops.conv3x3s2_packed(ins["x"].to(DEV), planes, w_slot, bias)
    with pytest.raises(NotImplementedError, match="forward only"):
        ops.conv3x3s2_packed(x.clone().requires_grad_(), planes, w_slot, bias)
    with pytest.raises(RuntimeError, match="residual must be channels-last frames of the output's shape"):
        ops.conv3x3s2_packed(x, planes, w_slot, bias, 1, x)
    with pytest.raises(RuntimeError, match="planes do not belong"):
        ops.conv3x3s2_packed(x, planes[:-8], w_slot, bias)
    with pytest.raises(RuntimeError, match="C_in a multiple of 32"):
        ops.conv3x3s2_planes(torch.zeros(64, 48, 3, 3, device=DEV))


# ------------------------------------------------------------------------------------------------------------------ the modules
def test_routed_downsampling_convolution_vs_float64(npvp):
    """a block2_conv-shaped group (Conv2d(128, 256, 3, stride 2, padding 1) -> BatchNorm2d -> ReLU, eval mode) folded and routed,
    against the unfused modules in float64"""
    import copy
    import torch.nn as nn
    from npvp_amd.models.ResNetAutoEncoder import _fold_sequential, _route_down3x3
    seq = nn.Sequential(nn.Conv2d(DC.MODULE_CIN, DC.MODULE_COUT, 3, stride=2, padding=1, bias=False), nn.BatchNorm2d(DC.MODULE_COUT),
                        nn.ReLU(True)).eval()
    O.key_hashed_fill(seq, 1821)
    ref_mod = copy.deepcopy(seq).double()
    with torch.no_grad():
        folded = _fold_sequential(seq.to(DEV).to(memory_format=torch.channels_last))
    _route_down3x3(list(folded))
    assert folded[0].down3x3 and folded[0]._npvp_planes.is_cuda and folded[0].act == 1
    x = O.seeded_randn((DC.MODULE_FRAMES, DC.MODULE_CIN, DC.MODULE_GRID, DC.MODULE_GRID), 1830)
    L = npvp._lib.lib()
    n0 = L.npvp_launch_count()
    with torch.no_grad():
        out = folded(x.to(DEV).contiguous(memory_format=torch.channels_last))
        ref = ref_mod(x.double())
    assert L.npvp_launch_count() - n0 == 2, "one npvp_amax pass over the untagged input and the convolution"
    e = DC.rel(out, ref)
    DC.log_line(f"down3x3 hip block2_conv {DC.MODULE_CIN} -> {DC.MODULE_COUT} grid {DC.MODULE_GRID}: rel-L2 {e:.3e} (bar {DC.BAR:.0e})")
    assert out.shape == ref.shape == (DC.MODULE_FRAMES, DC.MODULE_COUT, DC.MODULE_GRID // 2, DC.MODULE_GRID // 2)
    assert float(ref.abs().max()) > 0 and e < DC.BAR, e


@pytest.mark.parametrize("AE,ch,side,feat", [(AE_SMMNIST, 1, 64, (512, 8, 8)), (AE_NGF32, 3, 64, (512, 4, 4))], ids=["smmnist", "ngf32x4"])
def test_whole_encoder_hip_vs_stock(npvp, AE, ch, side, feat):
    """4 frames through the encoder: all three switches at "hip" against all at "stock", and down3x3="hip" alone against stock"""
    x = torch.rand(2, 2, ch, side, side, generator=torch.Generator().manual_seed(1841)).to(DEV)
    L = npvp._lib.lib()
    feats = {}
    for key, routes in (("stock", ALL_STOCK), ("all", ALL_HIP), ("down", DOWN_ONLY)):
        enc, dec = npvp.build_frozen_autoencoder(AE, ch)
        O.key_hashed_fill(enc, 1842)
        enc, _ = npvp.to_device_layout(enc, dec, DEV, **routes)
        routed = [m for m in enc.modules() if getattr(m, "down3x3", False)]
        assert len(routed) == (0 if key == "stock" else AE["n_downsampling"])
        with torch.no_grad():
            feats[key] = enc(x)
    assert feats["stock"].shape == (2, 2) + feat and float(feats["stock"].abs().max()) > 0
    for key in ("all", "down"):
        e = DC.rel(feats[key], feats["stock"])
        DC.log_line(f"encoder ngf {AE['ngf']} / {AE['n_downsampling']} downsamplings, 4 frames of {side}x{side}x{ch}: "
                    f"{'attn2d, conv3x3 and down3x3' if key == 'all' else 'down3x3 alone'} hip vs stock rel-L2 {e:.3e} (bar {DC.BAR:.0e})")
        assert e < DC.BAR, (key, e)


def test_routed_forward_refuses_grad_and_leaves_nchw_on_stock(npvp, monkeypatch):
    enc, dec = npvp.build_frozen_autoencoder(AE_SMMNIST, 1)
    O.key_hashed_fill(enc, 1842)
    enc, _ = npvp.to_device_layout(enc, dec, DEV, down3x3="hip")
    L = npvp._lib.lib()
    blk = enc.block2_conv
    x = O.seeded_randn((1, 128, 6, 8), 1850).to(DEV)
    xg = x.contiguous(memory_format=torch.channels_last).requires_grad_()
    n0 = L.npvp_launch_count()
    with pytest.raises(NotImplementedError, match='down3x3="hip"'):
        blk(xg)
    assert L.npvp_launch_count() == n0
    taken = []
    packed = npvp.ops.conv3x3s2_packed
    monkeypatch.setattr(npvp.ops, "conv3x3s2_packed", lambda *a, **k: (taken.append(1), packed(*a, **k))[1])
    with torch.no_grad():
        y = blk(xg)
        assert y.shape == (1, 256, 3, 4) and torch.isfinite(y).all() and len(taken) == 1
        # NCHW-contiguous: the stock forward (F.conv2d + one npvp_bias_act pass), no copy to channels-last, the kernel not called.  As in
        # tests/test_hip_frozen_conv3x3.py F.conv2d is replaced by a deterministic stand-in for the bit comparison (MIOpen does not repeat
        # its own bits for NCHW frames with channels-last weights): everything around it is the code under test.
        real = torch.nn.functional.conv2d
        convs = []

        def conv2d64(inp, w, *a):
            convs.append((tuple(inp.shape), inp.is_contiguous(), tuple(a)))
            return real(inp.double().cpu(), w.double().cpu(), *a).float().to(inp.device).contiguous(memory_format=torch.channels_last)
        monkeypatch.setattr(torch.nn.functional, "conv2d", conv2d64)
        del taken[:]
        n0 = L.npvp_launch_count()
        y = blk(x)
        assert L.npvp_launch_count() - n0 == 1 and not taken and len(convs) == 1 and convs[0][:2] == ((1, 128, 6, 8), True)
        assert convs[0][2][1:3] == ((2, 2), (1, 1))
        try:
            blk[0].down3x3 = False
            want = blk(x)
        finally:
            blk[0].down3x3 = True
        assert convs[1:] == convs[:1] and torch.equal(y, want)
        assert DC.rel(y, blk(xg)) < DC.BAR
