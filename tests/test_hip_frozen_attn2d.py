"""GPU: the frozen encoder's opt-in NonLocalAttenion2D route (to_device_layout(..., attn2d="hip")): the epilogue kernel
npvp_bias_act_scaled against float64 and against npvp_bias_act's bits, one routed attn2d against the float64 restatement of
tests/frozen_attn2d_cases.py, the whole pair against the reference's vectors and against the stock route, the memory and launch
counts that tell the routes apart, and the Stage-2 steps from pixels under either route.
NPVP_ERR_LOG=<file> appends the measured errors (profiles/frozen_attn2d_errors.txt)."""
import functools

import pytest
import torch

import ae3d_cases as AC
import frozen_attn2d_cases as FC
import golden_cases as GC
from oracle import ops as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MiB = 1 << 20
LOSS_TOL = 1e-4             # the step tolerance of tests/test_hip_ae3d.py (LOSS_TOL) and of tests/test_hip_golden.py (TOL)


@pytest.fixture(scope="module")
def npvp():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import npvp_amd
    return npvp_amd


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------------- the kernel
def _device_case(case):
    """x (at its offset inside a 16-byte aligned buffer), bias, residual and the planted scale on the device"""
    name, layout, outer, inner, C, off = case
    i = FC.kernel_inputs(case)
    buf = torch.empty(outer * inner + off, device=DEV)
    x = buf[off:]
    x.copy_(i["x"].flatten())
    assert x.data_ptr() % 16 == 4 * (off % 4)
    return dict(x=x, bias=i["bias"].to(DEV), res=i["res"].to(DEV), scale=torch.tensor([FC.SCALE], device=DEV), host=i)


def _scaled(L, case, d, act, scale, residual):
    """npvp_bias_act_scaled into a NaN-filled output; every element must have been written"""
    name, layout, outer, inner, C, off = case
    out = torch.full((outer, inner), float("nan"), device=DEV)
    rc = L.npvp_bias_act_scaled(d["x"].data_ptr(), d["bias"].data_ptr(), d["scale"].data_ptr() if scale else None,
                                d["res"].data_ptr() if residual else None, out.data_ptr(), outer, inner, C, layout, act, _stream())
    assert rc == 0, L.npvp_last_error()
    assert not bool(torch.isnan(out).any()), f"{name}: an element was left unwritten (act {act}, scale {scale}, residual {residual})"
    return out


def _plain(L, case, d, act, residual):
    name, layout, outer, inner, C, off = case
    out = torch.empty((outer, inner), device=DEV)
    rc = L.npvp_bias_act(d["x"].data_ptr(), d["bias"].data_ptr(), d["res"].data_ptr() if residual else None, out.data_ptr(), outer, inner,
                         C, layout, act, _stream())
    assert rc == 0, L.npvp_last_error()
    return out


def _check_combo(L, case, d, act, scale, residual):
    """act 0 / 1: against float64 within the two roundings.  tanh / sigmoid: no tolerance of its own for the device functions -
    against s * a + r formed in float64 from npvp_bias_act's act-only output a.  scale NULL: npvp_bias_act's bits, every act."""
    got = _scaled(L, case, d, act, scale, residual)
    if not scale:
        assert torch.equal(got, _plain(L, case, d, act, residual)), (case[0], act, residual, "differs from npvp_bias_act")
    s = FC.SCALE if scale else 1.0
    if act in (0, 1):
        ref, a = FC.kernel_ref64(case, act, s, residual)
    else:
        a = _plain(L, case, d, act, False).cpu().double()
        ref = s * a + (d["host"]["res"].double() if residual else 0.0)
    err = (got.cpu().double() - ref).abs()
    ratio = float((err / FC.two_rounding_bound(s, a, ref).clamp_min(1e-300)).max())
    return ratio, float(err.max())


@pytest.mark.parametrize("case", FC.SMALL_KERNEL_CASES, ids=lambda c: c[0])
def test_bias_act_scaled_kernel(npvp, case):
    """both kernel forms (vector; scalar by shape, by alignment and by layout), every act, scale NULL and planted, residual NULL and
    present"""
    L, d = npvp._lib.lib(), _device_case(case)
    assert FC.kernel_is_vector(case) == (case[3] % 4 == 0 and d["x"].data_ptr() % 16 == 0)
    n0 = L.npvp_launch_count()
    worst = 0.0
    for act in range(4):
        for scale in (False, True):
            for residual in (False, True):
                ratio, e = _check_combo(L, case, d, act, scale, residual)
                worst = max(worst, ratio)
                assert ratio <= 1.0, (case[0], act, scale, residual, ratio, e)
    assert L.npvp_launch_count() - n0 >= 32
    FC.log_line(f"bias_act_scaled[{case[0]}] 32 combinations: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("case", FC.LOOP_KERNEL_CASES, ids=lambda c: c[0])
def test_bias_act_scaled_grid_stride_loop(npvp, case):
    """more work than the capped grid has threads: the loop's second trip (the vector case holds over 16384 * 256 * 4 elements)"""
    L, d = npvp._lib.lib(), _device_case(case)
    assert FC.kernel_work(case) > FC.GRID_CAP
    for act, scale, residual in ((1, True, True), (3, False, False)):
        ratio, e = _check_combo(L, case, d, act, scale, residual)
        FC.log_line(f"bias_act_scaled[{case[0]}] act {act} scale {scale} residual {residual}: max error {e:.3e}, error / bound {ratio:.3f}")
        assert ratio <= 1.0, (case[0], act, ratio, e)


def test_op_takes_both_memory_formats_and_refuses_grad(npvp):
    x, b, r = O.seeded_randn((2, 8, 3, 5), 1).to(DEV), O.seeded_randn((8,), 2).to(DEV), O.seeded_randn((2, 8, 3, 5), 3).to(DEV)
    s = torch.tensor(FC.SCALE, device=DEV)
    want = r.double() + FC.SCALE * torch.relu(x.double() + b.double().view(1, 8, 1, 1))
    for fmt in (torch.contiguous_format, torch.channels_last):
        y = npvp.ops.bias_act_scaled(x.contiguous(memory_format=fmt), b, s, 1, residual=r.contiguous(memory_format=fmt))
        assert y.is_contiguous(memory_format=fmt) and FC.rel(y, want) < 1e-6
    assert torch.equal(npvp.ops.bias_act_scaled(x, b, None, 2), npvp.ops.bias_act(x, b, 2))
    with pytest.raises(NotImplementedError, match="forward only"):
        npvp.ops.bias_act_scaled(x.clone().requires_grad_(), b, s)


# ------------------------------------------------------------------------------------------------------------------- the module
def _routed(npvp, C, attn2d):
    """(block on the device with its attn2d on the given route, float64 parameters of the unfused attention)"""
    blk = FC.make_block(C)
    p = FC.params64(blk.attn2d)
    enc, _ = npvp.to_device_layout(FC.Holder(blk), FC.Holder(), DEV, attn2d=attn2d)
    return enc.blk, p


@pytest.mark.parametrize("shape", FC.MODULE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_routed_attn2d_vs_float64(npvp, shape):
    """the attention branch out - x of one hip-routed attn2d against the float64 restatement at the frozen pair's forward bar"""
    C, H, W, Fr = shape
    blk, p = _routed(npvp, C, "hip")
    a = blk.attn2d
    assert "forward" in a.__dict__ and float(a.gamma) == FC.GAMMA
    x = FC.module_input(shape)
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    L = npvp._lib.lib()
    n0 = L.npvp_launch_count()
    with torch.no_grad():
        out = a(xd)
        ref = FC.attn2d_ref64(p, x)
    assert L.npvp_launch_count() - n0 >= 2, "the attention core and the epilogue are library launches"
    assert out.shape == x.shape and out.is_contiguous(memory_format=torch.channels_last)
    e = FC.rel(out.cpu().double() - x.double(), ref - x.double())
    route = "config" if npvp.ops.nonlocal_attn_config_shape(C // 8, C // 2, H, W) else "grid"
    FC.log_line(f"attn2d hip vs float64 C {C} grid {H}x{W} frames {Fr} ({route} kernels): branch rel-L2 {e:.3e} (bar {FC.BAR:.0e})")
    assert e < FC.BAR, e


# --------------------------------------------------------------------------------------------------------------------- the pair
@pytest.mark.parametrize("tag", ["64", "128"])
def test_frozen_pair_hip_route_vs_the_reference_vectors(npvp, tag):
    """tests/test_hip_golden.py::test_frozen_autoencoder with the encoder's attn2d on the HIP route, at that test's bars; and the
    hip-routed encoder against the stock-routed one on the same frames"""
    res = GC.case_ae(npvp, DEV, tag, device_layout=functools.partial(npvp.to_device_layout, attn2d="hip"))
    gold = GC.load(f"ae_{tag}")
    g_res, g_gold = res.pop("g_feats"), gold.pop("g_feats")
    worst = GC.compare(res, gold, 1e-4, tag=f"ae_{tag}[attn2d=hip]")
    GC.compare({"g_feats": g_res}, {"g_feats": g_gold}, 5e-3, tag=f"ae_{tag}.g_feats[attn2d=hip]")
    ci, ngf, nd, nres, S = {"64": (1, 64, 3, 2, 64), "128": (3, 32, 4, 3, 128)}[tag]
    x = torch.rand(1, 2, ci, S, S, generator=torch.Generator().manual_seed(123)).to(DEV)
    feats = {}
    for route in ("stock", "hip"):
        enc = O.key_hashed_fill(npvp.ResnetEncoder(ci, ngf=ngf, n_downsampling=nd, num_res_blocks=nres, learn_3d=False), 121).eval()
        dec = npvp.ResnetDecoder(ci, ngf=ngf, n_downsampling=nd).eval()
        enc, _ = npvp.to_device_layout(enc, dec, DEV, attn2d=route)
        attns = [m.attn2d for m in enc.children() if isinstance(m, npvp.models.Factorized3DConvAttn)]
        assert len(attns) == nd - 1 + nres and all(("forward" in a.__dict__) == (route == "hip") for a in attns)
        assert all(abs(float(a.gamma)) > 1e-3 for a in attns), "a zero gamma switches the attention branch off: nothing is compared"
        with torch.no_grad():
            feats[route] = enc(x)
    e = FC.rel(feats["hip"], feats["stock"])
    FC.log_line(f"frozen pair ae_{tag}: hip route vs reference vectors worst key {worst:.3e}, hip vs stock encoder {e:.3e} (bars 1e-4)")
    assert torch.equal(feats["hip"], res["feats"]) or FC.rel(feats["hip"], res["feats"]) < 1e-4
    assert e < 1e-4, e


# ------------------------------------------------------------------------------------------------- what tells the routes apart
def test_hip_route_allocates_no_score_tensor_and_launches_library_kernels(npvp):
    """one attn2d at C 64 on 4 frames of 64 x 64: a score tensor is F * HW * HW/4 * 4 B = 64 MiB.  The stock forward's peak over
    the allocation level before the call reaches it (the probe sees the tensor); the hip route's stays below it.  The hip route
    launches at least two library kernels per call, the stock forward none."""
    C, H, W, Fr = 64, 64, 64, 4
    score_bytes = Fr * H * W * (H * W // 4) * 4
    assert score_bytes == 64 * MiB
    x = O.seeded_randn((Fr, C, H, W), 77).to(DEV).contiguous(memory_format=torch.channels_last)
    L = npvp._lib.lib()
    peaks, launches, outs = {}, {}, {}
    for route in ("stock", "hip"):
        a = _routed(npvp, C, route)[0].attn2d
        with torch.no_grad():
            a(x)                                    # warm-up: library handles and workspaces are allocated here
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            n0 = L.npvp_launch_count()
            outs[route] = a(x)
            torch.cuda.synchronize()
        launches[route] = L.npvp_launch_count() - n0
        peaks[route] = torch.cuda.max_memory_allocated() - base
    FC.log_line(f"attn2d C 64, 64x64, 4 frames: peak over the level before the call: stock {peaks['stock'] / MiB:.1f} MiB, "
                f"hip {peaks['hip'] / MiB:.1f} MiB (one score tensor: 64 MiB); library launches per call: {launches}")
    assert peaks["stock"] >= score_bytes, peaks
    assert peaks["hip"] < score_bytes, peaks
    assert launches["hip"] >= 2 and launches["stock"] == 0, launches
    assert FC.rel(outs["hip"] - x, outs["stock"] - x) < FC.BAR


def test_hip_routed_attn2d_refuses_an_input_that_requires_grad(npvp):
    a = _routed(npvp, 64, "hip")[0].attn2d
    x = O.seeded_randn((1, 64, 4, 6), 4).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_()
    L = npvp._lib.lib()
    n0 = L.npvp_launch_count()
    with pytest.raises(NotImplementedError, match='attn2d="hip"'):
        a(x)
    assert L.npvp_launch_count() == n0
    with torch.no_grad():
        assert torch.isfinite(a(x)).all()
    nchw = O.seeded_randn((1, 64, 4, 6), 5).to(DEV)            # not channels-last: the stock forward, no library launch, no copy
    n0 = L.npvp_launch_count()
    with torch.no_grad():
        y = a(nchw)
    assert L.npvp_launch_count() == n0 and y.is_contiguous()


# -------------------------------------------------------------------------------------------------------------------- the steps
def _pair(npvp, route):
    enc, dec = npvp.build_frozen_autoencoder(dict(AC.AE64_3D, out_layer='Sigmoid'), 1)
    O.key_hashed_fill(enc, 121); O.key_hashed_fill(dec, 122)
    return npvp.to_device_layout(enc, dec, DEV, attn2d=route)


@pytest.fixture(scope="module")
def pairs(npvp):
    return {route: _pair(npvp, route) for route in ("stock", "hip")}


def _clips():
    g_ = torch.Generator().manual_seed(153)
    return torch.rand(1, 3, 1, 64, 64, generator=g_).to(DEV), torch.rand(1, 4, 1, 64, 64, generator=g_).to(DEV)


def test_val_and_sample_steps_agree_between_the_routes(npvp, pairs):
    """full_val_step (a small deterministic predictor, as tests/test_hip_ae3d.py::test_full_val_step_with_a_3d_pair) and
    full_sample_step (a stochastic one): pred within 1e-4 rel-L2 between attn2d="stock" and "hip" """
    pf, ff = _clips()
    m = GC._small_predictor(npvp, False, 151, DEV)
    val = {r: npvp.full_val_step(m, *pairs[r], pf, ff, 0.01, 1e-6) for r in pairs}
    e = FC.rel(val["hip"]["pred"], val["stock"]["pred"])
    ms = GC._small_predictor(npvp, True, 151, DEV)
    smp = {r: npvp.full_sample_step(ms, *pairs[r], pf, 2, seed=7) for r in pairs}
    es = FC.rel(smp["hip"], smp["stock"])
    FC.log_line(f"full_val_step pred hip vs stock {e:.3e}, full_sample_step frames hip vs stock {es:.3e} (bar 1e-4)")
    assert torch.isfinite(val["hip"]["pred"]).all() and e < 1e-4, e
    assert smp["hip"].shape[:3] == (1, 2, 4) and es < 1e-4, es
    for k in ("loss", "Image_L1", "PF_L1"):
        assert abs(float(val["hip"][k]) - float(val["stock"][k])) <= LOSS_TOL * abs(float(val["stock"][k])), k


def test_train_step_gives_the_same_losses_under_either_route(npvp, pairs):
    pf, ff = _clips()
    eps = O.seeded_randn((1, 512, 8, 8), 154).to(DEV)
    got = {}
    for r in pairs:
        m = GC._small_predictor(npvp, True, 131, DEV)
        m.evt_prior.eps_fn = m.evt_posterior.eps_fn = lambda shape: eps
        m.train()
        opt = npvp.FlatAdamW(m, lr=1e-4, clip_module=m.transformer, max_grad_norm=1.0)
        got[r] = npvp.full_train_step(m, opt, *pairs[r], pf, ff, 0.01, 1e-6, 1.0)
    FC.log_line("full_train_step hip vs stock: " + ", ".join(
        f"{k} {abs(float(got['hip'][k]) - float(got['stock'][k])) / abs(float(got['stock'][k])):.2e}" for k in ("loss", "Image_L1", "PF_L1", "KL")))
    for k in ("loss", "Image_L1", "PF_L1", "KL"):
        assert abs(float(got["hip"][k]) - float(got["stock"][k])) <= LOSS_TOL * abs(float(got["stock"][k])), (k, got)


def test_attn1d_does_not_move_with_the_switch(npvp, pairs):
    """attn2d="hip" on a learn_3d=True pair: the same attn1d buffers, and attn1d's output on the same frames bit for bit"""
    from npvp_amd.models.ResNetAutoEncoder import _fused_attn1d
    T = 3
    n = 0
    for (name, s), (_, h) in zip(pairs["stock"][0].named_children(), pairs["hip"][0].named_children()):
        if not isinstance(s, npvp.models.Factorized3DConvAttn):
            continue
        n += 1
        assert "forward" in h.attn2d.__dict__ and "forward" not in s.attn2d.__dict__ and "forward" not in h.attn1d.__dict__
        assert torch.equal(s.attn1d._npvp_wqkv, h.attn1d._npvp_wqkv) and torch.equal(s.attn1d._npvp_bqkv, h.attn1d._npvp_bqkv)
        x = O.seeded_randn((2 * T, s.in_channels, 4, 4), 90 + n).to(DEV).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            assert torch.equal(_fused_attn1d(s.attn1d, x, T), _fused_attn1d(h.attn1d, x, T)), name
    assert n == 4
