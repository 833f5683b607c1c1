"""GPU: the norm, depthwise-conv, im2col and attention kernels that a feature grid other than 8 x 8 falls back to, as kernels -
through the npvp_amd.ops call sites the models use, forward values and EVERY gradient (parameters included) against the float64
CPU oracle, at 1e-5 on the whole tensor and on the worst row.  Cases, references, bound and comparison: tests/grid_kernel_cases.py;
tests/test_grid_kernel_cases_host.py shows that those cases reject a wrong kernel.  One recorded run: profiles/grid_kernels_errors.txt."""
import pytest
import torch

import grid_kernel_cases as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def K():
    """no GEMM below: one arithmetic mode (the default), one seed for the drop-path masks"""
    import npvp_amd  # noqa: F401
    from npvp_amd import ops
    assert torch.cuda.is_available()
    ops.set_gemm_precision("f16x3")
    ops.rng.manual_seed(1234, torch.device(DEV))
    yield ops


def dev(i):
    """the leaves of a case's inputs on the device (cotangents and None as they are)"""
    return {k: (None if t is None else t.detach().to(DEV).requires_grad_(t.requires_grad)) for k, t in i.items()}


def grads(y, cot, leaves):
    names = [k for k, v in leaves.items() if v is not None]
    return dict(zip(names, torch.autograd.grad((y * cot).sum(), [leaves[k] for k in names])))


# ------------------------------------------------------------------------------------------------------------------- depthwise 3x3
@pytest.mark.parametrize("case", G.DWCONV, ids=G.case_id)
def test_dwconv(K, case):
    """dwconv3x3_kernel forward and (taps flipped) input gradient, dwconv3x3_wgrad_kernel + the sum of its chunk partials"""
    Fr, H, W, Ch = case
    i = dev(G.dwconv_inputs(case))
    wtb = torch.cat([i["w"].detach().reshape(Ch, 9).t(), i["b"].detach().reshape(1, Ch)], 0).contiguous().requires_grad_()
    y = K.dwconv3x3(i["a"], wtb, Fr, H, W)
    g = grads(y, i["cot"], dict(da=i["a"], dwtb=wtb))
    G.close_all("dwconv", case, dict(y=y, da=g["da"], dw=g["dwtb"][:9], db=g["dwtb"][9]))


# ------------------------------------------------------------------------------------------------------------------- im2col
@pytest.mark.parametrize("case", G.IM2COL, ids=G.case_id)
def test_im2col_and_col2im(K, case):
    """im2col copies: EQUAL to the fp32 reference; col2im (sums of up to 9 values) within the bound; and the two are adjoint"""
    Fr, H, W, C = case
    i = dev(G.im2col_inputs(case))
    cols = K.im2col3x3(i["x"], Fr, H, W)
    dx = torch.autograd.grad((cols * i["cot"]).sum(), [i["x"]])[0]
    assert torch.equal(cols.detach().cpu(), G.ref32("im2col", case)["cols"])
    G.close_all("im2col", case, dict(cols=cols, dx=dx))
    # <im2col(x), y> = <x, col2im(y)>: the left side is exact up to the float64 sum, so the right may differ from it by
    # <x, dx - col2im(y)>, at most |x| |dx - col2im(y)| <= BOUND |x| |col2im(y)|
    x64, y64 = i["x"].detach().double().cpu(), i["cot"].double().cpu()
    lhs, rhs = float((cols.detach().double().cpu() * y64).sum()), float((x64 * dx.double().cpu()).sum())
    assert abs(lhs - rhs) <= G.BOUND * float(x64.norm() * G.ref64("im2col", case)["dx"].norm()), (lhs, rhs)


# ------------------------------------------------------------------------------------------------------------------- posfuse
def run_posfuse(fn, family, case):
    N, T = case[0], case[1]
    i = dev(G.posfuse_inputs(family, case))
    y = fn(i["x"], i["add"], i["beta"], i["gamma"], N, T)
    out = grads(y, i["cot"], dict(dx=i["x"], dadd=i["add"], dbeta=i["beta"], dgamma=i["gamma"]))
    out["y"] = y
    return out


@pytest.mark.parametrize("case", G.POSFUSE_LAYER, ids=G.case_id)
def test_posfuse_layer(K, case):
    """frame_stats_kernel + posfuse_apply_kernel; backward: posfuse_bwd_apply_kernel + the two batch reductions, or the fused
    apply with the batch loop in the thread - whichever npvp_posfuse_bwd_fused says"""
    G.close_all("posfuse_layer", case, run_posfuse(K.posfuse, "posfuse_layer", case))


@pytest.mark.parametrize("case", G.POSFUSE_INSTANCE, ids=G.case_id)
def test_posfuse_instance(K, case):
    G.close_all("posfuse_instance", case, run_posfuse(K.posfuse_instance, "posfuse_instance", case))


def test_posfuse_instance_refuses_more_than_64_pixels(K):
    P = G.POSFUSE_INSTANCE_TOO_MANY_PIXELS
    x = torch.zeros(2, P, 256, device=DEV)
    with pytest.raises(RuntimeError, match=r"P <= 64"):
        K.posfuse_instance(x, None, torch.zeros(P, 256, device=DEV), None, 2, 1)


# ------------------------------------------------------------------------------------------------------------------- frame LN + GELU
@pytest.mark.parametrize("case", G.FRAMELN, ids=G.case_id)
def test_frameln_act(K, case):
    """frame_stats_kernel, frameln_act_fwd_kernel; frameln_act_bwd_stats_kernel + frameln_act_bwd_fused_kernel over (ragged) frame
    chunks + the sum of the chunk partials"""
    Fr, P, Ch = case[:3]
    i = dev(G.frameln_inputs(case))
    w, b = i["w"].detach().reshape(-1).requires_grad_(), i["b"].detach().reshape(-1).requires_grad_()
    out = K.frameln_act(i["h"], w, b, i["res"], Fr)
    g = grads(out, i["cot"], dict(dh=i["h"], dw=w, db=b, dres=i["res"]))
    g["dw"], g["db"] = g["dw"].reshape(P, Ch), g["db"].reshape(P, Ch)
    g["out"] = out
    G.close_all("frameln", case, g)


def test_frameln_act_backward_refuses_a_frame_that_is_no_multiple_of_16(K):
    Fr, P, Ch = G.FRAMELN_BAD_PER_FRAME
    h = G.O.seeded_randn((Fr, P, Ch), 1990).to(DEV).requires_grad_()
    w, b = torch.ones(P * Ch, device=DEV, requires_grad=True), torch.zeros(P * Ch, device=DEV, requires_grad=True)
    out = K.frameln_act(h, w, b, None, Fr)
    ref = G.O.gelu(G.O.frame_ln(h.detach().double().cpu(), 1.0, 0.0))
    G.close("frameln[per_frame 12]", "out", out, ref)
    with pytest.raises(RuntimeError, match=r"multiple of 16"):
        out.sum().backward()


def test_frameln_act_drop_path(K):
    """per-sample drop-path (p = 0.5, 2 frames per sample, 16 samples): a dropped sample leaves out - res EXACTLY 0 and no input
    gradient, a kept one the branch / (1 - p); the parameter gradients are those of the kept samples.  The float64 reference is
    given the keep decisions read off the output, so all of it is one comparison; both kinds of sample must occur."""
    d = G.FRAMELN_DROPPATH
    Fr, fps, p = d["frames"], d["frames_per_sample"], d["p_dp"]
    case, seed = G.droppath_case(), G.SEED["droppath"]
    i = dev(G.frameln_inputs(case, seed=seed))
    w, b = i["w"].detach().reshape(-1).requires_grad_(), i["b"].detach().reshape(-1).requires_grad_()
    out = K.frameln_act(i["h"], w, b, i["res"], Fr, 0.0, p, fps)
    g = grads(out, i["cot"], dict(dh=i["h"], dw=w, db=b, dres=i["res"]))
    branch = (out.detach() - i["res"].detach()).reshape(Fr // fps, -1)
    dropped = (branch == 0).all(1)
    assert bool(dropped.any()) and not bool(dropped.all()), f"{int(dropped.sum())} of {Fr // fps} samples dropped: need both kinds"
    assert bool((branch[~dropped] != 0).any(1).all())
    dh = g["dh"].reshape(Fr // fps, -1)
    assert bool((dh[dropped] == 0).all()) and bool((dh[~dropped] != 0).any(1).all())
    scale = ((~dropped).double() / (1.0 - p)).repeat_interleave(fps).cpu()
    ref = G.frameln_reference(case, torch.float64, seed=seed, frame_scale=scale)
    f32 = G.frameln_reference(case, torch.float32, seed=seed, frame_scale=scale)
    g["dw"], g["db"] = g["dw"].reshape(d["P"], d["Ch"]), g["db"].reshape(d["P"], d["Ch"])
    g["out"] = out
    for k in ref:
        G.close("frameln[droppath]", k, g[k], ref[k], G.BOUND, f32[k])


# ------------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("case", G.LAYERNORM, ids=G.case_id)
def test_layernorm(K, case):
    """ln_fwd_kernel / ln_bwd_kernel <1>, <3>, <4>: one row (three idle waves), three rows, 1001 rows (251 blocks, the last with one row)"""
    i = dev(G.layernorm_inputs(case))
    y = K.layernorm(i["x"], i["w"], i["b"], 1e-5, bool(case[2]))
    g = grads(y, i["cot"], dict(dx=i["x"], dw=i["w"], db=i["b"]))
    g["y"] = y
    G.close_all("layernorm", case, g)


def test_layernorm_res(K):
    """(x, LN(x)) with both outputs in the loss: the residual branch's gradient is folded into the backward kernel"""
    i = dev(G.layernorm_inputs(G.layernorm_res_case(), seed=G.SEED["layernorm_res"]))
    xr, y = K.layernorm_res(i["x"], i["w"], i["b"])
    gx, gw, gb = torch.autograd.grad((y * i["cot"]).sum() + (xr * i["cot_x"]).sum(), [i["x"], i["w"], i["b"]])
    got = dict(x_out=xr, y=y, dx=gx, dw=gw, db=gb)
    ref, f32 = G.layernorm_res_reference(torch.float64), G.layernorm_res_reference(torch.float32)
    for k in ref:
        G.close("layernorm_res[5x768]", k, got[k], ref[k], G.BOUND, f32[k])


# ------------------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("case", G.ATTN_TEMPORAL, ids=G.case_id)
def test_attn_temporal_and_cross(K, case):
    """P != 64 pixel strips; every (nq, nk) of the MFMA dispatch and the generic 33 .. 128 kernels; 1 and 3 heads: a last block of
    four waves with fewer than four (group, head) pairs"""
    from npvp_amd.ops import AttnCfg
    N, P, Tq, Tk, mask, heads = case
    i = dev(G.attn_temporal_inputs(case))
    y = K.attn(i["q"], i["k"], i["v"], AttnCfg(1, N, P, G.ATTN_TEMPORAL_W[P], 0, Tq, Tk, heads, mask, 0.0))
    g = grads(y, i["cot"], dict(dq=i["q"], dk=i["k"], dv=i["v"]))
    g["y"] = y
    G.close_all("attn_temporal", case, g)


@pytest.mark.parametrize("case", G.ATTN_SPATIAL, ids=G.case_id)
def test_attn_spatial_rectangular(K, case):
    """windows that tile a grid with H != W (the window's rows lie W, not H, apart), packed q|k"""
    from npvp_amd.ops import AttnCfg
    Fr, H, W, ws = case
    cfg = AttnCfg.spatial(Fr, H, W, ws, G.SPATIAL_HEADS, 0.0)
    assert cfg.tiles and (cfg.P, cfg.W) == (H * W, W)
    i = dev(G.attn_spatial_inputs(case))
    y = K.attn_packed(i["qk"], i["v"], cfg)
    g = grads(y, i["cot"], dict(dqk=i["qk"], dv=i["v"]))
    g["y"] = y
    G.close_all("attn_spatial", case, g)
