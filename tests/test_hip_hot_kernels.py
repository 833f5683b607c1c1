"""GPU: the kernels of the shipped 8 x 8 x 512 point, one entry point at a time against float64 at 1e-5 on the whole tensor and on
the worst row (a frame mean: 1e-5 sigma) - MlpDWBN's fused middle and its neighbours through the C ABI (npvp_amd._lib.lib()), the
norms and the attention cores through the npvp_amd.ops call sites the models use.  Cases, references, bound and comparison:
tests/hot_kernel_cases.py; tests/test_hot_kernel_cases_host.py shows that those cases reject a wrong kernel.  One recorded run:
profiles/hot_kernels_errors.txt (NPVP_ERR_LOG=<file> appends `case output error worst-row-error fp32-cpu-error`).

The fused middle's BACKWARD (families mid_bwd and mid_n2 of the cases file) has no test here yet: see DESIGN.md.

Through the C ABI every operand is a view into a NaN-padded allocation and every output, buffer updated in place and workspace a
view into one filled with the bit pattern 0x7FC0BEEF, which must be intact around the view afterwards (helper_kernel_cases.Flat)."""
import pytest
import torch

import hot_kernel_cases as HK
from helper_kernel_cases import DEV, PATTERN, Flat, out_flat

pytestmark = pytest.mark.gpu

EPS = 1e-5


@pytest.fixture(scope="module")
def K():
    import npvp_amd  # noqa: F401
    from npvp_amd import ops
    assert torch.cuda.is_available()
    ops.set_gemm_precision("f16x3")
    ops.rng.manual_seed(1234, torch.device(DEV))
    yield ops


@pytest.fixture(scope="module")
def L(K):
    from npvp_amd._lib import lib
    return lib()


def stream():
    from npvp_amd import ops
    return ops._stream()


def ok(L, rc, what):
    torch.cuda.synchronize()
    assert rc == 0, f"{what}: rc {rc}: {L.npvp_last_error()}"


def refused(L, rc, what, outs):
    """an argument error: non-zero with a message, before any launch - the pattern-filled outputs are as they were"""
    torch.cuda.synchronize()
    msg = L.npvp_last_error()
    assert rc != 0 and msg, f"{what}: rc {rc}, message {msg!r}"
    for o in outs:
        assert bool((o.base.view(torch.int32) == PATTERN).all()), f"{what}: an output was written although the call was refused"


AMAX_SLOT_FLOATS = 32 * 16          # an amax slot is 2 KB: 32 words, 64 bytes apart (include/npvp_hip.h); a block raises word blockIdx.x % 32


def slot():
    """a zeroed amax slot of its full 2 KB, the pattern around it"""
    return out_flat(AMAX_SLOT_FLOATS, torch.zeros(AMAX_SLOT_FLOATS))


def intact(*bufs):
    for b in bufs:
        assert b.intact(), "written outside an output's extent"


def taps(i):
    """the Conv2d weight [Ch, 3, 3] as the kernels take it: tap-major [9, Ch]"""
    w = i["w"].detach()
    return w.reshape(w.shape[0], 9).t().contiguous()


def mid_operands(i):
    return {k: Flat(i[k].detach()) for k in ("h1", "w1n", "b1n", "bias", "w2n", "b2n")} | dict(wt=Flat(taps(i)))


def ws_flat(nbytes):
    return out_flat(max(int(nbytes) // 4, 1))


# ------------------------------------------------------------------------------------------------------------------- middle, forward
@pytest.mark.parametrize("case", HK.MID_FWD, ids=HK.case_id)
def test_mid_fwd(L, case):
    """npvp_mlpdw_mid_fwd (mean1 / rstd1 supplied: float64, rounded once): h2 and norm2's statistics"""
    Fr, Ch, kind = case
    i = HK.mid_inputs("mid_fwd", case)
    d = mid_operands(i)
    m1, r1 = (Flat(t) for t in HK.mid_stats_in(i))
    n = Fr * 64 * Ch
    h2, mean2, rstd2, ws = out_flat(n), out_flat(Fr), out_flat(Fr), ws_flat(Fr * (Ch // 512) * 8)
    ok(L, L.npvp_mlpdw_mid_fwd(d["h1"].ptr, m1.ptr, r1.ptr, d["w1n"].ptr, d["b1n"].ptr, d["wt"].ptr, d["bias"].ptr, h2.ptr, mean2.ptr,
                               rstd2.ptr, Fr, 8, 8, Ch, EPS, ws.ptr, ws.n * 4, stream()), "npvp_mlpdw_mid_fwd")
    intact(h2, mean2, rstd2, ws)
    HK.close_all("mid_fwd", case, dict(h2=h2.cpu(Fr, 64, Ch), mean2=mean2.cpu(), rstd2=rstd2.cpu()))


@pytest.mark.parametrize("case", HK.MID_FWD, ids=HK.case_id)
def test_mid_fwd_parts_and_the_norm_behind_it(L, case):
    """npvp_mlpdw_mid_fwd_parts: norm1's statistics merged from the fc1 GEMM's row-statistics layout (built on the CPU), each partial
    of part2 against the float64 (mean, M2) of its 32 768 values, their Chan merge against the frame's statistics; then
    npvp_frameln_act_fwd_parts on that part2, without and with a residual"""
    Fr, Ch, kind = case
    i = HK.mid_inputs("mid_fwd", case)
    d = mid_operands(i)
    J1, J2, n = Ch // 64, Ch // 512, Fr * 64 * Ch
    part1 = Flat(HK.mid_part1(i))
    mean1, rstd1, h2, part2 = out_flat(Fr), out_flat(Fr), out_flat(n), out_flat(Fr * J2 * 2)
    ok(L, L.npvp_mlpdw_mid_fwd_parts(d["h1"].ptr, part1.ptr, J1, 4096.0, mean1.ptr, rstd1.ptr, d["w1n"].ptr, d["b1n"].ptr, d["wt"].ptr,
                                     d["bias"].ptr, h2.ptr, part2.ptr, Fr, 8, 8, Ch, EPS, stream()), "npvp_mlpdw_mid_fwd_parts")
    intact(mean1, rstd1, h2, part2)
    p2 = part2.cpu(Fr, J2, 2)
    mm, mr = HK.chan_merge(p2, 32768.0)
    got = dict(h2=h2.cpu(Fr, 64, Ch), mean1=mean1.cpu(), rstd1=rstd1.cpu(), part2_mean=p2[:, :, 0], part2_m2=p2[:, :, 1],
               merged_mean2=mm, merged_rstd2=mr)
    # the consumer of part2: its own h2 in, so its input is the kernel's, not the reference's
    h2_in, p2_in, res = Flat(h2.v), Flat(part2.v), Flat(i["res"])
    for name, r in (("out", None), ("out_res", res)):
        mean2, rstd2, out, am = out_flat(Fr), out_flat(Fr), out_flat(n), slot()
        ok(L, L.npvp_frameln_act_fwd_parts(h2_in.ptr, p2_in.ptr, J2, 32768.0, EPS, mean2.ptr, rstd2.ptr, d["w2n"].ptr, d["b2n"].ptr,
                                           r.ptr if r else None, out.ptr, Fr, 64 * Ch, 0.0, 0, 0.0, 0, 1, None, am.ptr, stream()),
           "npvp_frameln_act_fwd_parts")
        intact(mean2, rstd2, out, am)
        got[name] = out.cpu(Fr, 64, Ch)
        got.update(mean2=mean2.cpu(), rstd2=rstd2.cpu())
    HK.close_all("mid_fwd", case, got)


# ------------------------------------------------------------------------------------------------------------------- depthwise 8 x 8
def dw_operands(i):
    return Flat(i["a"].detach()), Flat(taps(i)), Flat(i["b"].detach()), Flat(i["cot"])


@pytest.mark.parametrize("case", HK.DW_FWD, ids=HK.case_id)
def test_dwconv_window_forward_and_input_gradient(L, case):
    """dwconv3x3_win_kernel<8, 8, false>: flip 0 on the input, flip 1 (no bias) on the cotangent"""
    Fr, Ch, kind = case
    a, wt, b, cot = dw_operands(HK.dw_inputs("dw_fwd", case))
    y, da = out_flat(Fr * 64 * Ch), out_flat(Fr * 64 * Ch)
    ok(L, L.npvp_dwconv3x3(a.ptr, wt.ptr, b.ptr, y.ptr, Fr, 8, 8, Ch, 0, stream()), "npvp_dwconv3x3")
    ok(L, L.npvp_dwconv3x3(cot.ptr, wt.ptr, None, da.ptr, Fr, 8, 8, Ch, 1, stream()), "npvp_dwconv3x3 (flip)")
    intact(y, da)
    HK.close_all("dw_fwd", case, dict(y=y.cpu(Fr, 64, Ch), da=da.cpu(Fr, 64, Ch)))


@pytest.mark.parametrize("case", HK.DW_STATS, ids=HK.case_id)
def test_dwconv_window_with_statistics(L, case):
    """dwconv3x3_win_kernel<8, 8, true> + frame_stats_finalize_kernel: sums about a thread's first output, Chan-merged"""
    Fr, Ch, kind = case
    a, wt, b, _ = dw_operands(HK.dw_inputs("dw_stats", case))
    y, mean, rstd, ws = out_flat(Fr * 64 * Ch), out_flat(Fr), out_flat(Fr), ws_flat(Fr * (Ch // 1024) * 8)
    ok(L, L.npvp_dwconv3x3_stats(a.ptr, wt.ptr, b.ptr, y.ptr, mean.ptr, rstd.ptr, Fr, 8, 8, Ch, EPS, ws.ptr, ws.n * 4, stream()),
       "npvp_dwconv3x3_stats")
    intact(y, mean, rstd, ws)
    HK.close_all("dw_stats", case, dict(y=y.cpu(Fr, 64, Ch), mean=mean.cpu(), rstd=rstd.cpu()))


@pytest.mark.parametrize("case", HK.DW_WGRAD, ids=HK.case_id)
def test_dwconv_window_weight_gradient(L, case):
    """dwconv3x3_wgrad_win_kernel<8, 8> over frame chunks + the sum of the chunk partials"""
    Fr, Ch, kind = case
    a, _, _, cot = dw_operands(HK.dw_inputs("dw_wgrad", case))
    dwt, ws = out_flat(10 * Ch), ws_flat(L.npvp_dwconv3x3_wgrad_workspace_bytes(Fr, Ch))
    ok(L, L.npvp_dwconv3x3_wgrad(a.ptr, cot.ptr, dwt.ptr, Fr, 8, 8, Ch, ws.ptr, ws.n * 4, stream()), "npvp_dwconv3x3_wgrad")
    intact(dwt, ws)
    HK.close_all("dw_wgrad", case, dict(dwt_db=dwt.cpu(10, Ch)))


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_the_middle_refuses_what_it_cannot_run(L):
    """a grid that is not 8 x 8, Ch % 512 != 0, a short workspace: non-zero, a message, nothing written"""
    Fr, Ch = 1, 512
    i = HK.mid_inputs("mid_fwd", HK.MID_FWD[0])
    d = mid_operands(i)
    st = [Flat(t) for t in HK.mid_stats_in(i)]
    cot = Flat(i["cot"])
    n = Fr * 64 * Ch
    for what, (H, W, ch, short) in dict(grid=(4, 16, Ch, 0), channels=(8, 8, 768, 0), workspace=(8, 8, Ch, 4)).items():
        h2, mean2, rstd2, ws = out_flat(n), out_flat(Fr), out_flat(Fr), ws_flat(Fr * 2 * 8)
        rc = L.npvp_mlpdw_mid_fwd(d["h1"].ptr, st[0].ptr, st[1].ptr, d["w1n"].ptr, d["b1n"].ptr, d["wt"].ptr, d["bias"].ptr, h2.ptr,
                                  mean2.ptr, rstd2.ptr, Fr, H, W, ch, EPS, ws.ptr, 4 if short else ws.n * 4, stream())
        refused(L, rc, f"npvp_mlpdw_mid_fwd ({what})", (h2, mean2, rstd2, ws))
        if not short:
            part1, mean1, rstd1, part2 = Flat(HK.mid_part1(i)), out_flat(Fr), out_flat(Fr), out_flat(Fr * 2 * 2)
            rc = L.npvp_mlpdw_mid_fwd_parts(d["h1"].ptr, part1.ptr, Ch // 64, 4096.0, mean1.ptr, rstd1.ptr, d["w1n"].ptr, d["b1n"].ptr,
                                            d["wt"].ptr, d["bias"].ptr, h2.ptr, part2.ptr, Fr, H, W, ch, EPS, stream())
            refused(L, rc, f"npvp_mlpdw_mid_fwd_parts ({what})", (h2, mean1, rstd1, part2))
        da1, dwt, psum = out_flat(n), out_flat(10 * 768), out_flat(Fr * 3 * 2)
        wsb = ws_flat(L.npvp_mlpdw_mid_bwd_workspace_bytes(Fr, 768))
        rc = L.npvp_mlpdw_mid_bwd(cot.ptr, d["h1"].ptr, st[0].ptr, st[1].ptr, d["w1n"].ptr, d["b1n"].ptr, d["wt"].ptr, da1.ptr,
                                  dwt.ptr, psum.ptr, Fr, H, W, ch, 0, wsb.ptr, 4 if short else wsb.n * 4, stream())
        refused(L, rc, f"npvp_mlpdw_mid_bwd ({what})", (da1, dwt, psum, wsb))
    y, mean, rstd, ws = out_flat(n), out_flat(Fr), out_flat(Fr), ws_flat(64)
    rc = L.npvp_dwconv3x3_stats(d["h1"].ptr, d["wt"].ptr, d["bias"].ptr, y.ptr, mean.ptr, rstd.ptr, Fr, 8, 8, Ch, EPS, ws.ptr, ws.n * 4, stream())
    refused(L, rc, "npvp_dwconv3x3_stats (Ch % 1024)", (y, mean, rstd, ws))


# ------------------------------------------------------------------------------------------------------------------- norms
def dev(i):
    return {k: (None if t is None else t.detach().to(DEV).requires_grad_(t.requires_grad)) for k, t in i.items()}


def grads(y, cot, leaves):
    names = [k for k, v in leaves.items() if v is not None]
    return dict(zip(names, torch.autograd.grad((y * cot).sum(), [leaves[k] for k in names])))


@pytest.mark.parametrize("case", HK.LAYERNORM, ids=HK.case_id)
def test_layernorm_512(K, case):
    """ln_fwd_kernel<2> / ln_bwd_kernel<2>: the instantiation every shipped config runs"""
    i = dev(HK.layernorm_inputs(case))
    y = K.layernorm(i["x"], i["w"], i["b"], 1e-5, bool(case[2]))
    g = grads(y, i["cot"], dict(dx=i["x"], dw=i["w"], db=i["b"]))
    g["y"] = y
    HK.close_all("layernorm", case, g)


def test_layernorm_res_512(K):
    i = dev(HK.layernorm_inputs(HK.layernorm_res_case(), seed=HK.SEED["layernorm_res"]))
    xr, y = K.layernorm_res(i["x"], i["w"], i["b"])
    gx, gw, gb = torch.autograd.grad((y * i["cot"]).sum() + (xr * i["cot_x"]).sum(), [i["x"], i["w"], i["b"]])
    HK.close_dict("layernorm_res[5x512]", dict(x_out=xr, y=y, dx=gx, dw=gw, db=gb), HK.layernorm_res_reference(torch.float64),
                  HK.layernorm_res_reference(torch.float32))


@pytest.mark.parametrize("case", HK.LAYERNORM_NCHW, ids=HK.case_id)
def test_layernorm_nchw(K, case):
    """ln_nchw_fwd_kernel<256 | 512>, relu 0 and 1; backward: npvp_transpose + ln_bwd_kernel"""
    Fr, C, relu, kind = case
    i = dev(HK.layernorm_nchw_inputs(case))
    y = K.layernorm_nchw(i["x"], i["w"], i["b"], 1e-5, bool(relu), 1, Fr, 8, 8)
    g = grads(y, i["cot"], dict(dx=i["x"], dw=i["w"], db=i["b"]))
    g["y"] = y
    HK.close_all("layernorm_nchw", case, g)


@pytest.mark.parametrize("case", HK.POSFUSE, ids=HK.case_id)
def test_posfuse_at_64_pixels(K, L, case):
    """posfuse_fwd_frame_kernel<8> (the frame in a block's registers); backward: the fused apply (N = 3) or the apply + two batch
    reductions (N = 18, T = 2)"""
    N, T = case[0], case[1]
    assert L.npvp_posfuse_bwd_fused(N, T, 64 * 512) == (1 if N <= 16 else 0)
    i = dev(HK.posfuse_inputs("posfuse", case))
    y = K.posfuse(i["x"], i["add"], i["beta"], i["gamma"], N, T)
    g = grads(y, i["cot"], dict(dx=i["x"], dadd=i["add"], dbeta=i["beta"], dgamma=i["gamma"]))
    g["y"] = y
    HK.close_all("posfuse", case, g)


@pytest.mark.parametrize("case", HK.LN_POSFUSE, ids=HK.case_id)
def test_ln_posfuse_against_float64(K, case):
    """npvp_ln_posfuse_fwd against float64 LayerNorm -> posfuse (not against the two-kernel route)"""
    N, T = case[0], case[1]
    assert K.LN_POSFUSE_ONE_KERNEL
    i = dev(HK.posfuse_inputs("ln_posfuse", case))
    with torch.no_grad():
        y1, lst, fused, pst = K._raw_ln_posfuse_fwd(i["x"].reshape(-1, 512), i["lw"], i["lb"], 1e-5, i["add"], i["beta"], i["gamma"], N, T)
    HK.close_all("ln_posfuse", case, dict(y1=y1.reshape(N * T, 64, 512), ln_rstd=lst[1], fused=fused.reshape(N * T, 64, 512),
                                          mean=pst[0], rstd=pst[1]))


@pytest.mark.parametrize("mode", ["bf16x6", "f16x3"])
@pytest.mark.parametrize("case", HK.LINEAR_STATS, ids=HK.case_id)
def test_linear_frame_statistics_with_a_large_bias(K, case, mode):
    """linear(frame_stats=True) with a + 30 bias: the epilogue's statistics against float64 statistics of the kernel's OWN output"""
    R, N, Kd = case
    K.set_gemm_precision(mode)
    try:
        assert K.linear_frame_stats_supported(R, N)
        i = HK.linear_stats_inputs(case)
        with torch.no_grad():
            y, mean, rstd = K.linear(i["x"].to(DEV), i["w"].to(DEV), i["b"].to(DEV), frame_stats=True)
    finally:
        K.set_gemm_precision("f16x3")
    mu, rs = HK.frame_stats64(y.double().cpu().reshape(R // 64, -1))
    HK.close_dict(f"linear_stats[{HK.case_id(case)}|{mode}]", dict(mean=mean, rstd=rstd), dict(mean=mu, rstd=rs))


# ------------------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("case", HK.ATTN_T, ids=HK.case_id)
def test_attn_temporal_with_wide_scores(K, case):
    """P = 64: the MFMA backward (T = 10), the staged <2, 2> (18) and <2, 1> (28 x 2), the generic kernels (40) and the streaming
    ones (129), scores of sigma 2 with a planted 100 - on a masked key too, where it must not win"""
    from npvp_amd.ops import AttnCfg
    N, Tq, Tk, mask, plant = case
    i = dev(HK.attn_t_inputs(case))
    y = K.attn(i["q"], i["k"], i["v"], AttnCfg(1, N, 64, 8, 0, Tq, Tk, HK.HEADS, mask, 0.0))
    g = grads(y, i["cot"], dict(dq=i["q"], dk=i["k"], dv=i["v"]))
    g["y"] = y
    HK.close_all("attn_t", case, g)


@pytest.mark.parametrize("case", HK.ATTN_S, ids=HK.case_id)
def test_attn_spatial_with_wide_scores(K, case):
    from npvp_amd.ops import AttnCfg
    Fr, ws, plant = case
    i = dev(HK.attn_s_inputs(case))
    y = K.attn_packed(i["qk"], i["v"], AttnCfg.spatial(Fr, 8, 8, ws, HK.HEADS, 0.0))
    g = grads(y, i["cot"], dict(dqk=i["qk"], dv=i["v"]))
    g["y"] = y
    HK.close_all("attn_s", case, g)



@pytest.mark.parametrize("case", HK.ATTN_NL, ids=HK.case_id)
def test_attn_nonlocal_with_a_planted_winner(K, case):
    """npvp_nonlocal_attn_grid_* at (8, 32) on 4 x 4 and on 18 x 16 (two key tiles, the winner in either), npvp_nonlocal_attn_* at
    (64, 256) on 8 x 8: unscaled scores, one of 100"""
    route, A, Fr, H, W, plant = case
    i = dev(HK.attn_nl_inputs(case))
    y = (K.nonlocal_attn if route == "config" else K.nonlocal_attn_grid)(i["q"], i["k"], i["v"], H, W)
    g = grads(y, i["cot"], dict(dq=i["q"], dk=i["k"], dv=i["v"]))
    g["y"] = y
    HK.close_all("attn_nl", case, g)
