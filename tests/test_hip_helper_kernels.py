"""GPU: the small HBM-bound kernels of csrc/elementwise.hip, csrc/ae.hip, csrc/metrics.hip and csrc/data.hip, one by one through the
C ABI (npvp_amd._lib.lib(), on the current stream), against the float64 references of tests/helper_kernel_cases.py at the bars set
there (1e-5 on tensors and on the worst element, 1e-6 on the scalar sums, equality where the arithmetic is one fp32 operation).
tests/test_helper_kernel_cases_host.py shows that those cases reject a wrong kernel.  One recorded run:
profiles/helper_kernels_errors.txt (NPVP_ERR_LOG=<file> appends `case output metric error bar fp32-cpu-error`).

Every operand and every output is a view into a larger buffer of this test (Flat: at least 8 floats in front and behind; Mat: rows
of `ld` floats, the gap after each row's N columns included), so nothing ends flush with its allocation, a stray access stays inside
the test's own memory and shows as a wrong value:
  * the padding of an input is NaN - a NaN in a result is an operand read outside its extent;
  * the padding of an output, of a buffer updated in place and of a workspace holds the bit pattern 0x7FC0BEEF (so does an output
    before the launch) and must be bit-identical afterwards.
Views start 16-byte aligned except in the cases that are about misalignment."""
import os

import numpy as np
import pytest
import torch

import helper_kernel_cases as H
from helper_kernel_cases import DEV, PAD, PATTERN, Flat, out_flat  # noqa: F401  (shared with tests/test_hip_hot_kernels.py)

pytestmark = pytest.mark.gpu

LOG = os.environ.get("NPVP_ERR_LOG")


@pytest.fixture(scope="module")
def L():
    import npvp_amd  # noqa: F401
    from npvp_amd._lib import lib
    assert torch.cuda.is_available()
    return lib()


def stream():
    from npvp_amd import ops
    return ops._stream()


def ok(L, rc, what):
    torch.cuda.synchronize()
    assert rc == 0, f"{what}: rc {rc}: {L.npvp_last_error()}"


def dev_scalar(values):
    """a few floats of device memory (hyper, clip, gout), NaN around them"""
    return Flat(torch.tensor(values, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------------------- AdamW, clip
@pytest.mark.parametrize("case", H.ADAMW, ids=H.ids)
def test_adamw(L, case):
    """adamw_kernel: float4 lanes with the per-lane clip tests c0..c3, the scalar tail, clip = NULL, write_back_grad 0 and 1, a second
    sweep of the grid-stride loop, hyper re-read from device memory on every call"""
    n, rng, wb, wd, eps, calls = case
    i = H.adamw_inputs(case)
    p, g, m, v = (out_flat(n, i[k]) for k in "pgmv")
    hyper, clip = dev_scalar(list(H.ADAMW_HYPER[0])), dev_scalar([123.0, H.ADAMW_COEF])
    b, e = rng if rng else (0, 0)
    for k in range(calls):
        hyper.v.copy_(torch.tensor(H.ADAMW_HYPER[k]))                       # rewritten on the device between the calls
        ok(L, L.npvp_adamw_step(p.ptr, g.ptr, m.ptr, v.ptr, n, hyper.ptr, H.ADAMW_BETAS[0], H.ADAMW_BETAS[1], eps, wd,
                                clip.ptr if rng else None, b, e, wb, stream()), "npvp_adamw_step")
    for buf, name in zip((p, g, m, v), "pgmv"):
        assert buf.intact(), f"{name}: written outside [0, n)"
    if not wb or rng is None:
        assert H.same_bits(g.cpu(), i["g"]), "g changed although nothing was to be written back"
    else:
        outside = ~H.adamw_mask(n, rng)
        assert H.same_bits(g.cpu()[outside], i["g"][outside]), "g changed outside the clip range"
    H.close_case("adamw", case, dict(dp=p.cpu().double() - i["p"].double(), m=m.cpu(), v=v.cpu(), g=g.cpu()), LOG)


@pytest.mark.parametrize("case", H.CLIP, ids=H.ids)
def test_grad_norm_clip(L, case):
    """sumsq_partial_kernel (float4s, the tail, a second sweep) + clip_coef_kernel: out = {norm, min(1, max_norm / (norm + 1e-6))}"""
    n, kind = case
    i = H.clip_inputs(case)
    g, out, ws = Flat(i["g"]), out_flat(2), out_flat(1024)
    ok(L, L.npvp_grad_norm_clip(g.ptr, n, i["max_norm"], out.ptr, ws.ptr, 4096, stream()), "npvp_grad_norm_clip")
    assert out.intact() and ws.intact()
    got = out.cpu()
    if kind in ("below", "zero"):
        assert float(got[1]) == 1.0, f"the coefficient under max_norm is exactly 1, got {float(got[1])!r}"
    H.close_case("clip", case, dict(norm=got[0:1], coef=got[1:2]), LOG)


# ------------------------------------------------------------------------------------------------------------------- scalar losses
@pytest.mark.parametrize("case", H.L1, ids=H.ids)
def test_l1_mean_and_its_backward(L, case):
    """l1_partial_kernel + sum_finish_kernel; l1_bwd_kernel: c sign(a - b) to the bit, sign(0) = 0; two runs equal"""
    (n,) = case
    i = H.l1_inputs(case)
    a, b, gout = Flat(i["a"]), Flat(i["b"]), Flat(i["gout"])
    runs = []
    for _ in range(2):
        out, ws, da = out_flat(1), out_flat(1024), out_flat(n)
        ok(L, L.npvp_l1_mean(a.ptr, b.ptr, n, i["lam"], out.ptr, ws.ptr, 4096, stream()), "npvp_l1_mean")
        ok(L, L.npvp_l1_mean_bwd(a.ptr, b.ptr, n, gout.ptr, i["lam"], da.ptr, stream()), "npvp_l1_mean_bwd")
        assert out.intact() and ws.intact() and da.intact()
        runs.append(dict(l1=out.cpu(), da=da.cpu()))
    assert H.same_bits(runs[0]["l1"], runs[1]["l1"]) and H.same_bits(runs[0]["da"], runs[1]["da"]), "two runs differ"
    H.close_case("l1", case, runs[0], LOG)


@pytest.mark.parametrize("case", H.SUM, ids=H.ids)
def test_sum_all(L, case):
    (n,) = case
    x = Flat(H.sum_inputs(case)["x"])
    runs = []
    for _ in range(2):
        out, ws = out_flat(1), out_flat(1024)
        ok(L, L.npvp_sum_all(x.ptr, n, out.ptr, ws.ptr, 4096, stream()), "npvp_sum_all")
        assert out.intact() and ws.intact()
        runs.append(out.cpu())
    assert H.same_bits(runs[0], runs[1]), "two runs differ"
    H.close_case("sum", case, dict(sum=runs[0]), LOG)


# ------------------------------------------------------------------------------------------------------------------- layout helpers
@pytest.mark.parametrize("case", H.MID, ids=H.ids)
def test_reduce_mid_and_broadcast_mid(L, case):
    """reduce_mid_kernel (overwrite, and accumulate onto a non-zero out) and broadcast_mid_kernel, below and above the 4096 blocks"""
    A, B, Cc, acc = case
    i = H.mid_inputs(case)
    x, out = Flat(i["x"]), out_flat(A * Cc, i["out0"] if acc else None)
    ok(L, L.npvp_reduce_mid(x.ptr, out.ptr, A, B, Cc, i["scale"], acc, stream()), "npvp_reduce_mid")
    y, bc = Flat(i["y"]), out_flat(A * B * Cc)
    ok(L, L.npvp_broadcast_mid(y.ptr, bc.ptr, A, B, Cc, i["scale"], stream()), "npvp_broadcast_mid")
    assert out.intact() and bc.intact()
    H.close_case("mid", case, dict(reduce=out.cpu(A, Cc), broadcast=bc.cpu(A, B, Cc)), LOG)


@pytest.mark.parametrize("case", H.TRANSPOSE, ids=H.ids)
def test_transpose(L, case):
    b, R, C = case
    x, out = Flat(H.transpose_inputs(case)["x"]), out_flat(b * R * C)
    ok(L, L.npvp_transpose(x.ptr, out.ptr, b, R, C, stream()), "npvp_transpose")
    assert out.intact()
    H.close_case("transpose", case, dict(t=out.cpu(b, C, R)), LOG)


class Mat:
    """[rows, N] at row stride ld inside a NaN allocation: PAD floats in front, the ld - N floats after every row (the last one
    included) and PAD floats behind are NaN"""

    def __init__(self, full, N):
        rows, ld = full.shape
        self.base = torch.full((2 * PAD + rows * ld,), float("nan"), dtype=torch.float32, device=DEV)
        self.base[PAD:PAD + rows * ld].view(rows, ld)[:, :N] = full[:, :N].to(DEV)
        self.ptr = self.base[PAD:].data_ptr()


@pytest.mark.parametrize("case", H.COLSUM, ids=H.ids)
def test_colsum(L, case):
    """colsum_partial_kernel over exact, ragged and fewer-than-reserved row chunks at ld >= N, then the sum of the partial rows -
    with a workspace exactly as large as the query says"""
    rows, N, ld, acc = case
    i = H.colsum_inputs(case)
    x, out = Mat(i["full"], N), out_flat(N, i["out0"] if acc else None)
    nbytes = L.npvp_colsum_workspace_bytes(rows, N)
    assert nbytes == 4 * N * H.colsum_chunks(rows)[0]
    ws = out_flat(nbytes // 4)
    ok(L, L.npvp_colsum(x.ptr, rows, N, ld, out.ptr, acc, ws.ptr, nbytes, stream()), "npvp_colsum")
    assert out.intact() and ws.intact()
    H.close_case("colsum", case, dict(colsum=out.cpu()), LOG)


@pytest.mark.parametrize("case", H.DWTB, ids=H.ids)
def test_dwtb_build_and_accumulate(L, case):
    C, hb = case
    i = H.dwtb_inputs(case)
    w, b, wtb = Flat(i["w"]), Flat(i["b"]) if hb else None, out_flat(10 * C)
    ok(L, L.npvp_dwtb_build(w.ptr, b.ptr if hb else None, wtb.ptr, C, stream()), "npvp_dwtb_build")
    dwtb, gw, gb = Flat(i["dwtb"]), out_flat(9 * C, i["gw0"]), out_flat(C, i["gb0"])
    ok(L, L.npvp_dwtb_accumulate(dwtb.ptr, gw.ptr, gb.ptr, C, stream()), "npvp_dwtb_accumulate")
    assert wtb.intact() and gw.intact() and gb.intact()
    H.close_case("dwtb", case, dict(wtb=wtb.cpu(10, C), gw=gw.cpu(C, 9), gb=gb.cpu()), LOG)


def run_drop(L, x, rows, ncols, p, mode, g1, g2):
    """-> (out [rows, ncols] on the CPU, the amax slot's value); the canaries are checked here"""
    xin, out = Flat(x[:rows]), out_flat(rows * ncols)
    seed = torch.tensor([-1, -1, H.DROP_SEED, -1, -1], dtype=torch.int64, device=DEV)[2:3]
    slot = out_flat(512, torch.zeros(512))                                  # 32 words, 64 bytes apart (include/npvp_hip.h)
    ok(L, L.npvp_drop_apply(xin.ptr, out.ptr, rows, ncols, p, mode, g1, g2, seed.data_ptr(), H.DROP_SALT, slot.ptr, stream()), "npvp_drop_apply")
    assert out.intact() and slot.intact()
    return out.cpu(rows, ncols), float(slot.cpu().max())


@pytest.mark.parametrize("case", H.DROP, ids=H.ids)
def test_drop_apply(L, case):
    """drop_apply_kernel: every output is 0 or x * (1 / (1 - p)) to the bit; the decision depends on (row, column) - or on the row
    group (row / g1) % g2 - and not on the launch; the kept share; the amax slot"""
    rows, ncols, p, mode, g1, g2 = case
    x = H.drop_inputs(case)["x"]
    got, amax = run_drop(L, x, rows, ncols, p, mode, g1, g2)
    assert not torch.isnan(got).any()
    kept = got != 0
    want = torch.from_numpy(x.numpy() * H.drop_inv_keep(p))
    assert H.same_bits(got[kept], want[kept]), "a kept value is not x * (1 / (1 - p))"
    assert amax == float(got.abs().max())
    if rows > 3:
        first, _ = run_drop(L, x, 3, ncols, p, mode, g1, g2)
        assert H.same_bits(first, got[:3]), "the first 3 rows depend on the launch"
    if mode == 0:
        draws, share = rows * ncols, float(kept.double().mean())
    else:
        assert bool((kept == kept[:, :1]).all()), "a row-group mask varies along a row"
        group = (torch.arange(rows) // g1) % g2
        per_group = torch.zeros(g2, dtype=torch.bool)
        per_group[group] = kept[:, 0]
        assert torch.equal(per_group[group], kept[:, 0]), "rows of one group disagree"
        draws = int(group.max()) + 1
        share = float(per_group[:draws].double().mean())
    assert abs(share - (1 - p)) <= 4 * (p * (1 - p) / draws) ** 0.5, (share, draws)


# ------------------------------------------------------------------------------------------------------------------- epilogues
@pytest.mark.parametrize("case", H.BIAS_ACT, ids=H.ids)
def test_bias_act(L, case):
    """bias_act_kernel<true> and <false> (by shape and by alignment), both layouts, every activation, with and without a residual"""
    lay, outer, inner, C, act, r, mis = case
    i = H.bias_act_inputs(case)
    x, bias, res = Flat(i["x"], shift=mis), Flat(i["bias"]), Flat(i["res"]) if r else None
    out = out_flat(outer * inner)
    ok(L, L.npvp_bias_act(x.ptr, bias.ptr, res.ptr if r else None, out.ptr, outer, inner, C, lay, act, stream()), "npvp_bias_act")
    assert out.intact()
    H.close_case("bias_act", case, dict(y=out.cpu(outer, inner)), LOG)


@pytest.mark.parametrize("case", H.ACT_BWD, ids=H.ids)
def test_act_bwd(L, case):
    n, act = case
    i = H.act_bwd_inputs(case)
    g, y, dx = Flat(i["g"]), Flat(i["y"]), out_flat(n)
    ok(L, L.npvp_act_bwd(g.ptr, y.ptr, dx.ptr, n, act, stream()), "npvp_act_bwd")
    assert dx.intact()
    H.close_case("act_bwd", case, dict(dx=dx.cpu()), LOG)


# ------------------------------------------------------------------------------------------------------------------- metrics, data
@pytest.mark.parametrize("case", H.SQDIFF, ids=H.ids)
def test_sqdiff_per_image(L, case):
    """sqdiff_partial_kernel: blocks on the float4 path and on the scalar path within one launch, the 256-chunk cap"""
    N, per, rng, sk, mis = case
    i = H.sqdiff_inputs(case)
    x, y, out = Flat(i["x"], shift=mis), Flat(i["y"]), out_flat(N)
    nbytes = L.npvp_sqdiff_workspace_bytes(N, per)
    assert nbytes == 4 * N * H.sqdiff_chunks(per)[0]
    ws = out_flat(nbytes // 4)
    ok(L, L.npvp_sqdiff_per_image(x.ptr, y.ptr, N, per, i["data_range"], i["scale"], out.ptr, ws.ptr, nbytes, stream()), "npvp_sqdiff_per_image")
    assert out.intact() and ws.intact()
    H.close_case("sqdiff", case, dict(sq=out.cpu()), LOG)


@pytest.mark.parametrize("case", H.SSIM, ids=H.ids)
def test_ssim_per_image(L, case):
    """ssim_tile_kernel<3>, <5>, <7>, <11> on one pixel, on an image narrower than the window, on several ragged tiles"""
    ws_, N, C, Hh, W = case
    i = H.ssim_inputs(case)
    a, b, out = Flat(i["a"]), Flat(i["b"]), out_flat(N)
    taps = np.ascontiguousarray(i["taps"].numpy(), dtype=np.float32)
    nbytes = L.npvp_ssim_workspace_bytes(N, C, Hh, W)
    ws = out_flat(nbytes // 4)
    ok(L, L.npvp_ssim_per_image(a.ptr, b.ptr, N, C, Hh, W, taps.ctypes.data, ws_, out.ptr, ws.ptr, nbytes, stream()), "npvp_ssim_per_image")
    assert out.intact() and ws.intact()
    H.close_case("ssim", case, dict(ssim=out.cpu()), LOG)


@pytest.mark.parametrize("case", H.U8, ids=H.ids)
def test_u8_to_normalised_inside_a_larger_buffer(L, case):
    """u8hwc_to_f32chw_kernel with its output inside a larger buffer (tests/test_data.py holds the values; its output is flush)"""
    C, Hh, W = case
    i = H.u8_inputs(case)
    n = i["src"].size
    src = torch.full((n + 64,), 255, dtype=torch.uint8, device=DEV)
    src[32:32 + n] = torch.from_numpy(i["src"].reshape(-1)).to(DEV)
    out = out_flat(n)
    ok(L, L.npvp_u8hwc_to_f32chw(src[32:].data_ptr(), out.ptr, H.U8_FRAMES, Hh, W, C, i["mean"].ctypes.data, i["std"].ctypes.data, stream()),
       "npvp_u8hwc_to_f32chw")
    assert out.intact()
    got = out.cpu(H.U8_FRAMES, C, Hh, W).double().numpy()
    assert not np.isnan(got).any() and np.max(np.abs(got - H.u8_reference(case))) <= 2e-6


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_that_test_abi_does_not_cover(L):
    """NPVP_CHECK_ARG conditions: each returns a negative status before any launch and names its entry point.  Pointers are NULL
    or addresses inside real buffers."""
    buf = torch.zeros(65536 + 64, dtype=torch.float32, device=DEV)
    P, off = buf.data_ptr(), buf.data_ptr() + 4                         # 16-byte aligned; 4 bytes off
    seed = torch.zeros(1, dtype=torch.int64, device=DEV).data_ptr()
    taps = np.ones(11, dtype=np.float32)
    mean = np.ones(4, dtype=np.float32)
    big = 1 << 20
    calls = [
        ("drop_apply", L.npvp_drop_apply, (P, P, 4, 6, 0.5, 0, 1, 1, seed, 1, None, None)),                      # ncols % 4
        ("drop_apply", L.npvp_drop_apply, (None, P, 4, 8, 0.5, 0, 1, 1, seed, 1, None, None)),
        ("drop_apply", L.npvp_drop_apply, (P, None, 4, 8, 0.5, 0, 1, 1, seed, 1, None, None)),
        ("transpose", L.npvp_transpose, (P, P, 65536, 1, 1, None)),
        ("transpose", L.npvp_transpose, (None, P, 1, 4, 4, None)),
        ("transpose", L.npvp_transpose, (P, None, 1, 4, 4, None)),
        ("reduce_mid", L.npvp_reduce_mid, (P, P, 2, 2, 6, 1.0, 0, None)),                                        # Cc % 4
        ("reduce_mid", L.npvp_reduce_mid, (None, P, 2, 2, 8, 1.0, 0, None)),
        ("reduce_mid", L.npvp_reduce_mid, (P, None, 2, 2, 8, 1.0, 0, None)),
        ("broadcast_mid", L.npvp_broadcast_mid, (P, P, 2, 2, 6, 1.0, None)),
        ("broadcast_mid", L.npvp_broadcast_mid, (None, P, 2, 2, 8, 1.0, None)),
        ("broadcast_mid", L.npvp_broadcast_mid, (P, None, 2, 2, 8, 1.0, None)),
        ("colsum", L.npvp_colsum, (P, 8, 6, 8, P, 0, P, big, None)),                                             # N % 4
        ("colsum", L.npvp_colsum, (P, 8, 8, 10, P, 0, P, big, None)),                                            # ld % 4
        ("colsum", L.npvp_colsum, (P, 8, 8, 8, P, 0, P, L.npvp_colsum_workspace_bytes(8, 8) - 1, None)),         # one byte short
        ("colsum", L.npvp_colsum, (P, 8, 8, 8, P, 0, None, big, None)),
        ("colsum", L.npvp_colsum, (None, 8, 8, 8, P, 0, P, big, None)),
        ("colsum", L.npvp_colsum, (P, 8, 8, 8, None, 0, P, big, None)),
        ("dwtb_build", L.npvp_dwtb_build, (P, P, P, 0, None)),
        ("dwtb_build", L.npvp_dwtb_build, (None, P, P, 4, None)),
        ("dwtb_accumulate", L.npvp_dwtb_accumulate, (P, P, None, 4, None)),
        ("l1_mean", L.npvp_l1_mean, (off, P, 16, 1.0, P, P, 4096, None)),                                        # a off alignment
        ("l1_mean", L.npvp_l1_mean, (P, off, 16, 1.0, P, P, 4096, None)),
        ("l1_mean", L.npvp_l1_mean, (P, P, 16, 1.0, P, P, 4095, None)),                                          # one byte short
        ("l1_mean_bwd", L.npvp_l1_mean_bwd, (off, P, 16, P, 1.0, P, None)),
        ("l1_mean_bwd", L.npvp_l1_mean_bwd, (P, P, 16, P, 1.0, off, None)),
        ("sum_all", L.npvp_sum_all, (off, 16, P, P, 4096, None)),
        ("sum_all", L.npvp_sum_all, (P, 16, P, P, 4095, None)),
        ("grad_norm_clip", L.npvp_grad_norm_clip, (off, 16, 1.0, P, P, 4096, None)),
        ("grad_norm_clip", L.npvp_grad_norm_clip, (P, 16, 1.0, P, P, 4095, None)),
        ("grad_norm_clip", L.npvp_grad_norm_clip, (None, 16, 1.0, P, P, 4096, None)),                            # a null g
        ("grad_norm_clip", L.npvp_grad_norm_clip, (P, 16, 1.0, None, P, 4096, None)),
        ("adamw", L.npvp_adamw_step, (off, P, P, P, 16, P, 0.9, 0.999, 1e-8, 0.01, None, 0, 0, 1, None)),
        ("adamw", L.npvp_adamw_step, (P, P, P, off, 16, P, 0.9, 0.999, 1e-8, 0.01, None, 0, 0, 1, None)),
        ("adamw", L.npvp_adamw_step, (None, P, P, P, 16, P, 0.9, 0.999, 1e-8, 0.01, None, 0, 0, 1, None)),
        ("adamw", L.npvp_adamw_step, (P, P, None, P, 16, P, 0.9, 0.999, 1e-8, 0.01, None, 0, 0, 1, None)),
        ("adamw", L.npvp_adamw_step, (P, P, P, P, 16, P, 0.9, 0.999, 1e-8, 0.01, P, 9, 5, 1, None)),             # clip_begin > clip_end
        ("adamw", L.npvp_adamw_step, (P, P, P, P, 16, P, 0.9, 0.999, 1e-8, 0.01, P, 4, 17, 1, None)),            # clip_end > n
        ("bias_act", L.npvp_bias_act, (P, P, None, P, 4, 8, 4, 0, 1, None)),                                     # layout 0, inner != C
        ("bias_act", L.npvp_bias_act, (P, P, None, P, 4, 8, 8, 0, 4, None)),                                     # act = 4
        ("bias_act", L.npvp_bias_act, (P, P, None, P, 4, 8, 8, 2, 1, None)),
        ("act_bwd", L.npvp_act_bwd, (P, P, P, 16, 4, None)),
        ("sqdiff_per_image", L.npvp_sqdiff_per_image, (P, P, 2, 64, 1.0, 1.0, P, P, L.npvp_sqdiff_workspace_bytes(2, 64) - 1, None)),
        ("sqdiff_per_image", L.npvp_sqdiff_per_image, (P, P, 2, 64, 0.0, 1.0, P, P, big, None)),
        ("ssim_per_image", L.npvp_ssim_per_image, (P, P, 1, 1, 8, 8, taps.ctypes.data, 9, P, P, big, None)),     # window_size = 9
        ("ssim_per_image", L.npvp_ssim_per_image, (P, P, 1, 1, 40, 40, taps.ctypes.data, 11, P, P, L.npvp_ssim_workspace_bytes(1, 1, 40, 40) - 1, None)),
        ("ssim_per_image", L.npvp_ssim_per_image, (P, P, 65536, 1, 1, 1, taps.ctypes.data, 11, P, P, 65536 * 4, None)),   # N * C >= 65536
        ("u8hwc_to_f32chw", L.npvp_u8hwc_to_f32chw, (P, P, 65536, 1, 1, 1, mean.ctypes.data, mean.ctypes.data, None)),
    ]
    for name, fn, args in calls:
        rc = fn(*args)
        assert rc < 0, f"npvp_{name}{args[2:]} was accepted"
        assert name.encode() in (L.npvp_last_error() or b""), (name, L.npvp_last_error())
    torch.cuda.synchronize()
