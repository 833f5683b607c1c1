"""GPU: the kernels of the shipped 8 x 8 x 512 point, one entry point at a time against float64 at 1e-5 on the whole tensor and on
the worst row (a frame mean: 1e-5 sigma) - MlpDWBN's fused middle and its neighbours through the C ABI (npvp_amd._lib.lib()), the
norms and the attention cores through the npvp_amd.ops call sites the models use.  Cases, references, bound and comparison:
tests/hot_kernel_cases.py; tests/test_hot_kernel_cases_host.py shows that those cases reject a wrong kernel.  One recorded run:
profiles/hot_kernels_errors.txt (NPVP_ERR_LOG=<file> appends `case output error worst-row-error fp32-cpu-error`).

The fused middle's BACKWARD (families mid_bwd and mid_n2 of the cases file) makes its calls from the plans of tests/mid_bwd_calls.py:
every operand's size is a record there, held on the CPU to the extents the kernels index before anything runs here.

Through the C ABI every operand is a view into a NaN-padded allocation and every output, buffer updated in place and workspace a
view into one filled with the bit pattern 0x7FC0BEEF, which must be intact around the view afterwards (helper_kernel_cases.Flat)."""
import ctypes

import pytest
import torch

import hot_kernel_cases as HK
import mid_bwd_calls as MC
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


# ------------------------------------------------------------------------------------------------------------------- middle, backward
class Plan:
    """runs the steps of a call plan (tests/mid_bwd_calls.py): every buffer is allocated from its record - this file names no operand
    size - and after every call everything that is not an input must be intact around its view.  bufs: {buf name: Flat}"""

    def __init__(self, L, tensors):
        self.L, self.tensors, self.bufs, self.keep, self.host = L, dict(tensors), {}, [], {}

    def value(self, name, count):
        t = self.bufs[name].v if name in self.bufs else self.tensors[name]
        assert t.numel() == count, f"{name}: {t.numel()} values for a record of {count}"
        return t

    def operand(self, r, missing):
        if r.role == "null":
            return None
        if r.role == "host":                    # job records in host memory: a new one, or the one an earlier call wrote
            if r.fill is None:
                self.host[r.buf] = ctypes.create_string_buffer(4 * r.count)
            return ctypes.addressof(self.host[r.fill or r.buf])
        if r.role == "seed":                    # one 64-bit word, as tests/test_hip_helper_kernels.py::run_drop builds it
            assert r.count == MC.SEED_FLOATS
            s = torch.tensor([-1, -1, MC.DROP_SEED, -1, -1], dtype=torch.int64, device=DEV)[2:3]
            self.keep.append(s)
            return s.data_ptr()
        if r.role == "slot":
            assert r.count == AMAX_SLOT_FLOATS
            f = slot()
        elif r.role in ("in", "inout"):
            known = r.fill in self.bufs or r.fill in self.tensors
            v = self.value(r.fill, r.count) if known or missing is None else missing(r.count)
            f = Flat(v) if r.role == "in" else out_flat(r.count, v)
        else:
            assert r.role in ("out", "workspace"), r
            f = out_flat(r.count)
        if r.buf is not None:
            self.bufs[r.buf] = f
        self.keep.append(f)
        return f.ptr

    def launch(self, c, missing=None):
        """-> (return code, {role: the Flats of this call with it}).  missing: count -> values for an operand no step has made"""
        mine, args = {}, []
        for a in c.args:
            if isinstance(a, MC.Val):
                args.append(stream() if a.value == MC.STREAM else a.value)
                continue
            before = len(self.keep)
            args.append(self.operand(a, missing))
            mine.setdefault(a.role, []).extend(self.keep[before:])
        return getattr(self.L, c.entry)(*args), mine

    def run(self, steps):
        for s in steps:
            if isinstance(s, MC.Derive):
                self.tensors[s.name] = s.fn(self.bufs[s.source].cpu())
                continue
            rc, _ = self.launch(s)
            ok(self.L, rc, s.entry)
            for name, f in self.bufs.items():
                assert f.intact(), f"{s.entry}: written outside the extent of {name}"
            for name in s.untouched:
                assert bool((self.bufs[name].base.view(torch.int32) == PATTERN).all()), f"{s.entry} wrote {name}"
        return self

    def cpu(self, name, *shape):
        return self.bufs[name].cpu(*shape)

    def frame_sums(self, name, frames):
        """[frames][partials][2] -> [frames, 2]: a frame's partials added in float64"""
        return self.cpu(name).double().reshape(frames, -1, 2).sum(1)


def norm1_backward(p, Fr, Ch):
    """what every plan ends with: npvp_frameln_act_bwd_apply on the middle's own da1 and psum - and its amax slot is max |dh1| to the bit"""
    dh1 = p.cpu("dh1", Fr, 64, Ch)
    assert float(p.cpu("dh1_amax").max()) == float(dh1.abs().max()), "the amax slot of dh1"
    return dict(dh1=dh1, dw1n=p.cpu("dw1n", 64, Ch), db1n=p.cpu("db1n", 64, Ch))


@pytest.mark.parametrize("case", HK.MID_BWD, ids=HK.case_id)
def test_mid_bwd(L, case):
    """mlpdw_mid_bwd_kernel<1, false>: npvp_mlpdw_mid_bwd with accumulate 0, 1 (onto prior_dwt) and 2 (dwt_db left alone), the
    partials of the last through npvp_mlpdw_mid_bwd_reduce (accumulate 0 and 1), _reduce_into and _reduce_job + npvp_sum_rows_multi
    (onto prior_gw / prior_gb) - each against float64, none against another -, and norm1's backward on the kernel's own da1 and psum.
    127 | 128 | 129 frames: a chunk per frame, 128 chunks, 65 chunks of 2 with a last of 1."""
    Fr, Ch, kind = case
    p = Plan(L, MC.tensors("mid_bwd", case)).run(MC.plan("mid_bwd", case))
    got = dict(da1=p.cpu("da1", Fr, 64, Ch), dwt_db=p.cpu("dwt_db", 10, Ch), dwt_db_acc=p.cpu("dwt_db_acc", 10, Ch),
               psum=p.frame_sums("psum", Fr), gw=p.cpu("gw", Ch, 9), gb=p.cpu("gb"), **norm1_backward(p, Fr, Ch))
    for tag in ("_b", "_c"):                 # (the same launch but for where dwt_db goes)
        assert torch.equal(p.bufs["da1" + tag].v, p.bufs["da1"].v) and torch.equal(p.bufs["psum" + tag].v, p.bufs["psum"].v)
    label, ref, f32 = f"mid_bwd[{HK.case_id(case)}", HK.ref64("mid_bwd", case), HK.ref32("mid_bwd", case)
    failures = []
    for route, g in (("]", got), ("|reduce]", dict(dwt_db=p.cpu("dwt_db_r0", 10, Ch), dwt_db_acc=p.cpu("dwt_db_r1", 10, Ch))),
                     ("|reduce_job]", dict(gw=p.cpu("gw_q", Ch, 9), gb=p.cpu("gb_q")))):
        try:
            HK.close_dict(label + route, g, ref, f32)
        except AssertionError as e:           # (every route is measured and logged before the case fails)
            failures.append(str(e))
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("case", HK.MID_N2, ids=HK.case_id)
def test_mid_n2(L, case):
    """mlpdw_mid_bwd_kernel<1, true>: npvp_frameln_act_bwd_pgrad (norm2's frame sums as per_frame / 1024 partials, and its parameter
    gradients), npvp_mlpdw_mid_bwd_n2 on those partials - or, nparts2 = 1, on the frame's sums merged on the host - and norm1's backward
    behind it.  With dropout the reference takes the keep-scale that the kernels drew, recovered by npvp_drop_apply on ones with the
    same (p, salt, seed)."""
    Fr, Ch, drop_p, nparts2 = case
    p = Plan(L, MC.tensors("mid_n2", case)).run(MC.plan("mid_n2", case))
    got = dict(psum2=p.frame_sums("psum2", Fr), dw2n=p.cpu("dw2n", 64, Ch), db2n=p.cpu("db2n", 64, Ch), da1=p.cpu("da1", Fr, 64, Ch),
               dwt_db=p.cpu("dwt_db", 10, Ch), psum=p.frame_sums("psum", Fr), **norm1_backward(p, Fr, Ch))
    if drop_p == 0.0:
        return HK.close_all("mid_n2", case, got)
    keep = p.cpu("keep", Fr, 64, Ch)
    scale = float(keep.max())
    assert bool(((keep == 0) | (keep == scale)).all()) and abs(scale * (1.0 - drop_p) - 1.0) < 1e-6 and float(p.cpu("keep_amax").max()) == scale
    share = float((keep != 0).double().mean())
    assert abs(share - (1.0 - drop_p)) <= 4 * (drop_p * (1.0 - drop_p) / keep.numel()) ** 0.5, share
    HK.close_dict(f"mid_n2[{HK.case_id(case)}]", got, HK.mid_n2_reference(case, torch.float64, mask=keep.double()),
                  HK.mid_n2_reference(case, torch.float32, mask=keep.double()))


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_the_middle_refuses_what_it_cannot_run(L):
    """a grid that is not 8 x 8, Ch % 512 != 0, a short workspace: non-zero, a message, nothing written; and the backward's argument
    errors (mid_bwd_calls.refusals: nparts2 0 and 257, dropout without a seed or with p = 1, per_frame % 1024, nparts 0, a null psum,
    a workspace four bytes short for each producer), every other operand at the size of a call that runs"""
    for what, c, base, family, case in MC.refusals():
        p = Plan(L, MC.tensors(family, case))
        rc, mine = p.launch(c, missing=torch.zeros)
        assert not mine.get("inout")
        refused(L, rc, what, mine.get("out", []) + mine.get("workspace", []))
        assert all(s.intact() and not bool(s.v.any()) for s in mine.get("slot", [])), f"{what}: an amax slot was raised"
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
