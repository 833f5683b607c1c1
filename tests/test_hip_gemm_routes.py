"""GPU: every leaf of the GEMM dispatcher (tests/gemm_route_cases.py) against the fp64 product of the same operands, at ragged
tiles, with leading dimensions that differ from the logical widths, and with a look at what a launch must NOT touch.

Every operand and every output is a view into a larger buffer of this test, with padding on all four sides (nothing ends flush
with its allocation, so a stray access stays inside the test's own memory and shows as a wrong value):
  * the padding of A, B, bias, residual and aux_in is NaN - a NaN in a result is an operand read outside its logical extent;
  * the padding of C, aux_out and the bias gradient holds a bit pattern and must be bit-identical afterwards.
Bars are those of tests/test_hip_ops.py: whole-tensor rel-L2 1e-5 (5e-5 for f32 and bf16x3, as test_gemm_full_size_against_rocblas)
and the worst-row bar ROW_TOL of close().  The route of every launch is asserted at run time (npvp_gemm_route with `has_planes` as
the wrapper decided it): a mismatch fails, nothing is skipped - a case carries its own GEMM mode."""
import ctypes
import math

import pytest
import torch

import gemm_route_cases as T
from test_hip_ops import DEV, ROW_TOL, close

pytestmark = pytest.mark.gpu

PATTERN = 0x7FC0BEEF          # a quiet NaN with a payload: recognisable, and poison for whoever reads it as a number
PAD_R, PAD_C = 4, 8           # rows above / below, floats left / right of every view (16-byte aligned starts, ld % 4 == 0)


class Buf:
    """a [rows, cols] view inside a larger allocation: ld = cols + 2 * PAD_C (+ extra), PAD_R rows above and below"""

    def __init__(self, rows, cols, values=None, extra_ld=0, fill="nan"):
        ld = cols + 2 * PAD_C + extra_ld
        self.base = torch.empty(rows + 2 * PAD_R, ld, dtype=torch.float32, device=DEV)
        if fill == "nan":
            self.base.fill_(float("nan"))
        else:
            self.base.view(torch.int32).fill_(PATTERN)
        self.v = self.base[PAD_R:PAD_R + rows, PAD_C:PAD_C + cols]
        if values is not None:
            self.v.copy_(values)
        self.rows, self.cols = rows, cols

    def fill(self, values):
        self.base.view(torch.int32).fill_(PATTERN)
        self.v.copy_(values)
        return self

    def padding_intact(self):
        b = self.base.view(torch.int32).clone()
        b[PAD_R:PAD_R + self.rows, PAD_C:PAD_C + self.cols] = PATTERN
        return bool((b == PATTERN).all())


class Vec:
    """a length-n output vector with the bit pattern around it"""

    def __init__(self, n, values=None):
        self.base = torch.empty(n + 2 * PAD_C, dtype=torch.float32, device=DEV)
        self.base.view(torch.int32).fill_(PATTERN)
        self.v = self.base[PAD_C:PAD_C + n]
        self.n = n
        if values is not None:
            self.v.copy_(values)

    def padding_intact(self):
        i = self.base.view(torch.int32)
        return bool((i[:PAD_C] == PATTERN).all()) and bool((i[PAD_C + self.n:] == PATTERN).all())


def vec(n, values):
    """a length-n vector with NaN around it"""
    base = torch.full((n + 2 * PAD_C,), float("nan"), dtype=torch.float32, device=DEV)
    base[PAD_C:PAD_C + n] = values
    return base[PAD_C:PAD_C + n]


def tol_of(mode):
    return T.TOL[mode]


def test_the_table_holds_the_bars_of_this_suite():
    assert T.ROW_TOL == ROW_TOL and T.TOL == {"f32": 5e-5, "bf16x3": 5e-5, "bf16x6": 1e-5, "f16x3": 1e-5}
    assert (T.MEAN_TOL, T.RSTD_TOL) == (1e-6, 2e-6)


def route_now(a_kc, b_kc, M, N, K, mode, planes, plain):
    from npvp_amd._lib import lib
    out = (ctypes.c_int * 4)()
    assert lib().npvp_gemm_route(a_kc, b_kc, M, N, K, T.MODES[mode], int(planes), int(plain), ctypes.addressof(out)) == 0
    return tuple(out)


def assert_route(case, planes, plain=True):
    """the launch about to be made takes the route the table names (with the planes the wrapper really has)"""
    a_kc, b_kc = T.ROLES[case["role"]]
    r = route_now(a_kc, b_kc, case["M"], case["N"], case["K"], case["mode"], planes, plain)
    kid, variant, cls, parity = case["route"]
    if plain:
        got = (r[0], r[1], T.split_class(r[0], r[2]), "odd" if r[3] % 2 else "even")
        assert got == (kid, variant, cls, parity), f"route {got} ({r}), the table says {case['route']}"
    else:
        assert (r[0], r[1], r[2]) == (kid, variant, 1), f"route with an epilogue {r}, the table says {case['route']}"
    assert T.leaf_of(case["mode"], case["role"], planes, case.get("rowstats", False), r) == case["leaf"]
    return r


@pytest.fixture
def ops():
    """the library in whatever GEMM mode the case sets, back to the default afterwards"""
    import npvp_amd  # noqa: F401
    from npvp_amd import ops as o
    assert torch.cuda.is_available()
    dev = torch.device(DEV)
    o.rng.manual_seed(1234, dev)
    o.rng.begin_step(dev)
    yield o
    o.set_gemm_precision("f16x3")


def gelu64(u):
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def gelu_grad64(u):
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


FWD_CASES = [c for c in T.CASES if c["role"] != "wgrad" and not c.get("rowstats")]
STAT_CASES = [c for c in T.CASES if c.get("rowstats")]
WGRAD_CASES = [c for c in T.CASES if c["role"] == "wgrad"]


def ids(cs):
    return [f"{c['mode']}: {c['name']}" for c in cs]


def operands(ops, case, seed):
    """A [M, K] and the weight of a forward / dgrad case as padded views, their planes as the wrappers would make them, and the
    fp64 product"""
    M, N, K = case["M"], case["N"], case["K"]
    g = torch.Generator(device=DEV).manual_seed(seed)
    A = Buf(M, K, torch.randn(M, K, device=DEV, generator=g), extra_ld=4)
    if case["role"] == "fwd":
        W = Buf(N, K, torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K))
        ref = A.v.double() @ W.v.double().T
    else:
        W = Buf(K, N, torch.randn(K, N, device=DEV, generator=g) / math.sqrt(K), extra_ld=8)
        ref = A.v.double() @ W.v.double()
    assert A.v.stride(0) != K and W.v.stride(0) != W.v.shape[1]
    pl = None
    if case["planes"]:
        pl = ops.WeightPlanes.get(W.v, "F" if case["role"] == "fwd" else "D")
        assert (pl is not None) == (case["mode"] in ("bf16x6", "f16x3")), "planes exist in the bf16x6 and f16x3 modes"
    if M >= 256:          # what linear_fwd / linear_dgrad decide for this row count
        assert (ops._planes(W.v, "F" if case["role"] == "fwd" else "D", M) is not None) == (pl is not None), \
            "the table's `planes` is not what the wrappers would do"
    return A, W, pl, ref, g


@pytest.mark.parametrize("case", FWD_CASES, ids=ids(FWD_CASES))
def test_forward_and_dgrad_leaves(ops, case):
    """plain, bias + alpha, GELU + aux_out, ReLU + residual, act 3 / 4 with aux_in, accumulate, elementwise dropout, and on the fp16
    dgrads the row-group mask a_drop - each launch against fp64, the padding of every output bit-identical afterwards, c_amax exact (f16x3)"""
    ops.set_gemm_precision(case["mode"])
    mode, M, N, K = case["mode"], case["M"], case["N"], case["K"]
    a_kc, b_kc = T.ROLES[case["role"]]
    tol = tol_of(mode)
    A, W, pl, ref, g = operands(ops, case, 11)
    C = Buf(M, N, fill="pattern")
    ldc = C.v.stride(0)
    assert ldc == N + 2 * PAD_C

    def run(what, expect, plain=False, **kw):
        assert_route(case, pl is not None, plain=plain)
        if "keep_c" not in kw:
            C.base.view(torch.int32).fill_(PATTERN)
        kw.pop("keep_c", None)
        ops.gemm(a_kc, b_kc, M, N, K, A.v, A.v.stride(0), W.v, W.v.stride(0), C.v, b_pre=pl, **kw)
        assert bool(torch.isfinite(C.v).all()), f"{what}: a non-finite result - an operand was read outside its extent"
        close(C.v, expect, tol=tol, what=f"{case['leaf']} | {case['name']} | {what}")
        assert C.padding_intact(), f"{what}: the launch wrote outside C[:M, :N]"

    slot = ops.AmaxSlot.new(torch.device(DEV)) if mode == "f16x3" else None
    run("plain", ref, plain=True, c_amax=slot)
    if slot is not None:
        assert slot.read() == float(C.v.abs().max()), "c_amax is not max|C| over the valid region"
    bias = vec(N, torch.randn(N, device=DEV, generator=g))
    run("bias alpha=0.5", 0.5 * ref + bias.double(), bias=bias, alpha=0.5)
    pre = ref + bias.double()
    aux = Buf(M, N, fill="pattern")             # aux_out / aux_in are addressed with C's leading dimension
    run("gelu", gelu64(pre), bias=bias, act=1, aux_out=aux.v)
    close(aux.v, pre, tol=tol, what=f"{case['leaf']} | {case['name']} | aux_out")
    assert aux.padding_intact(), "aux_out: the launch wrote outside [:M, :N]"
    res = Buf(M, N, torch.randn(M, N, device=DEV, generator=g), extra_ld=12)
    assert res.v.stride(0) != ldc
    run("relu+residual", torch.relu(pre) + res.v.double(), bias=bias, act=2, residual=res.v)
    auxin = Buf(M, N, torch.randn(M, N, device=DEV, generator=g))
    run("act 3", ref * gelu_grad64(auxin.v.double()), act=3, aux_in=auxin.v)
    run("act 4", ref * (auxin.v.double() > 0), act=4, aux_in=auxin.v)
    c0 = torch.randn(M, N, device=DEV, generator=g)
    C.fill(c0)
    run("accumulate", c0.double() + ref, accumulate=True, keep_c=True)
    d = ops.Drop(0.25)
    mask = ops.drop_apply(torch.ones(M, N, device=DEV), d)
    keep = float((mask != 0).float().mean())
    assert abs(keep - 0.75) < 0.02, keep
    run("dropout", ref * mask.double(), drop=d)
    assert torch.equal(C.v != 0, mask != 0), "the kept pattern is not drop_apply's for the same site"
    if case["role"] == "dgrad" and case["route"][0] in (5, 7):
        # the backward of a DropPath site: the row-group mask folded into the rows of dy the fp16 kernel stages
        dp = ops.Drop(0.3, 1, 4, M // 4)
        Am = ops.drop_apply(A.v.contiguous(), dp)
        dead = int((Am.abs().sum(1) == 0).sum())
        assert 0 < dead < M, "the mask must drop some row groups and keep some"
        run("a_drop", Am.double() @ W.v.double(), a_drop=dp)
        assert torch.equal(C.v.abs().sum(1) == 0, Am.abs().sum(1) == 0), "dropped rows must be exactly zero"


@pytest.mark.parametrize("case", STAT_CASES, ids=ids(STAT_CASES))
def test_frame_statistics_leaves(ops, case):
    """the rowstats instantiations (fp16 and, in bf16x6, the wide and the 128 x 128 kernel's) with an odd number of 64-row frames (a half-empty last 128-row tile): output against fp64,
    frame mean / rstd against fp64 of the output, bars of test_linear_emits_frame_statistics"""
    from npvp_amd._lib import lib, check
    ops.set_gemm_precision(case["mode"])
    M, N, K = case["M"], case["N"], case["K"]
    assert ops.linear_frame_stats_supported(M, N) and (M // 64) % 2 == 1
    g = torch.Generator(device=DEV).manual_seed(21)
    A = Buf(M, K, torch.randn(M, K, device=DEV, generator=g) + 0.5, extra_ld=4)
    W = Buf(N, K, torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K))
    bias = vec(N, torch.randn(N, device=DEV, generator=g) + 2.0)
    pl = ops._planes(W.v, "F", M)
    assert pl is not None
    assert_route(case, True, plain=False)
    C = Buf(M, N, fill="pattern")
    frames = M // 64
    part = Buf(1, frames * (N // 64) * 2, fill="pattern")
    slot = ops.AmaxSlot.new(torch.device(DEV))
    ops.gemm(1, 1, M, N, K, A.v, A.v.stride(0), W.v, W.v.stride(0), C.v, bias=bias, b_pre=pl, rowstats=part.v, c_amax=slot)
    mean = torch.empty(frames, dtype=torch.float32, device=DEV)
    rstd = torch.empty_like(mean)
    check(lib().npvp_frame_stats_finalize(part.v.data_ptr(), N // 64, 4096.0, mean.data_ptr(), rstd.data_ptr(), frames, 1e-5,
                                          torch.cuda.current_stream().cuda_stream), "npvp_frame_stats_finalize")
    assert bool(torch.isfinite(C.v).all())
    close(C.v, A.v.double() @ W.v.double().T + bias.double(), tol=tol_of(case["mode"]), what=f"{case['leaf']} | {case['name']} | output")
    assert C.padding_intact() and part.padding_intact(), "the launch wrote outside C or outside the statistics partials"
    assert slot.read() == float(C.v.abs().max())
    fr = C.v.double().reshape(frames, -1)
    close(mean, fr.mean(1).float(), tol=T.MEAN_TOL, what=f"{case['leaf']} | {case['name']} | mean")
    close(rstd, (1.0 / torch.sqrt(fr.var(1, unbiased=False) + 1e-5)).float(), tol=T.RSTD_TOL, what=f"{case['leaf']} | {case['name']} | rstd")


@pytest.mark.parametrize("case", WGRAD_CASES, ids=ids(WGRAD_CASES))
def test_weight_gradient_leaves(ops, case):
    """dw[M, N] = dy[K, M]^T x[K, N]: overwrite and accumulate (alpha = 0.5), with and without the fused bias gradient; f16x3:
    the range flag stays 0 on well-ranged operands, and the row-group mask `a_drop` on the case that asks for it"""
    ops.set_gemm_precision(case["mode"])
    mode, M, N, K = case["mode"], case["M"], case["N"], case["K"]
    tol = tol_of(mode)
    dev = torch.device(DEV)
    g = torch.Generator(device=DEV).manual_seed(31)
    dy = Buf(K, M, torch.randn(K, M, device=DEV, generator=g), extra_ld=4)
    x = Buf(K, N, torch.randn(K, N, device=DEV, generator=g))
    ref = dy.v.double().T @ x.v.double()
    ref_b = dy.v.double().sum(0)
    C = Buf(M, N, fill="pattern")
    dbv = Vec(M)
    db, db_base = dbv.v, dbv.base
    ops.RangeGuard.reset()
    flag = ops.RangeGuard.flag(dev) if mode == "f16x3" else None
    name = f"{case['leaf']} | {case['name']}"

    def run(what, expect, expect_b=None, **kw):
        assert_route(case, False)
        ops.gemm(0, 0, M, N, K, dy.v, dy.v.stride(0), x.v, x.v.stride(0), C.v, range_flag=flag, **kw)
        assert bool(torch.isfinite(C.v).all()), f"{what}: a non-finite result - an operand was read outside its extent"
        close(C.v, expect, tol=tol, what=f"{name} | {what}")
        assert C.padding_intact(), f"{what}: the launch wrote outside dw[:M, :N]"
        if expect_b is not None:
            close(db.reshape(1, -1), expect_b.reshape(1, -1), tol=tol, what=f"{name} | {what} bias gradient")
            assert dbv.padding_intact(), f"{what}: wrote outside db[:M]"

    run("overwrite", ref)
    db_base.view(torch.int32).fill_(PATTERN)
    C.base.view(torch.int32).fill_(PATTERN)
    run("overwrite + bias gradient", ref, ref_b, colsum_a=db)
    c0, b0 = torch.randn(M, N, device=DEV, generator=g), torch.randn(M, device=DEV, generator=g)
    C.fill(c0)
    run("accumulate alpha=0.5", c0.double() + 0.5 * ref, accumulate=True, alpha=0.5)
    C.fill(c0)
    db.copy_(b0)
    run("accumulate + bias gradient", c0.double() + ref, b0.double() + ref_b, accumulate=True, colsum_a=db)
    if flag is not None:
        assert ops.RangeGuard.poll(dev) == 0, "well-ranged ragged operands raised the range flag"
    if case.get("adrop"):
        g1, g2 = 16, K // 16
        d = ops.Drop(0.3, 1, g1, g2)
        dym = ops.drop_apply(dy.v.contiguous(), d)
        dead = int((dym.view(g2, -1).abs().sum(1) == 0).sum())
        assert 0 < dead < g2, "the mask must drop some groups and keep some"
        C.base.view(torch.int32).fill_(PATTERN)
        db_base.view(torch.int32).fill_(PATTERN)
        run("a_drop", dym.double().T @ x.v.double(), dym.double().sum(0), colsum_a=db, a_drop=d)
        assert ops.RangeGuard.poll(dev) == 0
    ops.RangeGuard.reset()


def test_chained_weight_gradient_on_a_ragged_shape(ops):
    """npvp_wgrad_f16_chained + npvp_splitk_reduce_job at 1 120 token rows (2 splits of 35 K-steps), ragged 520 x 264 output, padded
    strides: against fp64, and bit-identical to npvp_gemm_f32's weight gradient + reduction launch"""
    from npvp_amd._lib import lib, check
    L = lib()
    ops.set_gemm_precision("f16x3")
    M, N, K = 520, 264, 1120
    assert L.npvp_wgrad_f16_chainable(M, N, K) == 1 and route_now(0, 0, M, N, K, "f16x3", 0, 1) == (6, 0, 2, 35)
    g = torch.Generator(device=DEV).manual_seed(41)
    dy = Buf(K, M, torch.randn(K, M, device=DEV, generator=g), extra_ld=4)
    x = Buf(K, N, torch.randn(K, N, device=DEV, generator=g))
    two, one = Buf(M, N, fill="pattern"), Buf(M, N, fill="pattern")
    dbv2, dbv1 = Vec(M), Vec(M)
    db2, db1 = dbv2.v, dbv1.v
    ops.gemm(0, 0, M, N, K, dy.v, dy.v.stride(0), x.v, x.v.stride(0), two.v, colsum_a=db2)
    sa, sb = ops.amax_of(dy.v), ops.amax_of(x.v)
    wsb = L.npvp_wgrad_f16_chain_workspace_bytes(M, N, K)
    ws = torch.empty(wsb // 4 + 64, dtype=torch.float32, device=DEV)
    job = ctypes.create_string_buffer(64)
    st = torch.cuda.current_stream().cuda_stream
    check(L.npvp_wgrad_f16_chained(M, N, K, dy.v.data_ptr(), dy.v.stride(0), x.v.data_ptr(), x.v.stride(0), one.v.data_ptr(),
                                   one.v.stride(0), db1.data_ptr(), 0, sa.data_ptr(), sb.data_ptr(), None, 0.0, 1, 1, 0, None, None,
                                   ctypes.addressof(job), ws.data_ptr(), wsb, st), "npvp_wgrad_f16_chained")
    check(L.npvp_splitk_reduce_job(ctypes.addressof(job), st), "npvp_splitk_reduce_job")
    torch.cuda.synchronize()
    close(one.v, dy.v.double().T @ x.v.double(), tol=1e-5, what="wgrad f16 chained | 520x264x1120 | dw")
    close(db1.reshape(1, -1), dy.v.double().sum(0).reshape(1, -1), tol=1e-5, what="wgrad f16 chained | 520x264x1120 | bias gradient")
    assert one.padding_intact() and two.padding_intact() and dbv1.padding_intact() and dbv2.padding_intact()
    assert torch.equal(one.v, two.v) and torch.equal(db1, db2), "chained and stand-alone reductions differ"


def test_one_launch_backward_on_a_ragged_shape(ops):
    """npvp_linear_bwd_f16 at R = 1 056 token rows (R % 64 != 0: the dgrad runs on 128 x 64 tiles, the weight gradient in 3 splits of
    22 K-steps): dx and dw against fp64 and bit-identical to the two launches.  A layer with ragged N / K is not taken
    (npvp_linear_bwd_f16_takes(1056, 520, 264) == 0: the small-tile dgrads need N % 128 == 0) - asserted."""
    from npvp_amd._lib import lib, check
    L = lib()
    ops.set_gemm_precision("f16x3")
    dev = torch.device(DEV)
    R, N, K = 1056, 512, 512
    assert L.npvp_linear_bwd_f16_takes(R, N, K) == 1 and L.npvp_linear_bwd_f16_takes(1056, 520, 264) == 0
    assert route_now(1, 0, R, K, N, "f16x3", 1, 0)[:2] == (7, 3) and route_now(0, 0, N, K, R, "f16x3", 0, 1) == (6, 0, 3, 22)
    g = torch.Generator(device=DEV).manual_seed(51)
    dy = Buf(R, N, torch.randn(R, N, device=DEV, generator=g), extra_ld=4)
    x = Buf(R, K, torch.randn(R, K, device=DEV, generator=g))
    W = Buf(N, K, torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K), extra_ld=8)
    auxin = Buf(R, K, torch.randn(R, K, device=DEV, generator=g))
    pl = ops._planes(W.v, "D", R)
    assert pl is not None
    planes, w_amax = pl
    gw0, gb0 = torch.randn(N, K, device=DEV, generator=g), torch.randn(N, device=DEV, generator=g)
    # two launches
    dx2 = Buf(R, K, fill="pattern")
    ops.linear_dgrad(dy.v, W.v, act=4, aux_in=auxin.v, out=dx2.v)
    gw2, gbv2 = Buf(N, K, fill="pattern").fill(gw0), Vec(N, gb0)
    gb2 = gbv2.v
    ops.gemm(0, 0, N, K, R, dy.v, dy.v.stride(0), x.v, x.v.stride(0), gw2.v, colsum_a=gb2, accumulate=True)
    # one launch
    dx1 = Buf(R, K, fill="pattern")
    gw1, gbv1 = Buf(N, K, fill="pattern").fill(gw0), Vec(N, gb0)
    gb1 = gbv1.v
    sa, sx = ops.amax_of(dy.v), ops.amax_of(x.v)
    wsb = L.npvp_wgrad_f16_chain_workspace_bytes(N, K, R)
    ws = torch.empty(wsb // 4 + 64, dtype=torch.float32, device=DEV)
    job = ctypes.create_string_buffer(64)
    st = torch.cuda.current_stream().cuda_stream
    assert auxin.v.stride(0) == dx1.v.stride(0)
    check(L.npvp_linear_bwd_f16(R, N, K, dy.v.data_ptr(), dy.v.stride(0), sa.data_ptr(), planes.data_ptr(), w_amax.data_ptr(),
                                dx1.v.data_ptr(), dx1.v.stride(0), 4, auxin.v.data_ptr(), None, 0, 0.0, 0, 1, 1, 0, None,
                                x.v.data_ptr(), x.v.stride(0), sx.data_ptr(), gw1.v.data_ptr(), gw1.v.stride(0), gb1.data_ptr(),
                                None, 0.0, 1, 1, 0, None, None, ctypes.addressof(job), ws.data_ptr(), wsb, st), "npvp_linear_bwd_f16")
    check(L.npvp_splitk_reduce_job(ctypes.addressof(job), st), "npvp_splitk_reduce_job")
    torch.cuda.synchronize()
    close(dx1.v, (dy.v.double() @ W.v.double()) * (auxin.v.double() > 0), tol=1e-5, what="one-launch backward | 1056x512x512 | dx")
    close(gw1.v, gw0.double() + dy.v.double().T @ x.v.double(), tol=1e-5, what="one-launch backward | 1056x512x512 | dw")
    close(gb1.reshape(1, -1), (gb0.double() + dy.v.double().sum(0)).reshape(1, -1), tol=1e-5, what="one-launch backward | 1056x512x512 | db")
    assert dx1.padding_intact() and gw1.padding_intact() and dx2.padding_intact() and gw2.padding_intact()
    assert gbv1.padding_intact() and gbv2.padding_intact(), "a bias gradient was written outside db[:N]"
    assert torch.equal(dx1.v, dx2.v), "the fused dgrad differs from the stand-alone launch"
    assert torch.equal(gw1.v, gw2.v) and torch.equal(gb1, gb2), "the fused weight gradient differs from the stand-alone launch"


# ---- what a C caller may leave out: the workspace and the amax slots (ops.gemm always hands both over, and npvp_gemm_route answers for
# a caller that does - so these branches of the planner are reached through ctypes only).  Bars: bf16x6's, as every launch below
# runs on the three-term bf16 kernels.

def raw_gemm(a_kc, b_kc, M, N, K, A, B, C, prec, bias=None, colsum=None, planes=None, a_amax=None, b_amax=None, ws=None, wsn=0,
             adrop_p=0.0, seed=None):
    """npvp_gemm_f32 as a C caller sees it -> (return code, launches made)"""
    from npvp_amd._lib import lib
    L = lib()
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    n0 = L.npvp_launch_count()
    rc = L.npvp_gemm_f32(a_kc, b_kc, M, N, K, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), C.data_ptr(), C.stride(0),
                         ptr(bias), 0, None, None, None, 0, 0.0, 0, 1, 1, ptr(seed), 0, 1.0, prec, ptr(colsum), ptr(planes), 0, None,
                         ptr(a_amax), ptr(b_amax), None, None, adrop_p, 4, max(M // 4, 1), 0, ptr(ws), wsn,
                         torch.cuda.current_stream().cuda_stream)
    return rc, L.npvp_launch_count() - n0


def test_fp16_forward_without_an_amax_slot_runs_as_bf16x6_without_planes(ops):
    """precision 6 with fp16 planes but no a_amax, on a shape gemm_f16_kernel would take: the three-term bf16 kernel without planes,
    bit-identical to the precision-4 call that hands no planes over"""
    ops.set_gemm_precision("f16x3")
    M, N, K = 2080, 224, 96
    assert route_now(1, 1, M, N, K, "f16x3", 1, 1)[:2] == (5, 1) and route_now(1, 1, M, N, K, "bf16x6", 0, 1) == (1, 0, 1, 6)
    g = torch.Generator(device=DEV).manual_seed(61)
    A = Buf(M, K, torch.randn(M, K, device=DEV, generator=g), extra_ld=4)
    W = Buf(N, K, torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K))
    planes, w_amax = ops.WeightPlanes.get(W.v, "F")
    six, four = Buf(M, N, fill="pattern"), Buf(M, N, fill="pattern")
    assert raw_gemm(1, 1, M, N, K, A.v, W.v, six.v, 6, planes=planes, b_amax=w_amax) == (0, 1)
    assert raw_gemm(1, 1, M, N, K, A.v, W.v, four.v, 4) == (0, 1)
    close(six.v, A.v.double() @ W.v.double().T, tol=T.TOL["bf16x6"], what="f16x3 without a_amax | 2080x224x96")
    assert six.padding_intact() and four.padding_intact()
    assert torch.equal(six.v, four.v), "precision 6 without an amax slot is not the bf16x6 launch without planes"


@pytest.mark.parametrize("short_by", [None, 4], ids=["no workspace", "workspace 4 bytes short"])
def test_fp16_weight_gradient_without_its_workspace_runs_unsplit(ops, short_by):
    """precision 6, both amax slots, 5 splits planned (npvp_gemm_route), but no workspace / one 4 bytes short of the fp16 kernel's
    need: the unsplit 128 x 128 bf16 kernel, bit-identical to the precision-4 call without a workspace, bias gradient included"""
    from npvp_amd._lib import lib
    ops.set_gemm_precision("f16x3")
    M, N, K = 520, 264, 2080
    assert route_now(0, 0, M, N, K, "f16x3", 0, 1) == (6, 0, 5, 26) and route_now(0, 0, M, N, K, "bf16x6", 0, 1) == (1, 0, 5, 26)
    g = torch.Generator(device=DEV).manual_seed(62)
    dy = Buf(K, M, torch.randn(K, M, device=DEV, generator=g), extra_ld=4)
    x = Buf(K, N, torch.randn(K, N, device=DEV, generator=g))
    sa, sb = ops.amax_of(dy.v), ops.amax_of(x.v)
    need = lib().npvp_wgrad_f16_chain_workspace_bytes(M, N, K)
    assert need > 0 and need <= lib().npvp_gemm_workspace_bytes(M, N, K)
    ws, wsn = (None, 0) if short_by is None else (torch.empty(need // 4 + 64, dtype=torch.float32, device=DEV), need - short_by)
    six, four = Buf(M, N, fill="pattern"), Buf(M, N, fill="pattern")
    db6, db4 = Vec(M), Vec(M)
    assert raw_gemm(0, 0, M, N, K, dy.v, x.v, six.v, 6, colsum=db6.v, a_amax=sa, b_amax=sb, ws=ws, wsn=wsn) == (0, 1)
    assert raw_gemm(0, 0, M, N, K, dy.v, x.v, four.v, 4, colsum=db4.v) == (0, 1)
    close(six.v, dy.v.double().T @ x.v.double(), tol=T.TOL["bf16x6"], what="f16x3 wgrad without workspace | 520x264x2080 | dw")
    close(db6.v.reshape(1, -1), dy.v.double().sum(0).reshape(1, -1), tol=T.TOL["bf16x6"], what="f16x3 wgrad without workspace | 520x264x2080 | db")
    assert six.padding_intact() and four.padding_intact() and db6.padding_intact() and db4.padding_intact()
    assert torch.equal(six.v, four.v) and torch.equal(db6.v, db4.v), "not the unsplit bf16x6 launch"


def test_split_k_forward_with_and_without_a_workspace(ops):
    """a forward shape pick_splits splits 8 ways (6 tiles, K = 2048, plain): two launches with a workspace, one without, both within
    the bars; with a bias it is never split - one launch, bit-identical with and without a workspace"""
    from npvp_amd._lib import lib
    ops.set_gemm_precision("bf16x6")
    M, N, K = 260, 136, 2048
    assert route_now(1, 1, M, N, K, "bf16x6", 0, 1) == (1, 0, 8, 16) and route_now(1, 1, M, N, K, "bf16x6", 0, 0) == (1, 0, 1, 128)
    g = torch.Generator(device=DEV).manual_seed(63)
    A = Buf(M, K, torch.randn(M, K, device=DEV, generator=g), extra_ld=4)
    W = Buf(N, K, torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K))
    bias = vec(N, torch.randn(N, device=DEV, generator=g))
    ref = A.v.double() @ W.v.double().T
    wsb = lib().npvp_gemm_workspace_bytes(M, N, K)
    assert wsb > 0
    ws = torch.empty(wsb // 4 + 64, dtype=torch.float32, device=DEV)
    out = {}
    for name, b, w, launches in (("split", None, ws, 2), ("no workspace", None, None, 1), ("bias", bias, ws, 1), ("bias, no workspace", bias, None, 1)):
        C = Buf(M, N, fill="pattern")
        assert raw_gemm(1, 1, M, N, K, A.v, W.v, C.v, 4, bias=b, ws=w, wsn=wsb if w is not None else 0) == (0, launches), name
        close(C.v, ref if b is None else ref + b.double(), tol=T.TOL["bf16x6"], what=f"db3<1,1> | 260x136x2048 | {name}")
        assert C.padding_intact(), name
        out[name] = C.v.clone()
    assert torch.equal(out["bias"], out["bias, no workspace"]), "a launch with an epilogue must not depend on the workspace"


def test_a_drop_on_a_shape_the_fp16_kernels_decline_is_an_argument_error(ops):
    """adrop_p > 0 with precision 6 at M = 68 (gemm_f16_variant takes 128 rows or more): the argument error, nothing launched"""
    ops.set_gemm_precision("f16x3")
    M, N, K = 68, 136, 64
    assert route_now(1, 0, M, N, K, "f16x3", 1, 1)[0] == 1
    g = torch.Generator(device=DEV).manual_seed(64)
    A = Buf(M, K, torch.randn(M, K, device=DEV, generator=g))
    W = Buf(K, N, torch.randn(K, N, device=DEV, generator=g))
    planes, w_amax = ops.WeightPlanes.get(W.v, "D")
    sa = ops.amax_of(A.v)
    seed = torch.zeros(2, dtype=torch.int64, device=DEV)
    C = Buf(M, N, fill="pattern")
    assert raw_gemm(1, 0, M, N, K, A.v, W.v, C.v, 6, planes=planes, a_amax=sa, b_amax=w_amax, adrop_p=0.25, seed=seed) == (-1, 0)
    torch.cuda.synchronize()
    assert bool((C.base.view(torch.int32) == PATTERN).all()), "the refused call wrote to C"
    assert raw_gemm(1, 0, M, N, K, A.v, W.v, C.v, 6, planes=planes, a_amax=sa, b_amax=w_amax) == (0, 1)
    close(C.v, A.v.double() @ W.v.double(), tol=T.TOL["bf16x6"], what="db3 planes dropped | 68x136x64 | after the refused call")
