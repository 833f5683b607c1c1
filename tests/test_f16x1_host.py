"""CPU: the one-term fp16 arithmetic ("f16x1", precision 7) up to the launch - the dispatcher's answers, the argument errors, the
decision ops.gemm takes per launch, the eval_arithmetic block, and the reference-side emulation (tests/f16x1_cases.py)."""
import ctypes
import math

import pytest
import torch

import f16x1_cases as X
import gemm_route_cases as T
import golden_cases as GC


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    from npvp_amd._lib import lib
    build.build(verbose=False)
    return lib()


def route(L, a_kc, b_kc, M, N, K, prec, planes, plain=1):
    out = (ctypes.c_int * 4)()
    assert L.npvp_gemm_route(a_kc, b_kc, M, N, K, prec, planes, plain, ctypes.addressof(out)) == 0, L.npvp_last_error()
    return tuple(out)


def test_precision_7_is_accepted_and_8_is_not(L):
    assert route(L, 1, 1, 2080, 224, 96, 7, 1) == (5, 1, 1, 3)
    assert route(L, 1, 1, 2080, 224, 96, 6, 1) == (5, 1, 1, 6)
    assert L.npvp_gemm_kernel_id(1, 1, 2080, 224, 96, 7, 1) == 5
    out = (ctypes.c_int * 4)()
    assert L.npvp_gemm_route(1, 1, 2080, 224, 96, 8, 1, 1, ctypes.addressof(out)) == -1
    assert L.npvp_gemm_route(1, 1, 2080, 224, 96, 3, 1, 1, ctypes.addressof(out)) == -1


def test_precision_7_routes_like_6_over_the_whole_table(L):
    """every shape of the table x every role x planes or none x plain or not: id, variant and splits of precision 6; on ids 5 / 7 one
    split and K / 32 steps of the launched kernel's own, the precision-6 answer everywhere else.  The one-term form is reached."""
    reached = set()
    for c in T.CASES:
        for role, (a_kc, b_kc) in T.ROLES.items():
            for planes in (0, 1):
                for plain in (0, 1):
                    six = route(L, a_kc, b_kc, c["M"], c["N"], c["K"], 6, planes, plain)
                    seven = route(L, a_kc, b_kc, c["M"], c["N"], c["K"], 7, planes, plain)
                    what = (c["name"], role, planes, plain)
                    assert seven[:3] == six[:3], what
                    assert L.npvp_gemm_kernel_id(a_kc, b_kc, c["M"], c["N"], c["K"], 7, planes) == \
                        L.npvp_gemm_kernel_id(a_kc, b_kc, c["M"], c["N"], c["K"], 6, planes), what
                    if six[0] in (5, 7):
                        assert seven[2] == 1 and seven[3] == c["K"] // 32 and six[3] == c["K"] // 16, what
                        reached.add((six[0], six[1]))
                    else:
                        assert seven == six, what
    assert reached == {(5, 1), (7, 2), (7, 3), (7, 4)}, "the table reaches every tile variant of the fp16 kernels"


def test_the_other_precisions_answer_as_before(L):
    assert route(L, 1, 1, 20480, 2048, 512, 4, 1) == (2, 1, 1, 32) and route(L, 1, 1, 20480, 512, 512, 0, 1) == (0, 0, 1, 16)
    assert route(L, 0, 0, 512, 512, 8192, 6, 0) == (6, 0, 32, 16) and route(L, 0, 0, 512, 512, 8192, 7, 0) == (6, 0, 32, 16)
    assert route(L, 1, 1, 64, 512, 512, 7, 1) == route(L, 1, 1, 64, 512, 512, 6, 1) == (1, 0, 1, 32)
    assert route(L, 1, 1, 2080, 224, 96, 5, 1) == (1, 0, 1, 6)


def raw_gemm(L, prec, adrop_p=0.0, skip_p=0.0, seed=0x1000):
    """npvp_gemm_f32_skip on made-up (aligned, never dereferenced) addresses: only calls that must be refused before a launch"""
    p = 0x10000
    return L.npvp_gemm_f32_skip(1, 0, 256, 128, 64, p, 64, p, 128, p, 128, None, 0, None, None, None, 0, 0.0, 0, 1, 1, seed, 0, 1.0, prec,
                                None, p, 0, None, p, p, None, None, adrop_p, 4, 64, 0, skip_p, 4, 64, 0, None, 0, None)


def test_precision_7_takes_no_row_mask_and_no_row_skip(L):
    n0 = L.npvp_launch_count()
    assert raw_gemm(L, 7, adrop_p=0.25) == -1 and b"precision 7" in L.npvp_last_error()
    assert raw_gemm(L, 7, skip_p=0.25) == -1 and b"precision 7" in L.npvp_last_error()
    assert raw_gemm(L, 7, adrop_p=0.25, skip_p=0.25) == -1
    assert raw_gemm(L, 8) == -1 and b"precision must be" in L.npvp_last_error()
    assert L.npvp_launch_count() == n0, "a refused call launched something"


def test_the_launch_decision_both_sides_of_every_input():
    from npvp_amd.ops import eval_launch_precision as d
    assert d("f16x1", 6, 5, True) == 7 and d("f16x1", 6, 7, True) == 7
    assert d("f16x3", 6, 5, True) == 6                                        # the arithmetic
    assert d("f16x1", 4, 5, True) == 4 and d("f16x1", 0, 5, True) == 0         # the GEMM mode
    for kid in (0, 1, 2, 3, 4, 6):                                            # the kernel
        assert d("f16x1", 6, kid, True) == 6
    assert d("f16x1", 6, 5, False) == 6 and d("f16x1", 6, 7, False) == 6       # autograd
    assert d("f16x1", 6, 5, True, masked=True) == 6 and d("f16x1", 6, 5, True, masked=False) == 7


def test_the_block_nests_counts_and_refuses_unknown_names():
    import npvp_amd
    from npvp_amd import ops
    assert npvp_amd.eval_arithmetic is ops.eval_arithmetic and ops.eval_arithmetic.current is None
    with pytest.raises(ValueError):
        ops.eval_arithmetic("f16x2")
    with pytest.raises(ValueError):
        ops.arithmetic_scope("fp8")
    ops.set_gemm_precision("f16x3")
    with ops.eval_arithmetic("f16x1") as a:
        assert ops.eval_arithmetic.current is a and a.switched == 0
        with ops.eval_arithmetic("f16x3") as b:
            assert ops.eval_arithmetic.current is b
        assert ops.eval_arithmetic.current is a
    assert ops.eval_arithmetic.current is None
    with ops.arithmetic_scope(None) as n:
        assert n is None and ops.eval_arithmetic.current is None
    try:
        ops.set_gemm_precision("bf16x6")
        with pytest.raises(RuntimeError):
            with ops.eval_arithmetic("f16x1"):
                pass
        assert ops.eval_arithmetic.current is None
        with ops.eval_arithmetic("f16x3"):
            pass
    finally:
        ops.set_gemm_precision("f16x3")


def test_autograd_is_seen_through_a_function_s_forward():
    """inside autograd.Function.forward grad mode is off whatever the caller's: the block must still tell a node autograd records
    from one it does not, and a backward pass from both"""
    from npvp_amd import ops
    seen = []

    class Probe(ops._Function):
        @staticmethod
        def forward(ctx, x):
            seen.append(("fwd", torch.is_grad_enabled(), ops._autograd_off()))
            return x * 2

        @staticmethod
        def backward(ctx, g):
            seen.append(("bwd", torch.is_grad_enabled(), ops._autograd_off()))
            return g * 2

    x = torch.ones(4, requires_grad=True)
    with ops.eval_arithmetic("f16x3"):
        y = Probe.apply(x)
        with torch.no_grad():
            Probe.apply(x)
            assert ops._autograd_off()
        assert not ops._autograd_off()
        y.sum().backward()
    assert seen == [("fwd", False, False), ("fwd", False, True), ("bwd", False, False)]
    assert ops._Function._recording == 0


def test_r11_is_scaled_fp16_rounding_and_costs_what_the_bars_assume():
    g = torch.Generator().manual_seed(0)
    for M, K, N in ((256, 32, 256), (256, 512, 256)):
        A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
        for t in (A, W):
            s = 2.0 ** (14 - math.floor(math.log2(float(t.abs().max()))))
            assert torch.equal((t.double() * s).half().double() / s, X.r11(t)), "r11 is not amax-scaled fp16 rounding"
        ex = A.double() @ W.double().T
        rd = X.r11(A) @ X.r11(W).T
        e = X.rel(rd, ex)
        rows = (rd - ex).norm(dim=1) / ex.norm(dim=1)
        assert abs(e - X.ONE_TERM_REL) < 0.3e-4, e
        assert X.FLOOR < float(rows.min()) and float(rows.max()) < X.CEIL
    x = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -60 * (1 + 2.0 ** -10), -3.0])
    assert X.r11(x).tolist() == [1.0, 1.0 + 2.0 ** -9, 2.0 ** -60 * (1 + 2.0 ** -10), -3.0], "ties go to even, no exponent limit"


def test_the_emulation_on_the_small_predictor():
    """the float64 oracle with every GEMM of 128 token rows or more rounded: the deviation lies in [3e-4, 3e-3] (measured 8.97e-4,
    71 rounded GEMMs), and the patch is gone afterwards"""
    import oracle
    from oracle import ops as O
    import torch.nn.functional as F
    lin0, conv0 = F.linear, F.conv2d
    N, To = 2, 3
    m = GC._small_predictor(oracle, True, 91, "cpu").eval().double()
    past = O.synth_features((N, To, 512, 8, 8), 92).double()
    eps = O.seeded_randn((N, 512, 8, 8), 94).double()
    m.evt_prior.eps_fn = lambda shape: eps
    e, y0, y1, count = X.emulated_deviation(m, lambda mod: mod(past))
    print(f"emulated f16x1 deviation {e:.3e} over {count} rounded GEMMs")
    assert F.linear is lin0 and F.conv2d is conv0
    assert count >= 50, count
    assert X.EMU_LO <= e <= X.EMU_HI, e
    with torch.no_grad():
        assert torch.equal(m(past), y0), "the model is not back to its own arithmetic"
