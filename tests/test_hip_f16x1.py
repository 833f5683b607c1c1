"""GPU: the one-term fp16 arithmetic ("f16x1": ops.eval_arithmetic, precision 7 of npvp_gemm_f32) on every kernel it has.

The reference of a launch is the fp64 product of the r11-ROUNDED operands (tests/f16x1_cases.py): what is left between it and the
kernel is fp32 accumulation, so the bars are the suite's own - whole tensor TOL["f16x3"] = 1e-5, worst row ROW_TOL -, c_amax is exact
and every padding intact (padded views with NaN / bit-pattern borders, as tests/test_hip_gemm_routes.py).  Against the UNROUNDED fp64
product a launch must lie in [1e-4, 1e-3] (3 x either side of the 2.9e-4 that 11-bit operands cost): a two-term result, at <= 1e-5,
fails the floor, so every case fails on a library that runs precision 7 as precision 6.  The route of every launch is asserted at run
time, and so is that the block switched it.

  1. every f16x3 forward / dgrad case of the route table on ids 5 / 7, six epilogues each;
  2. the frame-statistics cases of the table;
  3. K = 32 {1..8, 13} per tile variant at one ragged shape each: the prologue alone, every tail of the two-stage pair loop and of the
     three-stage period-6 loop, two full rounds;
  4. the row guard's second pass: half the rows 2^-20 below the others;
  5. Predictor.sample(arithmetic=...): None is the call as it was, f16x1 against the CPU oracle inside the bracket the emulation
     gives, the switched-launch counter, and a training step inside the block equal to the bit to one outside."""
import contextlib
import ctypes
import math

import pytest
import torch

import f16x1_cases as X
import gemm_route_cases as T
import golden_cases as GC
from oracle import ops as O
from test_hip_gemm_routes import PAD_C, PATTERN, Buf, gelu64, vec
from test_hip_ops import DEV, close

pytestmark = pytest.mark.gpu

TOL = T.TOL["f16x3"]
ONE_TERM_CASES = [c for c in T.CASES if c["mode"] == "f16x3" and c["role"] != "wgrad" and c["route"][0] in (5, 7) and not c.get("rowstats")]
STAT_CASES = [c for c in T.CASES if c["mode"] == "f16x3" and c.get("rowstats")]


def ids(cs):
    return [c["name"] for c in cs]


@pytest.fixture
def ops():
    import npvp_amd  # noqa: F401
    from npvp_amd import ops as o
    assert torch.cuda.is_available()
    dev = torch.device(DEV)
    o.set_gemm_precision("f16x3")
    o.rng.manual_seed(1234, dev)
    o.rng.begin_step(dev)
    return o


def route7(a_kc, b_kc, M, N, K, planes, plain):
    from npvp_amd._lib import lib
    out = (ctypes.c_int * 4)()
    assert lib().npvp_gemm_route(a_kc, b_kc, M, N, K, 7, int(planes), int(plain), ctypes.addressof(out)) == 0
    return tuple(out)


def one_term_gemm(ops, a_kc, b_kc, M, N, K, A, W, C, pl, expect_route, plain, **kw):
    """one ops.gemm under no_grad inside eval_arithmetic("f16x1"): the route is the one named, and the block switched the launch"""
    r = route7(a_kc, b_kc, M, N, K, pl is not None, plain)
    assert r == expect_route + (1, K // 32), f"route {r}, expected {expect_route} with one split of {K // 32} K-steps"
    with torch.no_grad(), ops.eval_arithmetic("f16x1") as ar:
        ops.gemm(a_kc, b_kc, M, N, K, A.v, A.v.stride(0), W.v, W.v.stride(0), C.v, b_pre=pl, **kw)
    assert ar.switched == 1, "the launch was not made in the one-term arithmetic"


def in_one_term_band(got, exact, what):
    e = X.rel(got, exact)
    print(f"{what}: rel-L2 against the unrounded product {e:.3e}")
    assert X.FLOOR <= e <= X.CEIL, f"{what}: {e:.3e} against the unrounded product is outside [{X.FLOOR:.0e}, {X.CEIL:.0e}]"
    return e


def operands(ops, role, M, N, K, seed, a_shift=0.0):
    """A [M, K] and the weight as padded views, the weight's fp16 planes, the exact and the r11-rounded fp64 products"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    A = Buf(M, K, torch.randn(M, K, device=DEV, generator=g) + a_shift, extra_ld=4)
    if role == "fwd":
        W = Buf(N, K, torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K))
        exact, ref = A.v.double() @ W.v.double().T, X.r11(A.v) @ X.r11(W.v).T
    else:
        W = Buf(K, N, torch.randn(K, N, device=DEV, generator=g) / math.sqrt(K), extra_ld=8)
        exact, ref = A.v.double() @ W.v.double(), X.r11(A.v) @ X.r11(W.v)
    pl = ops.WeightPlanes.get(W.v, "F" if role == "fwd" else "D")
    assert pl is not None
    return A, W, pl, exact, ref, g


# ------------------------------------------------------------------------------- 1. every leaf and epilogue
@pytest.mark.parametrize("case", ONE_TERM_CASES, ids=ids(ONE_TERM_CASES))
def test_every_leaf_and_epilogue(ops, case):
    M, N, K = case["M"], case["N"], case["K"]
    a_kc, b_kc = T.ROLES[case["role"]]
    A, W, pl, exact, ref, g = operands(ops, case["role"], M, N, K, 11)
    C = Buf(M, N, fill="pattern")
    name = f"f16x1 {case['leaf']} | {case['name']}"

    def run(what, expect, plain=False, keep_c=False, **kw):
        if not keep_c:
            C.base.view(torch.int32).fill_(PATTERN)
        one_term_gemm(ops, a_kc, b_kc, M, N, K, A, W, C, pl, case["route"][:2], plain, **kw)
        assert bool(torch.isfinite(C.v).all()), f"{what}: a non-finite result - an operand was read outside its extent"
        close(C.v, expect, tol=TOL, what=f"{name} | {what}")
        assert C.padding_intact(), f"{what}: the launch wrote outside C[:M, :N]"

    slot = ops.AmaxSlot.new(torch.device(DEV))
    run("plain", ref, plain=True, c_amax=slot)
    assert slot.read() == float(C.v.abs().max()), "c_amax is not max|C| over the valid region"
    in_one_term_band(C.v, exact, name)
    bias = vec(N, torch.randn(N, device=DEV, generator=g))
    run("bias alpha=0.5", 0.5 * ref + bias.double(), bias=bias, alpha=0.5)
    pre = ref + bias.double()
    aux = Buf(M, N, fill="pattern")
    run("gelu", gelu64(pre), bias=bias, act=1, aux_out=aux.v)
    close(aux.v, pre, tol=TOL, what=f"{name} | aux_out")
    assert aux.padding_intact(), "aux_out: the launch wrote outside [:M, :N]"
    res = Buf(M, N, torch.randn(M, N, device=DEV, generator=g), extra_ld=12)
    run("relu+residual", torch.relu(pre) + res.v.double(), bias=bias, act=2, residual=res.v)
    c0 = torch.randn(M, N, device=DEV, generator=g)
    C.fill(c0)
    run("accumulate", c0.double() + ref, accumulate=True, keep_c=True)
    d = ops.Drop(0.25)
    mask = ops.drop_apply(torch.ones(M, N, device=DEV), d)
    run("dropout", ref * mask.double(), drop=d)
    assert torch.equal(C.v != 0, mask != 0), "the kept pattern is not drop_apply's for the same site"


# ------------------------------------------------------------------------------- 2. frame statistics
@pytest.mark.parametrize("case", STAT_CASES, ids=ids(STAT_CASES))
def test_frame_statistics(ops, case):
    from npvp_amd._lib import lib, check
    M, N, K = case["M"], case["N"], case["K"]
    A, W, pl, exact, ref, g = operands(ops, "fwd", M, N, K, 21, a_shift=0.5)
    bias = vec(N, torch.randn(N, device=DEV, generator=g) + 2.0)
    C = Buf(M, N, fill="pattern")
    frames = M // 64
    part = Buf(1, frames * (N // 64) * 2, fill="pattern")
    slot = ops.AmaxSlot.new(torch.device(DEV))
    one_term_gemm(ops, 1, 1, M, N, K, A, W, C, pl, case["route"][:2], False, bias=bias, rowstats=part.v, c_amax=slot)
    mean = torch.empty(frames, dtype=torch.float32, device=DEV)
    rstd = torch.empty_like(mean)
    check(lib().npvp_frame_stats_finalize(part.v.data_ptr(), N // 64, 4096.0, mean.data_ptr(), rstd.data_ptr(), frames, 1e-5,
                                          torch.cuda.current_stream().cuda_stream), "npvp_frame_stats_finalize")
    name = f"f16x1 {case['leaf']} | {case['name']}"
    assert bool(torch.isfinite(C.v).all())
    close(C.v, ref + bias.double(), tol=TOL, what=f"{name} | output")
    in_one_term_band(C.v.double() - bias.double(), exact, name)
    assert C.padding_intact() and part.padding_intact(), "the launch wrote outside C or outside the statistics partials"
    assert slot.read() == float(C.v.abs().max())
    fr = C.v.double().reshape(frames, -1)
    close(mean, fr.mean(1).float(), tol=T.MEAN_TOL, what=f"{name} | mean")
    close(rstd, (1.0 / torch.sqrt(fr.var(1, unbiased=False) + 1e-5)).float(), tol=T.RSTD_TOL, what=f"{name} | rstd")


# ------------------------------------------------------------------------------- 3. K-step sweep per tile variant
SWEEP = {1: (136, 264), 4: (192, 128), 3: (132, 128), 2: (2052, 1024)}       # variant -> ragged M x N (gemm_f16_variant's text)
K_STEPS = (1, 2, 3, 4, 5, 6, 7, 8, 13)


@pytest.mark.parametrize("variant", sorted(SWEEP))
def test_k_step_sweep(ops, variant):
    M, N = SWEEP[variant]
    worst = 0.0
    for steps in K_STEPS:
        K = 32 * steps
        role = "dgrad" if steps % 2 == 0 else "fwd"
        a_kc, b_kc = T.ROLES[role]
        A, W, pl, exact, ref, g = operands(ops, role, M, N, K, 100 + steps)
        C = Buf(M, N, fill="pattern")
        slot = ops.AmaxSlot.new(torch.device(DEV))
        one_term_gemm(ops, a_kc, b_kc, M, N, K, A, W, C, pl, (5 if variant == 1 else 7, variant), True, c_amax=slot)
        name = f"f16x1 variant {variant} | {role} {M}x{N}x{K}"
        assert bool(torch.isfinite(C.v).all()), name
        close(C.v, ref, tol=TOL, what=name)
        assert C.padding_intact(), name
        assert slot.read() == float(C.v.abs().max()), name
        in_one_term_band(C.v, exact, name)
        worst = max(worst, X.rel(C.v, ref))
    print(f"variant {variant}: worst rel-L2 against the rounded product {worst:.3e}")


# ------------------------------------------------------------------------------- 4. the row guard's second pass
@pytest.mark.parametrize("N,route", [(264, (5, 1)), (128, (7, 4))], ids=["two stages", "three stages"])
def test_row_guard_second_pass(ops, N, route):
    """every other row 2^-20 below the tensor's bound: scaled by the tensor's amax alone such a row's elements are fp16 subnormals and
    lose bits; the second pass scales each row by its own maximum, and r11 has no exponent limit - the small rows must match it"""
    M, K = 256, 64
    g = torch.Generator(device=DEV).manual_seed(71)
    a = torch.randn(M, K, device=DEV, generator=g)
    a[1::2] *= 2.0 ** -20
    A = Buf(M, K, a, extra_ld=4)
    W = Buf(N, K, torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K))
    pl = ops.WeightPlanes.get(W.v, "F")
    exact, ref = A.v.double() @ W.v.double().T, X.r11(A.v) @ X.r11(W.v).T
    C = Buf(M, N, fill="pattern")
    one_term_gemm(ops, 1, 1, M, N, K, A, W, C, pl, route, True)
    name = f"f16x1 row guard | 256x{N}x64"
    close(C.v, ref, tol=TOL, what=name, row_floor=0.0)
    assert C.padding_intact()
    rows = (C.v.double() - exact).norm(dim=1) / exact.norm(dim=1)
    print(f"{name}: per-row rel-L2 against the unrounded product {float(rows.min()):.3e} .. {float(rows.max()):.3e}")
    assert X.FLOOR <= float(rows.min()) and float(rows.max()) <= X.CEIL, "a row does not carry 11-bit operands"


# ------------------------------------------------------------------------------- 5. the sampler
N_, TO, TP, S_ = 2, 3, 4, 3


def _oracle_layout(eps_s):
    """[N, H*W, C] canonical -> the reference's (N, C, H, W)"""
    return eps_s.transpose(1, 2).reshape(eps_s.shape[0], 512, 8, 8).contiguous()


@pytest.fixture(scope="module")
def sampler():
    import npvp_amd
    from npvp_amd import ops as o
    o.set_gemm_precision("f16x3")
    o.rng.manual_seed(1234, torch.device(DEV))
    m = GC._small_predictor(npvp_amd, True, 91, DEV).eval()
    past = O.synth_features((N_, TO, 512, 8, 8), 92)
    return m, past


def test_arithmetic_none_is_the_call_as_it_was(ops, sampler):
    import npvp_amd
    m, past = sampler
    p = past.to(DEV)
    plain, eps = m.sample(p, S_, seed=4321, return_eps=True)
    with ops.eval_arithmetic("f16x3") as outer:
        none, eps_n = m.sample(p, S_, seed=4321, return_eps=True, arithmetic=None)
        named, _ = m.sample(p, S_, seed=4321, return_eps=True, arithmetic="f16x3")
    assert torch.equal(none, plain) and torch.equal(eps_n, eps) and torch.equal(named, plain)
    assert outer.switched == 0
    assert torch.equal(npvp_amd.predictor_sample_step(m, p, S_, seed=4321, arithmetic=None), plain)
    with pytest.raises(ValueError):
        m.sample(p, 1, arithmetic="f16")
    with pytest.raises(ValueError):
        npvp_amd.predictor_sample_step(m, p, 1, arithmetic="f16")
    assert ops.eval_arithmetic.current is None and not m.training


def test_sample_f16x1_against_the_oracle(ops, sampler):
    """per sample against the unpatched CPU oracle fed the returned eps: at most 2 x e_emu (fp32 activations, and the GEMMs below 256
    token rows that stay two-term on the device while the emulation rounds from 128 rows on) and at least e_emu / 3, e_emu being the
    emulation's own deviation on the float64 oracle - a reference-side number"""
    import npvp_amd
    import oracle
    m, past = sampler
    p = past.to(DEV)
    with ops.eval_arithmetic("f16x1") as ar:
        out, eps = m.sample(p, S_, seed=4321, return_eps=True, arithmetic="f16x1")
        assert ar.switched == 0, "the entry point's own block counts its launches"
    plain, eps3 = m.sample(p, S_, seed=4321, return_eps=True)
    assert torch.equal(eps, eps3) and not torch.equal(out, plain)
    with ops.eval_arithmetic("f16x1") as ar:
        step = npvp_amd.predictor_sample_step(m, p, S_, seed=4321)
        n_sample = ar.switched
        with torch.no_grad():
            m(p)
        n_forward = ar.switched - n_sample
    assert n_sample > 0 and n_forward > 0, "the counter counts the switched launches of sample() and of forward under no_grad"
    assert torch.equal(step, out), "the block around the call and arithmetic='f16x1' are the same thing"

    ref = GC._small_predictor(oracle, True, 91, "cpu").eval()
    ref64 = GC._small_predictor(oracle, True, 91, "cpu").eval().double()
    e0 = _oracle_layout(eps[0].cpu())
    ref64.evt_prior.eps_fn = lambda shape: e0.double()
    e_emu, _, y_emu, count = X.emulated_deviation(ref64, lambda mod: mod(past.double()))
    assert X.EMU_LO <= e_emu <= X.EMU_HI and count >= 50, (e_emu, count)
    print(f"e_emu {e_emu:.3e} over {count} rounded GEMMs; switched launches: sample {n_sample}, forward {n_forward}")
    for s in range(S_):
        e_s = _oracle_layout(eps[s].cpu())
        ref.evt_prior.eps_fn = lambda shape: e_s
        with torch.no_grad():
            want = ref(past)
        e = GC.rel_err(out[:, s], want)
        e3 = GC.rel_err(plain[:, s], want)
        extra = f", against the emulated oracle {GC.rel_err(out[:, s], y_emu):.3e}" if s == 0 else ""
        print(f"sample {s}: f16x1 rel-L2 against the oracle {e:.3e} (f16x3: {e3:.3e}){extra}")
        assert e_emu / 3 <= e <= 2 * e_emu, f"sample {s}: {e:.3e} outside [{e_emu / 3:.3e}, {2 * e_emu:.3e}]"


def test_a_training_step_inside_the_block_is_untouched(ops):
    """forward launches of a differentiated node and every backward launch run with grad mode off, too: none may be switched"""
    import npvp_amd
    dev = torch.device(DEV)
    past = O.synth_features((N_, TO, 512, 8, 8), 92).to(DEV)
    fut = O.synth_features((N_, TP, 512, 8, 8), 93).to(DEV)
    eps = O.seeded_randn((N_, 512, 8, 8), 94).to(DEV)

    def step(block):
        m = GC._small_predictor(npvp_amd, True, 101, DEV)
        m.evt_prior.eps_fn = m.evt_posterior.eps_fn = lambda shape: eps
        m.train()
        opt = npvp_amd.FlatAdamW(m, lr=1e-4, clip_module=m.transformer)
        ops.rng.manual_seed(1234, dev)
        with block as ar:
            r = npvp_amd.predictor_train_step(m, opt, past, fut, 0.01, 1e-6, 1.0, sync=False)
            switched = None if ar is None else ar.switched
        torch.cuda.synchronize()
        return r["loss"].clone(), opt.flat_g.clone(), opt.flat_p.clone(), switched

    loss_o, g_o, p_o, _ = step(contextlib.nullcontext())
    loss_i, g_i, p_i, switched = step(ops.eval_arithmetic("f16x1"))
    assert switched == 0, f"{switched} launches of a training step were switched"
    assert torch.equal(loss_i, loss_o) and torch.equal(g_i, g_o) and torch.equal(p_i, p_o)
    assert float(g_o.abs().max()) > 0
