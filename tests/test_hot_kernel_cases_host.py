"""CPU: the cases of tests/test_hip_hot_kernels.py can see what they claim to see (tests/hot_kernel_cases.py).

  * every mutant of a family - a deliberately wrong float64 reference - is rejected by the GPU test's own comparison at >= 10 x the
    bound (or as a non-finite value) in at least one case of the family;
  * the fp32 CPU oracle passes every case and every output at bound / 4: a condition on the INPUTS, so that the bound is not inside
    the reference's own arithmetic noise;
  * the tables take both sides of every predicate the launchers branch on (the library's pure functions, no device)."""
import pytest
import torch

import hot_kernel_cases as HK
from oracle import ops as O


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    build.build(verbose=False)
    from npvp_amd._lib import lib
    return lib()


@pytest.mark.parametrize("family,mutant", [(f, m) for f in HK.MUTANTS for m in HK.MUTANTS[f]])
def test_a_wrong_reference_is_rejected(family, mutant):
    seen = []
    for case in HK.CASES[family]:
        w = HK.worst(HK.reference(family, case, torch.float64, mutant), HK.ref64(family, case))
        seen.append((HK.case_id(case), f"{w:.2e}"))
        if w >= 10 * HK.BOUND:
            return
    pytest.fail(f"{family}: no case puts the mutant '{mutant}' at 10 x the bound: {seen}")


@pytest.mark.parametrize("family", list(HK.CASES))
def test_the_fp32_oracle_is_well_inside_the_bound(family):
    bad = []
    for case in HK.CASES[family]:
        ref, f32 = HK.ref64(family, case), HK.ref32(family, case)
        for k in ref:
            if k.startswith("_"):
                continue
            e = HK.err_of(k, f32, ref)
            print(f"{family}[{HK.case_id(case)}] {k} fp32-cpu {e:.3e}")
            if not e <= HK.BOUND / 4:
                bad.append((HK.case_id(case), k, f"{e:.2e}"))
    assert not bad, bad


def test_the_fp32_oracle_on_the_layernorm_pair():
    assert HK.worst(HK.layernorm_res_reference(torch.float32), HK.layernorm_res_reference(torch.float64)) <= HK.BOUND / 4


def test_the_inputs_the_kernels_are_given_are_those_of_the_reference():
    """part1 (the fc1 GEMM's row statistics, built on the CPU) merges to the frame's statistics; a planted score is 100"""
    for case in HK.MID_FWD:
        i = HK.mid_inputs("mid_fwd", case)
        mu, rs = HK.chan_merge(HK.mid_part1(i), 4096.0)
        ref = HK.ref64("mid_fwd", case)
        assert HK.sigma_err(mu, ref["mean1"], ref["rstd1"]) < 1e-6 and HK.rel(rs, ref["rstd1"]) < 1e-6
    N, Tq, Tk, mask, plant = case = HK.ATTN_T[1]
    i = HK.attn_t_inputs(case, torch.float64)
    q, k = i["q"].detach(), i["k"].detach()
    s = lambda tq, tk, p, h: float(q[tq * 64 + p, 64 * h:64 * h + 64] @ k[tk * 64 + p, 64 * h:64 * h + 64]) / 8.0
    assert abs(s(1, plant, 5, 2) - HK.PLANTED) < 1e-3 and abs(s(0, Tk - 1, 9, 4) - HK.PLANTED) < 1e-3
    assert bool(O.encoder_temporal_mask(Tq)[0, Tk - 1])
    scores = (q[:64, :64] @ k[:64, :64].t()) / 8.0                      # (any unplanted block: sigma WIDE_Q)
    assert 0.85 * HK.WIDE_Q < float(scores.std()) < 1.15 * HK.WIDE_Q


def both(values):
    return set(bool(v) for v in values) == {False, True}


def test_the_tables_take_both_sides_of_every_route(L):
    # the fused middle's chunks: one per frame below 128 frames, 128 chunks at 128, chunks of unequal length at 129
    chunks = {f: HK.mid_chunks(L, f, ch) for (f, ch, _) in HK.MID_BWD}
    assert chunks[127] == (1, 127) and chunks[128] == (1, 128) and chunks[129] == (2, 65) and 129 % 2 == 1
    assert all(ch % 512 == 0 for (_, ch, _) in HK.MID_FWD + HK.MID_BWD)
    assert {ch // 512 for (_, ch, _) in HK.MID_FWD} == {1, 3, 4} and {f for (f, _, _) in HK.MID_FWD} == {1, 3}
    assert {k for (*_, k) in HK.MID_FWD} == {"plain", "flat", "shift", "chan"}
    assert {n for (*_, n) in HK.MID_N2} >= {1, 256} and both(p > 0 for (_, _, p, _) in HK.MID_N2)
    assert all(n in (1, ch // 16) and n <= 256 for (_, ch, _, n) in HK.MID_N2)
    # depthwise weight gradient: 255 | 256 | 257 frames, a last block with one live quad, a half-empty block, two blocks
    dw = {f: HK.G.dwconv_chunks(L, f, ch) for (f, ch, _) in HK.DW_WGRAD}
    assert dw[255] == (1, 255) and dw[256] == (1, 256) and dw[257] == (2, 129)
    assert {ch for (_, ch, _) in HK.DW_WGRAD} == {260, 512, 1536} and both(ch % 1024 == 0 for (_, ch, _) in HK.DW_FWD + HK.DW_STATS)
    assert all(ch % 1024 == 0 for (_, ch, _) in HK.DW_STATS) and {k for (*_, k) in HK.DW_STATS} == {"shift", "chan", "flat"}
    # posfuse at per_frame = 32768: the fused and the unfused backward
    assert both(L.npvp_posfuse_bwd_fused(n, t, 64 * 512) for (n, t, *_) in HK.POSFUSE)
    assert {k for (*_, k) in HK.POSFUSE} == {"plain", "flat", "shift", "lead"}
    assert {c for (_, c, *_) in HK.LAYERNORM} == {512} and {c for (_, c, *_) in HK.LAYERNORM_NCHW} == {256, 512}
    assert both(r for (_, _, r, _) in HK.LAYERNORM_NCHW) and both(r for (_, _, r, _) in HK.LAYERNORM)
    # attention: each route of the P = 64 dispatch, masked and not; the streaming winner in the first and in the last key tile
    assert {(tq, tk) for (_, tq, tk, *_) in HK.ATTN_T} == {(10, 10), (18, 18), (28, 2), (40, 40), (129, 129)}
    assert all(both(m for (_, tq, _, m, _) in HK.ATTN_T if tq == t) for t in (10, 18, 40, 129))
    assert {pl // 16 for (_, tq, _, m, pl) in HK.ATTN_T if tq == 129 and not m} == {0, 8}
    assert {ws for (_, ws, _) in HK.ATTN_S} == {4, 8}
    # non-local attention at (8, 32): key tiles of 64 - the 72 keys of 18 x 16 are a full and a partial tile, a winner in each
    from npvp_amd import ops
    assert all(ops.nonlocal_attn_config_shape(a, 4 * a, h, w) == (r == "config") for (r, a, _, h, w, _) in HK.ATTN_NL)
    assert {pl // 64 for (r, a, _, h, w, pl) in HK.ATTN_NL if (h // 2) * (w // 2) > 64} == {0, 1}
    assert min(a for (_, a, *_) in HK.ATTN_NL) == min(ops._NL_GRID) and any((h, w) == (4, 4) for (_, _, _, h, w, _) in HK.ATTN_NL)
