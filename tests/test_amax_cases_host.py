"""CPU: the case tables of tests/amax_cases.py plant what they claim.  For every producer case without dropout the float64 oracle's
output has its |max| at the planted element and every other element below half of it; every producer's table covers each planted
position it has a region for; every `second_trip` case is larger than its launcher's grid cap (restated in amax_cases.CAPS) and its
planted element lies beyond the first trip."""
import pytest
import torch

import amax_cases as A

PLAIN = [c for c in A.all_cases() if not A.has_dropout(c)]


@pytest.mark.parametrize("case", PLAIN, ids=A.case_id)
def test_the_planted_element_is_the_maximum_by_a_factor_of_two(case):
    i, ref = A.build(case)
    assert i["at"], "no planted output"
    for name, at in i["at"].items():
        m, idx, rest = A.planted_ok(ref[name], at)
        assert idx == at, f"{name}: |max| {m} at {idx}, planted at {at}"
        assert rest < m / 2, f"{name}: the second largest value {rest} is not below half of {m}"
        assert m < 6.0e4, "the planted maximum stays a plausible activation (inside fp16's range before scaling)"


def test_dropout_cases_plant_at_an_element_the_masks_keep():
    """with a synthetic keep pattern (every third element dropped, every second sample dropped) the builders move the planted element to
    a kept one and the oracle's maximum is there"""
    for case in A.all_cases():
        if not A.has_dropout(case):
            continue
        if case["producer"] == "drop_apply":
            n = case["rows"] * case["cols"]
            keep = ((torch.arange(n) % 3) != 0).float().reshape(case["rows"], case["cols"]) / (1 - A.DROP_P)
        elif case["producer"] in ("attn_fwd", "attn_bwd"):
            sh = A.attn_keep_shape(case)
            n = sh[0] * sh[1] * sh[2] * sh[3]
            keep = ((torch.arange(n) % 3) != 1).float().reshape(sh) / (1 - A.ATTN_DROP_P)
        elif case["producer"] == "gemm":
            rc = A._route_case(case["shape"])
            M, N = rc["M"], rc["N"]
            if case["ep"] == "dropout":
                keep = ((torch.arange(M * N) % 3) != 2).float().reshape(M, N) / (1 - A.GEMM_DROP_P)
            else:
                keep = (((torch.arange(M) // A.GEMM_DP_G1) % 2) == 0).float().reshape(M, 1).expand(M, N) / (1 - A.GEMM_DROP_P)
        else:
            frames, pf = case["frames"], case["pf"]
            keep = dict(drop=((torch.arange(frames * pf) % 3) != 1).float().reshape(frames, pf) / (1 - A.FLN_DROP_P) if case["drop"] else None,
                        dp=(((torch.arange(frames) // A.FLN_FRAMES_PER_SAMPLE) % 2) == 0).float() / (1 - A.FLN_DP_P) if case["dp"] else None)
        i, ref = A.build(case, keep)
        for name, at in i["at"].items():
            m, idx, rest = A.planted_ok(ref[name], at)
            assert idx == at and rest < m / 2, (case["id"], name, m, idx, at, rest)


@pytest.mark.parametrize("producer", sorted(A.PRODUCERS))
def test_every_position_of_a_producer_is_in_its_table(producer):
    table = A.PRODUCERS[producer][0]
    assert all(c["producer"] == producer for c in table)
    have = {c["pos"] for c in table}
    assert set(A.REQUIRED[producer]) <= have, f"{producer}: no case for {sorted(set(A.REQUIRED[producer]) - have)}"
    assert have <= set(A.POSITIONS)
    assert len({c["id"] for c in table}) == len(table), "case ids must be unique"


def test_required_operands_are_planted_through():
    """the operand a kernel is most likely to leave out of its bound carries the maximum in at least one case"""
    via = {(c["producer"], c.get("via")) for c in A.all_cases()}
    for want in (("layernorm_bwd", "dres"), ("layernorm_bwd", "dy"), ("grid_center_cut", "addend"), ("posfuse_fwd", "beta"),
                 ("ln_posfuse_fwd", "beta"), ("ln_posfuse_fwd", "x"), ("frameln_act_fwd", "res"), ("frameln_act_fwd", "h")):
        assert want in via, want
    assert {c["C"] for c in A.LAYERNORM_FWD} == {256, 1024} == {c["C"] for c in A.LAYERNORM_BWD}
    assert {c["relu"] for c in A.LAYERNORM_FWD} == {0, 1} and {c["dres"] for c in A.LAYERNORM_BWD} == {0, 1}
    assert any(c["rows"] % 4 for c in A.LAYERNORM_FWD) and any(c["rows"] % 4 for c in A.LAYERNORM_BWD)
    assert {c["pf"] == 32768 for c in A.POSFUSE} == {True, False}, "both launch paths of npvp_posfuse_fwd (csrc/norm.hip:993)"
    assert all(c["P"] == 60 for c in A.POSFUSE_INSTANCE) and any(c["C"] % 256 for c in A.POSFUSE_INSTANCE)
    assert all((c["pf"] // 4) % 256 != 0 and c["pf"] % 16 == 0 for c in A.FRAMELN_BWD), "some threads take the early-commit branch"
    assert {(c["drop"], c["dp"]) for c in A.FRAMELN_FWD} >= {(0, 0), (1, 0), (0, 1)}
    assert {c["mode"] for c in A.DROP_APPLY} == {0, 1}
    assert {c["ld"] > c["cols"] for c in A.AMAX} == {True, False}
    assert len(A.SPLIT_RECORDS) == 3
    assert {(c["kid"], c["ep"]) for c in A.GEMM} >= {(k, e) for k in (0, 1, 2, 4, 5, 7) for e in A.GEMM_EPILOGUES}
    assert {c["ep"] for c in A.GEMM} >= {"rowstats", "split", "split_accumulate"}
    for table, targets in ((A.ATTN_FWD, {"v"}), (A.ATTN_BWD, {"dq", "dk", "dv"})):
        for shape in A.ATTN_SHAPES:
            mine = [c for c in table if c["shape"] == shape]
            assert {c["via"] for c in mine} == targets and any(c["drop"] for c in mine), shape
    assert any(c["mask"] for c in A.ATTN_FWD) and any(c["mask"] for c in A.ATTN_BWD)


def test_attention_shapes_reach_the_kernels_they_name():
    """the launcher's conditions (csrc/attn.hip: nq = ceil(L / 16), nk = ceil(S / 16); nq > 2 or nk > 2 -> generic) restated per shape"""
    want = {"mfma11": (1, 1), "mfma12": (1, 2), "staged21": (2, 1), "staged22": (2, 2), "spatial4": (1, 1)}
    for name, (mode, dim0, P, W, ws, Tq, Tk, heads, long_) in A.ATTN_SHAPES.items():
        L, S = (ws * ws, ws * ws) if mode == 0 else (Tq, Tk)
        nq, nk = (L + 15) // 16, (S + 15) // 16
        if name in want:
            assert (nq, nk) == want[name] and not long_
        elif long_:
            assert L in (64, 65, 129) and (L > 64 or mode == 0)
        else:
            assert (nq > 2 or nk > 2) and 33 <= max(L, S) <= 128, name
        if mode == 1:
            assert (dim0 * P * heads) % 4 != 0, "temporal: groups * heads is no multiple of 4"
    assert {A.ATTN_SHAPES[n][4] for n in A.ATTN_SHAPES if A.ATTN_SHAPES[n][0] == 0} == {4, 8}
    assert any(max(sh[5], sh[6]) == 128 and sh[5] != sh[6] for sh in A.ATTN_SHAPES.values())


SECOND = [c for c in A.all_cases() if c["pos"] == "second_trip"]


@pytest.mark.parametrize("case", SECOND, ids=A.case_id)
def test_second_trip_cases_exceed_the_grid_cap(case):
    items, per_trip, width = A.trips(case)
    assert items > per_trip, f"{items} work items fit the capped grid's first trip of {per_trip}"
    if A.has_dropout(case):
        return                      # (the position depends on the device's mask; the GPU test checks the argmax)
    i, _ = A.build(case)
    (at,) = i["at"].values()
    assert at // width >= per_trip, f"planted work item {at // width} lies in the first trip of {per_trip}"


def test_caps_are_the_launchers():
    """the caps restated in amax_cases.CAPS are the numbers in the launchers' source"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "npvp_amd", "csrc")
    src = {n: open(os.path.join(csrc, n)).read() for n in ("norm.hip", "elementwise.hip", "gemm_f16.hip", "gridpad.hip")}
    assert f"nb > {A.CAPS['ln_fwd']['blocks']} ? {A.CAPS['ln_fwd']['blocks']} : nb" in src["norm.hip"]
    assert f"b > {A.CAPS['ln_bwd']['blocks']} ? {A.CAPS['ln_bwd']['blocks']} : b" in src["norm.hip"]
    for f in ("norm.hip", "elementwise.hip"):
        assert re.search(r"ew_blocks\(long long total, int threads\) \{[^}]*if \(b > %d\) b = %d;" % ((A.CAPS["ew_blocks"]["blocks"],) * 2), src[f])
    assert f"if (blocks > {A.CAPS['npvp_amax']['blocks']}) blocks = {A.CAPS['npvp_amax']['blocks']};" in src["gemm_f16.hip"]
    assert f"(n4 + 256 * 8 - 1) / (256 * 8)" in src["gemm_f16.hip"] and A.CAPS["npvp_amax"]["float4_per_block"] == 256 * 8
    assert f"weights_amax_kernel, dim3({A.CAPS['weights_amax']['blocks']}, count)" in src["gemm_f16.hip"]
    assert f"if (b > {A.CAPS['gridpad']['blocks']}) b = {A.CAPS['gridpad']['blocks']};" in src["gridpad.hip"]
