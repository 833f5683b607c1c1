"""CPU: the cases of tests/test_hip_helper_kernels.py can see what they claim to see (tests/helper_kernel_cases.py).

  * every mutant of a family - a deliberately wrong float64 reference - is rejected by the GPU test's own comparison at >= 10 x its
    bar in at least one case of the family;
  * the fp32 CPU restatement passes every case at a quarter of its bar: the bars are outside the reference's own arithmetic noise;
  * the AdamW restatement is torch.optim.AdamW (with clip_grad_norm_) in float64, the SSIM restatement is the oracle's;
  * the tables take both values of every predicate the launchers branch on, each computed from the case."""
import pytest
import torch

import helper_kernel_cases as H
from oracle import metrics as OM
from oracle import ops as O


@pytest.mark.parametrize("family,mutant", [(f, m) for f in H.MUTANTS for m in H.MUTANTS[f]])
def test_a_wrong_reference_is_rejected(family, mutant):
    seen = []
    for case in H.CASES[family]:
        if max(int(v) for v in case if isinstance(v, int)) > 2000000 and seen:
            continue                                       # (the largest cases repeat a small one's branch at a second sweep)
        w = H.worst_ratio(family, case, H.reference(family, case, torch.float64, mutant))
        seen.append((H.ids(case), f"{w:.2e}"))
        if w >= 10:
            return
    pytest.fail(f"{family}: no case puts the mutant '{mutant}' at 10 x its bar: {seen}")


@pytest.mark.parametrize("family", list(H.CASES))
def test_the_fp32_restatement_is_well_inside_the_bars(family):
    bad = []
    for case in H.CASES[family]:
        for (k, m, e, bar) in H.measure(family, H.ref32(family, case), H.ref64(family, case), H.floors(family, case)):
            print(f"{H.label(family, case)} {k} {m} fp32-cpu {e:.3e}")
            if not H.ratio(e, bar) <= 0.25:
                bad.append((H.ids(case), k, m, f"{e:.2e}"))
    assert not bad, bad


def test_the_adamw_restatement_is_torch_adamw_with_clip_grad_norm():
    """three steps from zero state in float64: clip_grad_norm_ on a slice of the parameters, then torch.optim.AdamW - against
    clip_reference's coefficient formula and adamw_formula on the flat vector, to 1e-12"""
    n, (b, e), max_norm, lr, wd, eps = 43, (7, 41), 0.5, H.f32(1e-2), H.f32(0.01), H.f32(1e-8)
    b1, b2 = H.f32(H.ADAMW_BETAS[0]), H.f32(H.ADAMW_BETAS[1])
    p0 = (0.1 * O.seeded_randn((n,), 1)).double()
    head, mid, tail = (torch.nn.Parameter(t.clone()) for t in (p0[:b], p0[b:e], p0[e:]))
    opt = torch.optim.AdamW([head, mid, tail], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    mask = H.adamw_mask(n, (b, e))
    for step in (1, 2, 3):
        g = O.seeded_randn((n,), 10 + step).double()
        head.grad, mid.grad, tail.grad = g[:b].clone(), g[b:e].clone(), g[e:].clone()
        norm = torch.nn.utils.clip_grad_norm_([mid], max_norm)
        opt.step()
        mine = torch.sqrt((g[b:e] ** 2).sum())
        assert abs(float(mine) - float(norm)) <= 1e-12 * float(norm)
        coef = H.clip_coef(mine, torch.tensor(max_norm, dtype=torch.float64))
        assert float(coef) < 1.0
        p, m, v = H.adamw_formula(p, torch.where(mask, g * coef, g), m, v, lr, float(step), b1, b2, eps, wd)
        want = torch.cat([head.data, mid.data, tail.data])
        assert float((p - want).abs().max()) <= 1e-12 * float(want.abs().max()), step


def test_the_ssim_restatement_is_the_oracle():
    """ssim_restated carries the mutants; without one it is oracle.metrics.ssim_per_image, in float64 and on fp32 input"""
    for case in H.SSIM:
        i = H.ssim_inputs(case)
        for dt, tol in ((torch.float64, 1e-13), (torch.float32, 1e-6)):
            a, b = i["a"].to(dt), i["b"].to(dt)
            assert H.rel(H.ssim_restated(a, b, case[0]), OM.ssim_per_image(a, b, case[0])) <= tol, (case, dt)
        assert i["taps"].dtype == torch.float32 and i["taps"].numel() == case[0]


def both(values):
    return set(bool(v) for v in values) == {False, True}


def test_the_tables_take_both_sides_of_every_route():
    all4 = {0, 1, 2, 3}
    # flat lengths: every n % 4, a tail-only length, one length above and one below each grid cap
    flat = [c[0] for c in H.ADAMW + H.CLIP + H.L1 + H.SUM]
    assert {n % 4 for n in flat} == all4
    for table in (H.ADAMW, H.CLIP, H.L1, H.SUM):
        assert any(c[0] < 4 for c in table) and any(c[0] > 4 and c[0] % 4 for c in table)          # tail only; float4s and a tail
    assert {c[0] % 4 for c in H.L1} == all4 == {c[0] % 4 for c in H.SUM}
    assert both(c[0] > H.ADAMW_SWEEP for c in H.ADAMW) and any(c[0] > H.ADAMW_SWEEP and c[0] % 4 for c in H.ADAMW)
    assert both(c[0] > H.LOSS_SWEEP for c in H.CLIP) and both(c[0] > H.LOSS_SWEEP for c in H.SUM)
    assert both(c[0] > H.LOSS_SWEEP for c in H.L1) and both(c[0] > 4096 * 256 * 4 for c in H.L1)          # forward cap, backward cap
    # AdamW: clip ranges at every alignment of either end, a range that ends in the tail, one that IS the tail, one element, none;
    # both values of write_back_grad; the decays and the eps asked for; a second call
    ranges = [(c[0], c[1]) for c in H.ADAMW if c[1] is not None]
    assert {b % 4 for _, (b, e) in ranges} == all4 == {e % 4 for _, (b, e) in ranges}
    assert all(0 <= b < e <= n for n, (b, e) in ranges)
    assert any(b < (n & ~3) < e < n for n, (b, e) in ranges), "a range that starts in the vector part and ends inside the tail"
    assert any(b == (n & ~3) and e == n for n, (b, e) in ranges) and any(e - b == 1 for _, (b, e) in ranges)
    assert any((b, e) == (0, n) for n, (b, e) in ranges) and any(c[1] is None for c in H.ADAMW)
    assert both(c[2] for c in H.ADAMW) and {c[3] for c in H.ADAMW} == {0.0, 0.01, 0.3} and {c[4] for c in H.ADAMW} == {1e-8, 1e-3}
    assert {c[5] for c in H.ADAMW} == {1, 2} and 0.2 < H.ADAMW_COEF < 0.4 and H.ADAMW_HYPER[0] == (1e-2, 3.0)
    # clip: the norm on either side of max_norm, and zero
    for case in H.CLIP:
        r = H.ref64("clip", case)
        assert (float(r["norm"]) > H.clip_inputs(case)["max_norm"]) == (case[1] in ("above", "small")), case
        assert (float(r["coef"]) == 1.0) == (case[1] in ("below", "zero")) and (float(r["norm"]) == 0.0) == (case[1] == "zero")
    assert {k for _, k in H.CLIP} >= {"above", "below", "zero"}
    # ties on every 7th element of the L1 pairs
    i = H.l1_inputs((1003,))
    assert bool((i["a"][::7] == i["b"][::7]).all()) and int((i["a"] == i["b"]).sum()) == len(range(0, 1003, 7))
    # reduce / broadcast over the middle axis: above and below the cap, accumulate on and off, a scale other than 1
    assert both(a * c // 4 > H.EW_SWEEP4 for (a, b, c, _) in H.MID) and both(acc for (*_, acc) in H.MID) and H.MID_SCALE != 1.0
    assert all(c % 4 == 0 for (_, _, c, _) in H.MID) and any(b == 1 for (_, b, _, _) in H.MID)
    # transpose: tiles that are full and ragged in either direction, more than one batch
    assert both(R % 32 for (_, R, C) in H.TRANSPOSE) and both(C % 32 for (_, R, C) in H.TRANSPOSE) and both(b > 1 for (b, _, _) in H.TRANSPOSE)
    # colsum: chunks fewer than the query reserves, a ragged last chunk, exact chunks; ld above N; fewer than 128 rows
    ch = [(r,) + H.colsum_chunks(r) for (r, *_) in H.COLSUM]
    assert both(used < wanted for (r, wanted, per, used) in ch) and both(r % per for (r, wanted, per, used) in ch)
    assert H.colsum_chunks(130) == (128, 2, 65) and H.colsum_chunks(1001) == (128, 8, 126) and H.colsum_chunks(100) == (100, 1, 100)
    assert both(ld > n for (_, n, ld, _) in H.COLSUM) and both(r < 128 for (r, *_) in H.COLSUM) and both(acc for (*_, acc) in H.COLSUM)
    assert all(n % 4 == 0 and ld % 4 == 0 for (_, n, ld, _) in H.COLSUM) and both(n // 4 > 256 for (_, n, _, _) in H.COLSUM)
    # depthwise table: C off a multiple of 256, one block and several, with and without a bias
    assert all(c % 256 for (c, _) in H.DWTB) and both(10 * c > 256 for (c, _) in H.DWTB) and both(hb for (_, hb) in H.DWTB)
    # drop_apply: above and below the cap, both keying modes, both probabilities
    assert both(r * (nc // 4) > H.EW_SWEEP4 for (r, nc, *_) in H.DROP) and {c[3] for c in H.DROP} == {0, 1} and {c[2] for c in H.DROP} == {0.1, 0.5}
    assert any(nc // 4 == 1025 for (_, nc, *_) in H.DROP) and all(nc % 4 == 0 for (_, nc, *_) in H.DROP)
    # bias_act: vector and scalar by shape and by alignment, in both layouts; every act with and without a residual; both caps
    for lay in (0, 1):
        assert both(H.bias_act_is_vector(c) for c in H.BIAS_ACT if c[0] == lay)
    assert both(c[2] % 4 for c in H.BIAS_ACT) and any(c[2] % 4 == 0 and c[6] for c in H.BIAS_ACT)
    assert {(c[4], c[5]) for c in H.BIAS_ACT} == {(a, r) for a in range(4) for r in (0, 1)}
    assert all(c[0] == 1 or c[2] == c[3] for c in H.BIAS_ACT)
    vec_n = [c[1] * c[2] for c in H.BIAS_ACT if H.bias_act_is_vector(c)]
    sca_n = [c[1] * c[2] for c in H.BIAS_ACT if not H.bias_act_is_vector(c)]
    assert max(vec_n) == 4 * H.AE_CAP + 1028 and min(vec_n) < 4 * H.AE_CAP and max(sca_n) == H.AE_CAP + 9 and min(sca_n) < H.AE_CAP
    assert both(n > H.AE_CAP for (n, _) in H.ACT_BWD) and {a for (_, a) in H.ACT_BWD} == {0, 1, 2, 3} and any(n == 1 for (n, _) in H.ACT_BWD)
    # sqdiff: blocks on the float4 path and on the scalar path, by shape, by the chunk's start and by alignment; the 256-chunk cap
    blocks = {c: [H.sqdiff_block_is_vector(c[1], n, j, c[4]) for n in range(c[0]) for j in range(H.sqdiff_chunks(c[1])[0])] for c in H.SQDIFF}
    assert H.sqdiff_chunks(16388) == (2, 8194) and blocks[(2, 16388, 1.0, "one", 0)] == [True, False, True, False]
    assert H.sqdiff_chunks(4200004) == (256, 16407) and -(-4200004 // 16384) > 256 and both(blocks[(2, 4200004, 255.0, "mean", 0)])
    assert not any(blocks[(2, 1004, 1.0, "one", 1)]) and all(blocks[(2, 1004, 255.0, "mean", 0)])          # misaligned / aligned
    assert {c[2] for c in H.SQDIFF} == {1.0, 255.0} and {c[3] for c in H.SQDIFF} == {"mean", "one"} and any(c[1] < 4 for c in H.SQDIFF)
    # SSIM: every window; an image narrower than the window; one that spans two tiles, in either direction
    assert {c[0] for c in H.SSIM} == {3, 5, 7, 11}
    for ws in (3, 5, 7, 11):
        mine = [c for c in H.SSIM if c[0] == ws]
        assert any(c[4] < ws and c[3] < ws for c in mine) and any(c[3] > 32 for c in mine) and any(c[4] > 64 for c in mine)
        assert any(c[1] * c[2] > 1 for c in mine)
    assert [c for c in H.U8] == [(1, 64, 64), (3, 45, 70), (4, 5, 3)]
