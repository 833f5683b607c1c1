"""CPU: the cases of tests/test_hip_grid_kernels.py can see what they claim to see (tests/grid_kernel_cases.py).

  * every mutant of a family - a deliberately wrong float64 reference - is rejected by the GPU test's own comparison at >= 10 x the
    bound in at least one case of the family;
  * the fp32 CPU oracle passes every case at bound / 4: the bound is not inside the reference's own arithmetic noise;
  * the tables take both values of every predicate the kernels' launchers branch on (the library's pure functions, no device)."""
import pytest
import torch
import torch.nn.functional as F

import grid_kernel_cases as G
from oracle import ops as O


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    build.build(verbose=False)
    from npvp_amd._lib import lib
    return lib()


@pytest.mark.parametrize("family,mutant", [(f, m) for f in G.MUTANTS for m in G.MUTANTS[f]])
def test_a_wrong_reference_is_rejected(family, mutant):
    seen = []
    for case in G.CASES[family]:
        w = G.worst(G.reference(family, case, torch.float64, mutant), G.ref64(family, case))
        seen.append((G.case_id(case), f"{w:.2e}"))
        if w >= 10 * G.BOUND:
            return
    pytest.fail(f"{family}: no case puts the mutant '{mutant}' at 10 x the bound: {seen}")


@pytest.mark.parametrize("family", list(G.CASES))
def test_the_fp32_oracle_is_well_inside_the_bound(family):
    bad = []
    for case in G.CASES[family]:
        ref, f32 = G.ref64(family, case), G.ref32(family, case)
        for k in ref:
            e = max(G.errors(f32[k], ref[k]))
            print(f"{family}[{G.case_id(case)}] {k} fp32-cpu {e:.3e}")
            if e > G.BOUND / 4:
                bad.append((G.case_id(case), k, f"{e:.2e}"))
    assert not bad, bad


def test_the_fp32_oracle_on_the_layernorm_pair_and_the_droppath_case():
    a, b = G.layernorm_res_reference(torch.float32), G.layernorm_res_reference(torch.float64)
    assert G.worst(a, b) <= G.BOUND / 4
    case, seed = G.droppath_case(), G.SEED["droppath"]
    scale = torch.tensor([0.0, 0.0, 2.0, 2.0] * 8)
    a, b = (G.frameln_reference(case, dt, seed=seed, frame_scale=scale) for dt in (torch.float32, torch.float64))
    assert G.worst(a, b) <= G.BOUND / 4


def test_the_restated_posfuse_equals_the_oracle():
    """posfuse_restated carries the index mutants; without one it is oracle.ops.posfuse"""
    for family in ("posfuse_layer", "posfuse_instance"):
        for case in G.CASES[family][:4]:
            i = G.posfuse_inputs(family, case, torch.float64)
            norm = "layer" if family == "posfuse_layer" else "instance"
            want = O.posfuse(i["x"], case[1], i["beta"], i["gamma"], i["add"], norm)
            got = G.posfuse_restated(i["x"], case[1], i["beta"], i["gamma"], i["add"], norm)
            assert G.rel(got, want) < 1e-15


@pytest.mark.parametrize("case", G.IM2COL, ids=G.case_id)
def test_im2col_reference(case):
    """the pad-and-slice im2col against torch's unfold (channel-major there, tap-major here), and col2im as its adjoint:
    <im2col(x), y> == <x, col2im(y)> in float64 to 1e-12"""
    Fr, H, W, C = case
    i = G.im2col_inputs(case, torch.float64)
    ref = G.ref64("im2col", case)
    unf = F.unfold(i["x"].detach().reshape(Fr, H, W, C).permute(0, 3, 1, 2), 3, padding=1)        # [Fr, C*9, P]
    assert torch.equal(ref["cols"], unf.reshape(Fr, C, 9, H * W).permute(0, 3, 2, 1).reshape(Fr * H * W, 9 * C))
    lhs, rhs = float((ref["cols"] * i["cot"]).sum()), float((i["x"].detach() * ref["dx"]).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)
    assert torch.equal(G.ref32("im2col", case)["cols"].double(), ref["cols"])                       # a copy: exact in any dtype


def both(values):
    return set(bool(v) for v in values) == {False, True}


def test_the_tables_take_both_sides_of_every_route(L):
    pf_layer = [(n, t, p * c) for (n, t, p, c, *_) in G.POSFUSE_LAYER]
    assert both(L.npvp_posfuse_bwd_fused(n, t, pf) for n, t, pf in pf_layer)
    # per_frame % 1024 == 0 and STILL the unfused backward (few blocks, more than 16 samples)
    assert any(pf % 1024 == 0 and not L.npvp_posfuse_bwd_fused(n, t, pf) for n, t, pf in pf_layer)
    pf_fln = [p * ch for (_, p, ch, *_) in G.FRAMELN]
    for pfs in ([pf for _, _, pf in pf_layer], pf_fln):
        assert both(pf % 1024 != 0 for pf in pfs)
        assert both(pf < 2048 for pf in pfs)
        assert all(pf % 4 == 0 and pf != 32768 for pf in pfs)
    assert both((pf // 4) % 256 != 0 for pf in pf_fln) and all(pf % 16 == 0 for pf in pf_fln)
    bad = G.FRAMELN_BAD_PER_FRAME
    assert (bad[1] * bad[2]) % 4 == 0 and (bad[1] * bad[2]) % 16 != 0
    # frame chunks of the frame-LN backward: whole and ragged, few and many frames
    chunks = [(f,) + G.frameln_chunks(L, f, p * ch) for (f, p, ch, *_) in G.FRAMELN]
    assert both(f % per != 0 for f, per, n in chunks) and both(f > 256 for f, per, n in chunks)
    assert all((n - 1) * per < f <= n * per for f, per, n in chunks)
    # depthwise conv: pixel groups of 4, blocks of 256 channels, more frames than chunks (then some chunks stay empty)
    assert not any(H == 8 and W == 8 for (_, H, W, _) in G.DWCONV + G.IM2COL)
    assert both((H * W) % 4 != 0 for (_, H, W, _) in G.DWCONV) and both(ch % 256 != 0 for (*_, ch) in G.DWCONV)
    assert any(ch > 256 and ch % 256 == 4 for (*_, ch) in G.DWCONV)                    # a block with one live channel quad
    assert both(f > 256 for (f, *_) in G.DWCONV)
    f, _, _, ch = G.DWCONV[4]
    per, n = G.dwconv_chunks(L, f, ch)
    assert per == 2 and n == 150 and n < L.npvp_dwconv3x3_wgrad_workspace_bytes(f, ch) // (40 * ch) == 256
    assert any(H == 1 for (_, H, W, _) in G.DWCONV) and any(W == 1 for (_, H, W, _) in G.DWCONV)
    # instance norm: P below the register array's 64, a last block of channels that is not full
    assert all(p < 64 for (_, _, p, *_) in G.POSFUSE_INSTANCE) and both(c % 256 != 0 for (_, _, _, c, *_) in G.POSFUSE_INSTANCE)
    assert G.POSFUSE_INSTANCE_TOO_MANY_PIXELS > 64
    # LayerNorm: every instantiation but C = 512, one wave, one block, many blocks; its backward's partial rows from the library
    assert {c // 256 for (_, c, *_) in G.LAYERNORM} == {1, 3, 4} and {r for (r, *_) in G.LAYERNORM} == {1, 3, 1001}
    assert {L.npvp_layernorm_bwd_workspace_bytes(r, 256) // 2048 for r in (1, 3, 1001)} == {1, 251}
    # attention: every (nq, nk) of the MFMA dispatch and the generic kernels; a last block of fewer than 4 (group, head) pairs
    routes = {G.attn_route(tq, tk) for (_, _, tq, tk, _, _) in G.ATTN_TEMPORAL} | {G.attn_route(ws * ws, ws * ws) for (*_, ws) in G.ATTN_SPATIAL}
    assert routes == {(1, 1), (1, 2), (2, 1), (2, 2), "generic"}
    assert "generic" in {G.attn_route(ws * ws, ws * ws) for (*_, ws) in G.ATTN_SPATIAL}
    assert both((n * p * h) % 4 != 0 for (n, p, _, _, _, h) in G.ATTN_TEMPORAL)
    assert not any(p == 64 for (_, p, *_) in G.ATTN_TEMPORAL) and both(m for (*_, m, _) in G.ATTN_TEMPORAL)
    assert all(H != W and H % ws == 0 and W % ws == 0 for (_, H, W, ws) in G.ATTN_SPATIAL)
    # every mutant with an input it needs: an add, a mask, a flat field
    for fam in ("posfuse_layer", "posfuse_instance"):
        assert both(a for (*_, a, g, k) in G.CASES[fam]) and both(g for (*_, a, g, k) in G.CASES[fam])
        assert {(a, g) for (*_, a, g, k) in G.POSFUSE_LAYER} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for fam in ("posfuse_layer", "posfuse_instance", "frameln", "layernorm"):
        assert any(c[-1] == "flat" for c in G.CASES[fam])
    assert any(c[-1] == "shift" for c in G.POSFUSE_LAYER)
