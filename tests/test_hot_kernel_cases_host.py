"""CPU: the cases of tests/test_hip_hot_kernels.py can see what they claim to see (tests/hot_kernel_cases.py).

  * every mutant of a family - a deliberately wrong float64 reference - is rejected by the GPU test's own comparison at >= 10 x the
    bound (or as a non-finite value) in at least one case of the family;
  * the fp32 CPU oracle passes every case and every output at bound / 4: a condition on the INPUTS, so that the bound is not inside
    the reference's own arithmetic noise;
  * the tables take both sides of every predicate the launchers branch on (the library's pure functions, no device);
  * the C-ABI calls of the fused middle's backward tests (tests/mid_bwd_calls.py) hand every pointer parameter exactly the floats
    the kernels index behind it."""
import pytest
import torch

import hot_kernel_cases as HK
import mid_bwd_calls as MC
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


# ------------------------------------------------------------------------------------------------------------------- call plans
# The fused middle's backward tests make their C-ABI calls from plans (tests/mid_bwd_calls.py).  Before a GPU sees one: every pointer
# record has exactly the extent that the kernels index (the table read off csrc/, workspaces from the library's queries), every amax
# slot its 2 KB, every pointer parameter of the prototype a record, every operand a definition.  (The first version of these tests
# wrote an operand's size by hand beside the call: a 16-byte amax slot, where frameln_act_bwd_fused_kernel peeks and raises word
# (blockIdx.x & 31) * 16 of 512 - an illegal memory access.)
PLANS = [(f, c) for f in ("mid_bwd", "mid_n2") for c in HK.CASES[f]]
plan_ids = lambda fc: f"{fc[0]}-{HK.case_id(fc[1])}"


def calls_of(family, case):
    return [s for s in MC.plan(family, case) if isinstance(s, MC.Call)]


def prototype_params(entry):
    """[(C type, name)] of an entry point's parameters: the types from npvp_amd._lib.PROTOTYPES (the parser tests/test_abi.py holds to
    its grammar), the names read beside them from the same header"""
    import re
    from npvp_amd import _lib
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)" % entry, text)
    names = [re.search(r"(\w+)\s*$", p).group(1) for p in m.group(1).split(",")]
    types = _lib.PROTOTYPES[entry][1]
    assert len(names) == len(types), entry
    return list(zip(types, names))


def values_of(c):
    return {a.name: a.value for a in c.args if isinstance(a, MC.Val)}


def plan_extent_mismatches(L, steps):
    bad = []
    for c in (s for s in steps if isinstance(s, MC.Call)):
        s = values_of(c)
        for r in MC.ptrs(c):
            want = MC.EXTENTS[c.entry][r.name][0](s, L)
            if want == 0:           # not dereferenced with these arguments: a null, or an output that must come back all pattern
                if not (r.role == "null" or (r.role == "out" and r.buf in c.untouched)):
                    bad.append((c.entry, r.name, r.role, r.count, "is not touched"))
            elif r.role == "null" or r.count != want:
                bad.append((c.entry, r.name, r.role, r.count, want))
    return bad


@pytest.mark.parametrize("fc", PLANS, ids=plan_ids)
def test_every_record_of_a_plan_has_the_extent_the_kernels_index(L, fc):
    """`==`, not `>=`: the views are exact, and the padding around them is the canary"""
    assert plan_extent_mismatches(L, MC.plan(*fc)) == []
    assert all(r.role in MC.ROLES and r.count >= 0 for c in calls_of(*fc) for r in MC.ptrs(c))


def short_slots(steps):
    """records of role `slot` that are not 512 floats, and amax parameters that got anything but a slot or a null"""
    return [(c.entry, r.name, r.role, r.count) for c in steps if isinstance(c, MC.Call) for r in MC.ptrs(c)
            if (r.role == "slot" and r.count != 512) or ("amax" in r.name and r.role not in ("slot", "null"))]


def test_every_amax_slot_has_its_2_kb():
    import ast
    import os
    for fc in PLANS:
        assert short_slots(MC.plan(*fc)) == [], fc
        assert any(r.role == "slot" for c in calls_of(*fc) for r in MC.ptrs(c)), fc
    # the slot() helper of the GPU test, which every slot operand there comes from, read from its source: its constant and its allocation
    src = ast.parse(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_hip_hot_kernels.py")).read())
    ns = {}
    exec(compile(ast.Module(body=[n for n in src.body if isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) == "AMAX_SLOT_FLOATS"],
                            type_ignores=[]), "test_hip_hot_kernels.py", "exec"), ns)
    assert ns["AMAX_SLOT_FLOATS"] == 512 == MC.AMAX_SLOT_FLOATS
    fn = next(n for n in src.body if isinstance(n, ast.FunctionDef) and n.name == "slot")
    assert ast.unparse(fn.body[-1]) == "return out_flat(AMAX_SLOT_FLOATS, torch.zeros(AMAX_SLOT_FLOATS))"


def plan_prototype_mismatches(steps):
    bad = []
    for c in (s for s in steps if isinstance(s, MC.Call)):
        params = prototype_params(c.entry)
        if len(params) != len(c.args):
            bad.append((c.entry, len(c.args), len(params)))
            continue
        for (ctype, name), a in zip(params, c.args):
            pointer = ctype.endswith("*")
            if a.name != name or pointer != isinstance(a, MC.Ptr) or (ctype == "npvp_stream_t") != (isinstance(a, MC.Val) and a.value == MC.STREAM):
                bad.append((c.entry, name, ctype, a))
        if set(c.untouched) - {r.buf for r in MC.ptrs(c) if r.role == "out"}:
            bad.append((c.entry, "untouched", c.untouched))
    return bad


@pytest.mark.parametrize("fc", PLANS, ids=plan_ids)
def test_every_pointer_parameter_of_a_prototype_has_a_record_in_order(fc):
    assert plan_prototype_mismatches(MC.plan(*fc)) == []


def plan_undefined_operands(family, case, steps):
    """a `fill` names a tensor of the case's inputs or what an earlier step left, with the record's count; no buffer name is given twice"""
    known = {k: t.numel() for k, t in MC.tensors(family, case).items()}
    bad = []
    for s in steps:
        if isinstance(s, MC.Derive):
            if known.get(s.source) is None or s.name in known:
                bad.append(("derive", s.name, s.source))
            known[s.name] = s.count
            continue
        for r in MC.ptrs(s):
            if r.role in ("in", "inout") or (r.role == "host" and r.fill):
                if known.get(r.fill) != r.count:
                    bad.append((s.entry, r.name, r.fill, known.get(r.fill), r.count))
            elif r.fill is not None:
                bad.append((s.entry, r.name, "a fill on a", r.role))
        for r in MC.ptrs(s):
            if r.buf is not None:
                if r.buf in known or r.role == "in":
                    bad.append((s.entry, r.name, "names again", r.buf))
                known[r.buf] = r.count
    return bad


@pytest.mark.parametrize("fc", PLANS, ids=plan_ids)
def test_every_operand_of_a_plan_is_defined(fc):
    assert plan_undefined_operands(*fc, MC.plan(*fc)) == []


def test_the_plan_checks_see_a_short_record(L):
    """each of the four checks above fails on a plan with one slot cut to 4 floats, and on one with a psum a partial short"""
    for fc in PLANS:
        steps = MC.plan(*fc)
        assert steps[-1].entry == "npvp_frameln_act_bwd_apply"
        record = lambda name: next(r for r in MC.ptrs(steps[-1]) if r.name == name)
        cut = lambda name, count: steps[:-1] + [MC.replaced(steps[-1], **{name: record(name)._replace(count=count)})]
        slot4, psum_short = cut("dh_amax", 4), cut("psum", record("psum").count - 2)
        assert plan_extent_mismatches(L, slot4) and short_slots(slot4) and plan_extent_mismatches(L, psum_short)
        assert plan_undefined_operands(*fc, psum_short)              # (the producer left more than the record takes)
        assert plan_prototype_mismatches(steps[:-1] + [steps[-1]._replace(args=tuple(a for a in steps[-1].args if a.name != "dh_amax"))])


def test_the_refusals_are_complete_calls_at_full_size(L):
    """the calls the GPU test expects to be refused: complete, and - but for the argument under test - with the extents of a call that
    runs, so that one which is not refused stays inside its buffers"""
    for what, c, base, family, case in MC.refusals():
        assert plan_prototype_mismatches([c]) == [] and plan_extent_mismatches(L, [base]) == [], what
        assert all(r == b or r.role == "null" for r, b in zip(MC.ptrs(c), MC.ptrs(base))), what
        assert sum(a != b for a, b in zip(c.args, base.args)) == 1, what


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
