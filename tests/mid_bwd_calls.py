"""The C-ABI calls of the fused middle's backward tests (families mid_bwd and mid_n2 of tests/hot_kernel_cases.py) as DATA, so that the
CPU can inspect every operand before a GPU sees it (tests/test_hot_kernel_cases_host.py), and tests/test_hip_hot_kernels.py only
allocates what a plan says and calls what it names.

  plan(family, case) -> steps: a Call (an entry point of include/npvp_hip.h and its arguments in prototype order: a Ptr record per pointer
      parameter, a Val per value parameter) or a Derive (a tensor made on the host from a buffer a call wrote);
  tensors(family, case) -> the case's input tensors by name (what an `in` / `inout` record's `fill` names, unless an earlier step made it);
  EXTENTS -> the floats each entry point may read or write behind each pointer parameter, read off csrc/ line by line and kept apart
      from the plans on purpose: the host test holds every record of every plan to it with `==`.

A Ptr carries the parameter's name in the header, a role, a count of floats, `fill` (the tensor that fills an `in` / `inout`) and `buf` (the
name under which later steps and the test find what the call left there).  Roles: `in` (read; a NaN-padded copy of `fill`), `out` (pattern-filled), `inout` (`fill` inside the pattern), `workspace` (pattern-
filled, handed over with its byte count), `slot` (a zeroed amax slot of AMAX_SLOT_FLOATS), `seed` (one 64-bit word on the device), `host`
(48-byte job records in host memory; `fill`: the record an earlier call wrote) and `null`.  Counts are floats (4 bytes)."""
import collections

import torch

import hot_kernel_cases as HK
from helper_kernel_cases import DROP_SALT, DROP_SEED  # noqa: F401  (the GPU test builds its seed word from DROP_SEED)

Ptr = collections.namedtuple("Ptr", "name role count fill buf")        # name: the parameter's name in the header; buf: what the buffer is called afterwards
Val = collections.namedtuple("Val", "name value")
Call = collections.namedtuple("Call", "entry args untouched")          # untouched: the `buf`s of `out` records the call must leave all pattern
Derive = collections.namedtuple("Derive", "name count source fn")      # tensors[name] = fn(the buffer `source` on the CPU), `count` floats

ROLES = ("in", "out", "inout", "workspace", "slot", "seed", "host", "null")
AMAX_SLOT_FLOATS = 32 * 16          # include/npvp_hip.h:170: a slot is 2 KB, 32 words 64 bytes apart
SEED_FLOATS = 2                     # one unsigned long long
JOB_FLOATS = 12                     # a 48-byte SumRowsJob record (include/npvp_hip.h:265)
STREAM = "<stream>"                 # the value of every npvp_stream_t parameter: the GPU test puts its stream there
P64 = HK.P64


def I(name, count, fill=None):
    return Ptr(name, "in", count, fill or name, None)


def O(name, count, buf=None):
    return Ptr(name, "out", count, None, buf or name)


def IO(name, count, fill, buf):
    return Ptr(name, "inout", count, fill, buf)


def WS(count, buf):
    return Ptr("workspace", "workspace", count, None, buf)


def SLOT(name, buf):
    return Ptr(name, "slot", AMAX_SLOT_FLOATS, None, buf)


def SEED():
    return Ptr("seed", "seed", SEED_FLOATS, None, None)


def NULL(name):
    return Ptr(name, "null", 0, None, None)


def call(entry, *args, untouched=()):
    return Call(entry, tuple(args), tuple(untouched))


def ptrs(c):
    return [a for a in c.args if isinstance(a, Ptr)]


def scalar(c, name):
    return next(a.value for a in c.args if isinstance(a, Val) and a.name == name)


def replaced(c, **changes):
    """the call with the named arguments replaced: a value for a Val, a Ptr record for a Ptr"""
    assert set(changes) <= {a.name for a in c.args}, (c.entry, sorted(changes))
    return c._replace(args=tuple((changes[a.name] if isinstance(changes[a.name], Ptr) else Val(a.name, changes[a.name]))
                                 if a.name in changes else a for a in c.args))


# ------------------------------------------------------------------------------------------------------------------- sizes of the plans
def mid_ws_floats(frames, Ch):
    """weight-gradient partials [chunks wanted][10][Ch], a chunk per frame up to 128"""
    return min(frames, 128) * 10 * Ch


def fln_ws_floats(frames, per_frame):
    """[frames][4][2] frame sums (unused by _apply and _pgrad), then [chunks wanted][dw | db]: 32 chunks from 512 frames on, else at
    most 16 of at least two frames"""
    chunks = 32 if frames >= 512 else max(1, min(frames // 2, 16))
    return frames * 8 + chunks * 2 * per_frame


def merge_frame_sums(nparts):
    """[frames * nparts * 2] -> [frames * 2]: a frame's partial (sum g, sum g hhat) pairs added in float64, rounded once"""
    return lambda t: t.double().reshape(-1, nparts, 2).sum(1).float().reshape(-1)


# ------------------------------------------------------------------------------------------------------------------- the calls
def mid_bwd_call(Fr, Ch, accumulate, tag, dwt_db, cot="cot", n2=None):
    n, nblk, ws = Fr * P64 * Ch, Ch // 256, mid_ws_floats(Fr, Ch)
    tail = (I("h1", n), I("mean1", Fr), I("rstd1", Fr), I("w1n", P64 * Ch), I("b1n", P64 * Ch), I("wt", 9 * Ch), O("da1", n, "da1" + tag), dwt_db,
            O("psum", Fr * nblk * 2, "psum" + tag), Val("frames", Fr), Val("H", 8), Val("W", 8), Val("Ch", Ch), Val("accumulate", accumulate),
            WS(ws, "ws" + tag), Val("ws_bytes", ws * 4), Val("stream", STREAM))
    untouched = (dwt_db.buf,) if accumulate == 2 else ()
    if n2 is None:
        return call("npvp_mlpdw_mid_bwd", I("dh2", n, cot), *tail, untouched=untouched)
    return call("npvp_mlpdw_mid_bwd_n2", I("da2", n, cot), I("h2", n), I("mean2", Fr), I("rstd2", Fr), I("w2n", P64 * Ch), I("b2n", P64 * Ch),
                *n2, *tail, untouched=untouched)


def apply_call(Fr, Ch, da1="da1", psum="psum"):
    """norm1's backward on the middle's own da1 and psum (nparts = Ch / 256), into a full amax slot"""
    n, pf = Fr * P64 * Ch, P64 * Ch
    ws = fln_ws_floats(Fr, pf)
    return call("npvp_frameln_act_bwd_apply", I("dout", n, da1), I("h", n, "h1"), I("mean", Fr, "mean1"), I("rstd", Fr, "rstd1"), I("w", pf, "w1n"),
                I("b", pf, "b1n"), I("psum", Fr * (Ch // 256) * 2, psum), Val("nparts", Ch // 256), O("dh", n, "dh1"), O("dw", pf, "dw1n"),
                O("db", pf, "db1n"), Val("frames", Fr), Val("per_frame", pf), Val("accumulate", 0), SLOT("dh_amax", "dh1_amax"),
                WS(ws, "ws_apply"), Val("ws_bytes", ws * 4), Val("stream", STREAM))


def mid_bwd_plan(case):
    """the three accumulate modes, the four reductions of the partials an accumulate = 2 call leaves, norm1's backward behind it"""
    Fr, Ch, kind = case
    ws = mid_ws_floats(Fr, Ch)
    red = (Val("frames", Fr), Val("Ch", Ch))
    return [mid_bwd_call(Fr, Ch, 0, "", O("dwt_db", 10 * Ch)),
            mid_bwd_call(Fr, Ch, 1, "_b", IO("dwt_db", 10 * Ch, "prior_dwt", "dwt_db_acc")),
            mid_bwd_call(Fr, Ch, 2, "_c", O("dwt_db", 10 * Ch, "dwt_db_c")),
            call("npvp_mlpdw_mid_bwd_reduce", I("workspace", ws, "ws_c"), O("dwt_db", 10 * Ch, "dwt_db_r0"), *red, Val("accumulate", 0),
                 Val("stream", STREAM)),
            call("npvp_mlpdw_mid_bwd_reduce", I("workspace", ws, "ws_c"), IO("dwt_db", 10 * Ch, "prior_dwt", "dwt_db_r1"), *red, Val("accumulate", 1),
                 Val("stream", STREAM)),
            call("npvp_mlpdw_mid_bwd_reduce_into", I("workspace", ws, "ws_c"), IO("gw", 9 * Ch, "prior_gw", "gw"), IO("gb", Ch, "prior_gb", "gb"), *red,
                 Val("stream", STREAM)),
            # (the queued form: the job records the pointers, npvp_sum_rows_multi sums into them - the buffers are judged when the plan has run)
            call("npvp_mlpdw_mid_bwd_reduce_job", I("workspace", ws, "ws_c"), IO("gw", 9 * Ch, "prior_gw", "gw_q"), IO("gb", Ch, "prior_gb", "gb_q"), *red,
                 Ptr("job", "host", JOB_FLOATS, None, "job")),
            call("npvp_sum_rows_multi", Ptr("jobs", "host", JOB_FLOATS, "job", None), Val("n", 1), Val("stream", STREAM)),
            apply_call(Fr, Ch)]


def mid_n2_plan(case):
    """norm2's frame sums and parameter gradients, the keep-scale the kernels drew (a dropout case), the middle with norm2 inside, norm1's
    backward behind it"""
    Fr, Ch, p, nparts2 = case
    n, pf = Fr * P64 * Ch, P64 * Ch
    nblk2, ws = pf // 1024, fln_ws_floats(Fr, pf)
    seed = SEED() if p > 0 else NULL("seed")
    drop = (Val("drop_p", p), Val("salt", DROP_SALT))
    steps = [call("npvp_frameln_act_bwd_pgrad", I("dout", n, "cot"), I("h", n, "h2"), I("mean", Fr, "mean2"), I("rstd", Fr, "rstd2"),
                  I("w", pf, "w2n"), I("b", pf, "b2n"), O("psum", Fr * nblk2 * 2, "psum2"), O("dw", pf, "dw2n"), O("db", pf, "db2n"), Val("frames", Fr),
                  Val("per_frame", pf), *drop, Val("dp_p", 0.0), Val("dp_salt", 0), Val("frames_per_sample", 1), seed, Val("accumulate", 0),
                  WS(ws, "ws_pgrad"), Val("ws_bytes", ws * 4), Val("stream", STREAM))]
    handed = "psum2"
    if nparts2 != nblk2:
        assert nparts2 == 1, case
        steps.append(Derive("psum2_merged", Fr * 2, "psum2", merge_frame_sums(nblk2)))
        handed = "psum2_merged"
    if p > 0:
        steps.append(call("npvp_drop_apply", I("x", n, "ones"), O("out", n, "keep"), Val("rows", Fr * P64), Val("ncols", Ch), Val("p", p), Val("mode", 0),
                          Val("g1", 1), Val("g2", 1), seed, Val("salt", DROP_SALT), SLOT("out_amax", "keep_amax"), Val("stream", STREAM)))
    steps.append(mid_bwd_call(Fr, Ch, 0, "", O("dwt_db", 10 * Ch), n2=(I("psum2", Fr * nparts2 * 2, handed), Val("nparts2", nparts2), *drop, seed)))
    steps.append(apply_call(Fr, Ch))
    return steps


def plan(family, case):
    return dict(mid_bwd=mid_bwd_plan, mid_n2=mid_n2_plan)[family](case)


def tensors(family, case):
    """the fp32 tensors a plan's `fill`s name: the case's inputs as the kernels take them (statistics in float64, rounded once)"""
    i = HK.mid_inputs(family, case)
    w = i["w"].detach()
    t = {k: i[k].detach() for k in ("h1", "w1n", "b1n", "w2n", "b2n", "cot", "prior_dwt", "prior_gw", "prior_gb")}
    t["wt"] = w.reshape(w.shape[0], 9).t().contiguous()          # the Conv2d weight [Ch, 3, 3] tap-major [9, Ch]
    t["mean1"], t["rstd1"] = HK.mid_stats_in(i)
    if family == "mid_n2":
        t["h2"], t["mean2"], t["rstd2"] = HK.mid_n2_stats_in(case)
        t["ones"] = torch.ones_like(t["h1"])
    return t


# ------------------------------------------------------------------------------------------------------------------- refusals
def refusals():
    """(what, the call, the call it was made of by changing one argument, the family and case whose tensors fill it): argument errors that an NPVP_CHECK_ARG rejects before any launch -
    mlpdw.hip:644-645 (shape, workspace), :674-675 (norm2 and dropout arguments), norm.hip:1204-1206 (_apply), :1228-1230 (_pgrad).  A
    null goes only where that line tests the pointer.  The calls are those of mid_n2's dropout case and of mid_bwd's first, every operand
    at its full size (a call that is not refused runs inside its buffers)."""
    case = HK.MID_N2[1]
    Fr, Ch, p, nparts2 = case
    pgrad, _, n2, apply_ = mid_n2_plan(case)
    bwd = mid_bwd_plan(HK.MID_BWD[0])[0]
    short = lambda c: dict(ws_bytes=scalar(c, "ws_bytes") - 4)
    out = [("nparts2 = 0", n2, dict(nparts2=0)), ("nparts2 = 257", n2, dict(nparts2=257)), ("drop_p > 0, null seed", n2, dict(seed=NULL("seed"))),
           ("drop_p = 1", n2, dict(drop_p=1.0)), ("per_frame % 1024", pgrad, dict(per_frame=P64 * Ch - 512)), ("nparts = 0", apply_, dict(nparts=0)),
           ("null psum", apply_, dict(psum=NULL("psum")))] + [("workspace 4 bytes short", c, short(c)) for c in (bwd, n2, pgrad, apply_)]
    return [(f"{c.entry} ({what})", replaced(c, **change), c) + (("mid_bwd", HK.MID_BWD[0]) if c is bwd else ("mid_n2", case)) for what, c, change in out]


# ------------------------------------------------------------------------------------------------------------------- extents, from csrc/
# EXTENTS[entry][parameter] = (floats the entry point's kernels may touch behind the pointer, where that was read).  s: the call's value
# arguments by name (frames, Ch, per_frame, nparts, nparts2, accumulate, drop_p, rows, ncols, n); L: the library, for the workspace
# queries.  0: not dereferenced with these arguments - the record is then a null, or an `out` that the call lists as untouched.
def _n(s):
    return s["frames"] * 64 * s["Ch"]


def _mid_ws(s, L):
    return L.npvp_mlpdw_mid_bwd_workspace_bytes(s["frames"], s["Ch"]) // 4


def _fln_ws(s, L):
    return L.npvp_frameln_act_bwd_workspace_bytes(s["frames"], s["per_frame"]) // 4


_MID_BWD = {
    "dh2": (lambda s, L: _n(s), "mlpdw.hip:267,310 gf + (hh * 8 + w) * Ch + c, c < Ch (grid Ch / 256 x 256 threads, :649)"),
    "h1": (lambda s, L: _n(s), "mlpdw.hip:266,309"),
    "mean1": (lambda s, L: s["frames"], "mlpdw.hip:265, f < min(frames, f0 + per chunk) (:263)"),
    "rstd1": (lambda s, L: s["frames"], "mlpdw.hip:265"),
    "w1n": (lambda s, L: 64 * s["Ch"], "mlpdw.hip:309 w1n + pix * Ch + c, pix < 64"),
    "b1n": (lambda s, L: 64 * s["Ch"], "mlpdw.hip:309"),
    "wt": (lambda s, L: 9 * s["Ch"], "mlpdw.hip:257 wt + t * Ch + c, t < 9"),
    "da1": (lambda s, L: _n(s), "mlpdw.hip:268,360"),
    "dwt_db": (lambda s, L: 0 if s["accumulate"] == 2 else 10 * s["Ch"], "mlpdw.hip:631,655; partials.h:49 (accumulate 2: no sum is launched), norm.hip:195-203 c < ncols = 10 Ch"),
    "psum": (lambda s, L: s["frames"] * (s["Ch"] // 256) * 2, "mlpdw.hip:369 psum[(f * nblk + blockIdx.x) * 2 + 1], nblk = gridDim.x = Ch / 256"),
    "workspace": (_mid_ws, "mlpdw.hip:371-374 part + blockIdx.y * 10 Ch, blockIdx.y < chunks used <= wanted (partials.h:36-38), checked :645"),
}
_FLN_IN = {
    "dout": (lambda s, L: s["frames"] * s["per_frame"], "norm.hip:757 / :798 dout + f * per_frame + e, e < per_frame"),
    "h": (lambda s, L: s["frames"] * s["per_frame"], "norm.hip:757 / :798"),
    "mean": (lambda s, L: s["frames"], "norm.hip:752 / :796"),
    "rstd": (lambda s, L: s["frames"], "norm.hip:752 / :796"),
    "w": (lambda s, L: s["per_frame"], "norm.hip:744 / :790 ld4(p.w + e)"),
    "b": (lambda s, L: s["per_frame"], "norm.hip:744 / :790"),
    "dw": (lambda s, L: s["per_frame"], "norm.hip:1160 (out = dw, split = per_frame), :195-224 the sum of the partial rows"),
    "db": (lambda s, L: s["per_frame"], "norm.hip:1160 (out_b = db: columns >= per_frame)"),
    "workspace": (_fln_ws, "norm.hip:1160 lead frames * 8, then [chunks][2 per_frame] (:773-775 / :811-813), checked :1206 / :1230"),
}
_SEED = (lambda s, L: SEED_FLOATS if s["drop_p"] > 0 else 0, "mlpdw.hip:251 / norm.hip:789 *seed only with a drop threshold")
EXTENTS = {
    "npvp_mlpdw_mid_bwd": _MID_BWD,
    "npvp_mlpdw_mid_bwd_n2": dict(
        {k: v for k, v in _MID_BWD.items() if k != "dh2"},
        da2=(lambda s, L: _n(s), "mlpdw.hip:292 gf + off (the n2 form's dh2 IS da2, :680)"),
        h2=(lambda s, L: _n(s), "mlpdw.hip:273,292"),
        mean2=(lambda s, L: s["frames"], "mlpdw.hip:272"), rstd2=(lambda s, L: s["frames"], "mlpdw.hip:272"),
        w2n=(lambda s, L: 64 * s["Ch"], "mlpdw.hip:292 n2.w2n + off, off < 64 Ch"), b2n=(lambda s, L: 64 * s["Ch"], "mlpdw.hip:292"),
        psum2=(lambda s, L: s["frames"] * s["nparts2"] * 2, "mlpdw.hip:275-276 psum2[(f * nparts2 + j) * 2 + 1], j < nparts2 <= 256 (:674)"),
        seed=_SEED),
    "npvp_mlpdw_mid_bwd_reduce": {
        "workspace": (_mid_ws, "mlpdw.hip:714,631: nb = chunks used rows of 10 Ch (norm.hip:196 / :219), inside the producer's workspace"),
        "dwt_db": (lambda s, L: 10 * s["Ch"], "norm.hip:202-203 / :222-224, c < ncols = 10 Ch")},
    "npvp_mlpdw_mid_bwd_reduce_into": {
        "workspace": (_mid_ws, "mlpdw.hip:692 part[k * 10 Ch + i], k < chunks used, i < 10 Ch"),
        "gw": (lambda s, L: 9 * s["Ch"], "mlpdw.hip:694 gw[c * 9 + tap], tap < 9"), "gb": (lambda s, L: s["Ch"], "mlpdw.hip:694 gb[c]")},
    "npvp_mlpdw_mid_bwd_reduce_job": {
        "workspace": (_mid_ws, "mlpdw.hip:709: recorded; read by sum_rows_multi_kernel, norm.hip:867"),
        "gw": (lambda s, L: 9 * s["Ch"], "norm.hip:874 J.out + ch * 9 + tap"), "gb": (lambda s, L: s["Ch"], "norm.hip:874 J.out_b + ch"),
        "job": (lambda s, L: JOB_FLOATS, "partials.h:20,40 memcpy of 48 bytes, host memory")},
    "npvp_sum_rows_multi": {"jobs": (lambda s, L: JOB_FLOATS * s["n"], "norm.hip:970-976 J[at + i], i < n, host memory")},
    "npvp_frameln_act_bwd_pgrad": dict(
        _FLN_IN, psum=(lambda s, L: s["frames"] * (s["per_frame"] // 1024) * 2, "norm.hip:809 psum[(f * nblk + blockIdx.x) * 2 + 1], nblk = per_frame / 1024 (:1233)"),
        seed=_SEED),
    "npvp_frameln_act_bwd_apply": dict(
        _FLN_IN, psum=(lambda s, L: s["frames"] * s["nparts"] * 2, "norm.hip:755 psum[(f * nparts + j) * 2 + 1], j < nparts"),
        dh=(lambda s, L: s["frames"] * s["per_frame"], "norm.hip:768 st4(dh + g0)"),
        dh_amax=(lambda s, L: AMAX_SLOT_FLOATS, "norm.hip:736,771 every block; common.h:72-81 word (blockIdx.x & 31) * 16: float offset <= 496")),
    "npvp_drop_apply": {
        "x": (lambda s, L: s["rows"] * s["ncols"], "elementwise.hip:23"), "out": (lambda s, L: s["rows"] * s["ncols"], "elementwise.hip:33"),
        "seed": (lambda s, L: SEED_FLOATS, "elementwise.hip:14 *seedp, always (p > 0 is required: :189)"),
        "out_amax": (lambda s, L: AMAX_SLOT_FLOATS, "elementwise.hip:17,36; common.h:72-81")},
}
