"""GPU: the amax-slot contract (include/npvp_hip.h: 32 words, 64 bytes apart; the bound of a tensor is their maximum).

1. PRODUCERS, entry point by entry point through the C ABI (ops.gemm / ops.linear_bwd where only the wrapper can build the arguments),
on inputs whose maximum is PLANTED where a kernel is most likely to leave it out of its bound (tests/amax_cases.py;
tests/test_amax_cases_host.py proves on the CPU that each case plants what it names).  Per case:
  (a) the slot is EXACTLY max|stored output| (float equality: an integer atomic max of bit patterns), and only the 32 words changed;
  (b) the argmax of |stored output| is the planted element, every other element below half of it;
  (c) the stored output agrees with the float64 oracle at the bound of the kernel's own value test (norm, elementwise, grid and
      attention kernels: tests/test_hip_grid_kernels.py's 1e-5 on the whole tensor and the worst row; GEMMs: tests/gemm_route_cases.py);
  then the same launch on a slot pre-set BELOW the maximum (raised to it exactly), pre-set ABOVE it (left as it is; the two
  weight-split calls zero their slot first and must return the exact new maximum) and with a NULL slot (stored output bit-identical).
  Padding that must not count holds 1e30: the columns [cols, ld) of npvp_amax, the ldc > N padding of a GEMM output, the rows of q, k, v
  beyond the sequence.  No producer documents its slot as an upper bound only: (a) is equality everywhere.
2. CONSUMERS: one forward + backward / training step with every slot checked where it reaches a kernel (class Audit below).

With NPVP_AMAX_LOG set every case appends its figures to that file (profiles/amax_slots.txt is one such run)."""
import os

import pytest
import torch

import amax_cases as A
from golden_cases import max_row_rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 1e-5
SALT, DP_SALT = 11, 12


@pytest.fixture(scope="module")
def K():
    import npvp_amd  # noqa: F401
    from npvp_amd import ops
    assert torch.cuda.is_available()
    ops.set_gemm_precision("f16x3")
    ops.rng.manual_seed(1234, torch.device(DEV))
    yield ops


def L():
    from npvp_amd._lib import lib
    return lib()


def call(name, *args):
    from npvp_amd._lib import check
    check(getattr(L(), name)(*args), name)


def P(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def new_slot(fill=0.0):
    s = torch.zeros(A.WORDS * A.STRIDE, dtype=torch.float32, device=DEV)
    s[::A.STRIDE] = fill
    return s


def read_slot(s):
    return float(s[::A.STRIDE].max())


def empty(*shape):
    return torch.empty(*shape, dtype=torch.float32, device=DEV)


def ws_of(nbytes):
    n = max(int(nbytes), 16)
    return empty((n + 3) // 4), n


def seed_ptr(K):
    return K.rng.seed_tensor(torch.device(DEV)).data_ptr()


# ------------------------------------------------------------------------------------------------------------------- runners
# run(K, case, d, slots) -> {output name: the tensor the kernel stored, valid region}; d = the case's inputs on the device,
# slots = {output name: slot tensor or None}
def run_layernorm(K, c, d, s):
    rows, C = c["rows"], c["C"]
    if c["producer"] == "layernorm_fwd":
        y, st = empty(rows, C), empty(2, rows)
        call("npvp_layernorm_fwd", P(d["x"]), P(d["w"]), P(d["b"]), P(y), P(st[0]), P(st[1]), rows, C, EPS, c["relu"], P(s["y"]), stream())
        return dict(y=y)
    dx, dw, db = empty(rows, C), empty(C), empty(C)
    ws, wsn = ws_of(L().npvp_layernorm_bwd_workspace_bytes(rows, C))
    call("npvp_layernorm_bwd", P(d["dy"]), P(d["x"]), P(d["w"]), P(d["b"]), P(d["mean"]), P(d["rstd"]), P(dx), P(dw), P(db), rows, C, 0,
         P(d.get("dres")), 0, P(s["dx"]), P(ws), wsn, stream())
    return dict(dx=dx)


def run_posfuse(K, c, d, s):
    N, T = c["N"], c["T"]
    if c["producer"] == "ln_posfuse_fwd":
        rows = N * T * 64
        y1, fused, lst, pst = empty(N * T, 64 * 512), empty(N * T, 64 * 512), empty(2, rows), empty(2, N * T)
        call("npvp_ln_posfuse_fwd", P(d["x"]), P(d["lw"]), P(d["lb"]), EPS, P(y1), P(lst[0]), P(lst[1]), P(d["add"]), P(d["beta"]),
             P(d["gamma"]), P(fused), P(pst[0]), P(pst[1]), N, T, 64, 512, EPS, P(s["y1"]), P(s["fused"]), stream())
        return dict(y1=y1, fused=fused)
    pf = c["pf"]
    y, st = empty(N * T, pf), empty(2, N * T)
    call("npvp_posfuse_fwd", P(d["x"]), P(d["add"]), P(d["beta"]), P(d["gamma"]), P(y), P(st[0]), P(st[1]), N, T, pf, EPS, P(s["y"]), stream())
    return dict(y=y)


def run_posfuse_instance(K, c, d, s):
    N, T, Pp, C = c["N"], c["T"], c["P"], c["C"]
    y, st = empty(N * T, Pp * C), empty(2, N * T * C)
    call("npvp_posfuse_instance_fwd", P(d["x"]), P(d["add"]), P(d["beta"]), P(d["gamma"]), P(y), P(st[0]), P(st[1]), N, T, Pp, C, EPS,
         P(s["y"]), stream())
    return dict(y=y)


def fln_drop_args(K, c):
    dp, dpp = (A.FLN_DROP_P if c["drop"] else 0.0), (A.FLN_DP_P if c["dp"] else 0.0)
    return (dp, SALT, dpp, DP_SALT, A.FLN_FRAMES_PER_SAMPLE if c["dp"] else 1, seed_ptr(K) if (c["drop"] or c["dp"]) else None)


def run_frameln(K, c, d, s):
    frames, pf, name = c["frames"], c["pf"], c["producer"]
    drop = fln_drop_args(K, c)
    if name == "frameln_act_fwd":
        out = empty(frames, pf)
        call("npvp_frameln_act_fwd", P(d["h"]), P(d["mean"]), P(d["rstd"]), P(d["w"]), P(d["b"]), P(d["res"]), P(out), frames, pf, *drop,
             P(s["out"]), stream())
        return dict(out=out)
    if name == "frameln_act_fwd_parts":
        out, st = empty(frames, pf), empty(2, frames)
        call("npvp_frameln_act_fwd_parts", P(d["h"]), P(d["part"]), d["part"].shape[1], A.FLN_PARTS_NB, EPS, P(st[0]), P(st[1]), P(d["w"]),
             P(d["b"]), P(d["res"]), P(out), frames, pf, *drop, P(s["out"]), stream())
        return dict(out=out)
    dh, dw, db = empty(frames, pf), empty(pf), empty(pf)
    ws, wsn = ws_of(L().npvp_frameln_act_bwd_workspace_bytes(frames, pf))
    if name == "frameln_act_bwd":
        call("npvp_frameln_act_bwd", P(d["dout"]), P(d["h"]), P(d["mean"]), P(d["rstd"]), P(d["w"]), P(d["b"]), P(dh), P(dw), P(db), frames,
             pf, *drop, 0, P(s["dh"]), P(ws), wsn, stream())
    else:
        call("npvp_frameln_act_bwd_apply", P(d["dout"]), P(d["h"]), P(d["mean"]), P(d["rstd"]), P(d["w"]), P(d["b"]), P(d["psum"]),
             d["psum"].shape[1], P(dh), P(dw), P(db), frames, pf, 0, P(s["dh"]), P(ws), wsn, stream())
    return dict(dh=dh)


def run_drop(K, c, d, s):
    out = empty(c["rows"], c["cols"])
    call("npvp_drop_apply", P(d["x"]), P(out), c["rows"], c["cols"], A.DROP_P, c["mode"], A.DROP_G1, A.DROP_G2, seed_ptr(K), SALT,
         P(s["out"]), stream())
    return dict(out=out)


def run_grid(K, c, d, s):
    F, H, W, Hp, Wp, top, left, C = (c[k] for k in ("F", "H", "W", "Hp", "Wp", "top", "left", "C"))
    if c["producer"] == "grid_center_pad":
        rows = F * Hp * Wp + c["tail"]
        dst = torch.full((rows, C), A.PAD, dtype=torch.float32, device=DEV)          # every element is written: none of this survives
        call("npvp_grid_center_pad", P(d["src"]), C, P(dst), C, F, H, W, Hp, Wp, top, left, C, rows, P(s["dst"]), stream())
        return dict(dst=dst)
    dst = empty(F * H * W, C)
    call("npvp_grid_center_cut", P(d["src"]), C, P(d["addend"]), 0 if d["addend"] is None else C, P(dst), C, F, H, W, Hp, Wp, top, left, C,
         P(s["dst"]), stream())
    return dict(dst=dst)


def run_amax(K, c, d, s):
    call("npvp_amax", P(d["x"]), c["rows"], c["cols"], c["ld"], P(s["x"]), stream())
    return dict(x=d["x"][:, :c["cols"]])


def run_split(K, c, d, s):
    recs = d["recs"]
    planes = [(torch.empty(2 * N * Kk, dtype=torch.float16, device=DEV), torch.empty(2 * N * Kk, dtype=torch.float16, device=DEV))
              for (N, Kk, ld) in recs]
    if c["producer"] == "split_weight_f16":
        (N, Kk, ld), = recs
        call("npvp_split_weight_f16", P(d["w"][0]), ld, N, Kk, P(planes[0][0]), P(planes[0][1]), P(s["w0"]), stream())
    else:
        # the slots of the three records lie in one table, as ops.WeightPlanes keeps them
        table = s["_table"]
        desc = torch.tensor([[w.data_ptr(), ld, N, Kk, f.data_ptr(), dd.data_ptr(), table[j].data_ptr(), 0]
                             for j, (w, (N, Kk, ld), (f, dd)) in enumerate(zip(d["w"], recs, planes))], dtype=torch.int64).to(DEV)
        call("npvp_split_weights_f16", P(desc), len(recs), P(table), table.numel() * 4, stream())
    out = {f"w{j}": w[:, :Kk] for j, (w, (N, Kk, ld)) in enumerate(zip(d["w"], recs))}
    out["_planes"] = planes
    return out


def padded(rows, cols, values=None):
    """a [rows, cols] view with row stride cols + LDC_PAD whose padding holds 1e30 (it must not count, and must survive)"""
    base = torch.full((rows, cols + A.LDC_PAD), A.PAD, dtype=torch.float32, device=DEV)
    v = base[:, :cols]
    if values is not None:
        v.copy_(values)
    return v


def gemm_route(a_kc, b_kc, M, N, Kk, prec, planes, plain):
    import ctypes
    out = (ctypes.c_int * 4)()
    assert L().npvp_gemm_route(a_kc, b_kc, M, N, Kk, prec, int(planes), int(plain), ctypes.addressof(out)) == 0
    return tuple(out)


def gemm_drop(K, c):
    """the case's dropout site: the SAME Drop object (salt) draws the mask of every launch of the case"""
    if c["ep"] == "dropout":
        return K.Drop(A.GEMM_DROP_P)
    if c["ep"] == "droppath":
        return K.Drop(A.GEMM_DROP_P, 1, A.GEMM_DP_G1, 1 << 20)
    return K.NO_DROP


def run_gemm(K, c, d, s):
    import gemm_route_cases as T
    M, N, Kk, role, ep = d["M"], d["N"], d["K"], d["role"], c["ep"]
    a_kc, b_kc = T.ROLES[role]
    K.set_gemm_precision(d["mode"])
    try:
        pl = K.WeightPlanes.get(d["W"], "F" if role == "fwd" else "D") if d["planes"] else None
        split = ep.startswith("split")
        route = gemm_route(a_kc, b_kc, M, N, Kk, T.MODES[d["mode"]], pl is not None, split)
        assert route[0] == c["kid"] and (route[2] > 1) == split, f"{c['id']}: route {route}"
        C = padded(M, N, d.get("base"))
        kw = {}
        if ep in ("gelu_aux", "rowstats"):
            kw["bias"] = d["bias"]
        aux = None
        if ep == "gelu_aux":
            aux = padded(M, N)
            kw.update(act=1, aux_out=aux)
        if ep == "act3":
            kw.update(act=3, aux_in=padded(M, N, d["aux_in"]))
        if ep in ("dropout", "droppath"):
            kw["drop"] = d["_drop"]
        if ep == "residual":
            kw["residual"] = d["residual"]
        if "base" in d:
            kw["accumulate"] = True
        if ep == "rowstats":
            kw["rowstats"] = empty(M // 64, N // 64, 2)
        K.gemm(a_kc, b_kc, M, N, Kk, d["A"], d["A"].stride(0), d["W"], d["W"].stride(0), C, b_pre=pl, c_amax=s["C"], **kw)
        torch.cuda.synchronize()
        for v in (C, aux):
            assert v is None or bool((v._base[:, N:] == A.PAD).all()), f"{c['id']}: the launch wrote into the ldc > N padding"
        return dict(C=C, aux_out=aux) if aux is not None else dict(C=C)
    finally:
        K.set_gemm_precision("f16x3")


def attn_args(K, c):
    mode, dim0, Pp, W, ws, Tq, Tk, heads, long_ = A.ATTN_SHAPES[c["shape"]]
    p = A.ATTN_DROP_P if c["drop"] else 0.0
    return (mode, dim0, Pp, W, ws, Tq, Tk, heads, 64, c["mask"], p, seed_ptr(K) if c["drop"] else None, SALT), long_


def run_attn(K, c, d, s):
    """q, k, v (and go) carry ATTN_PAD_ROWS rows of 1e30 beyond the sequence; so do the outputs, and those must survive"""
    args, long_ = attn_args(K, c)
    C = d["q"].shape[1]
    nq, nk = d["q"].shape[0] - A.ATTN_PAD_ROWS, d["k"].shape[0] - A.ATTN_PAD_ROWS
    full = lambda rows: torch.full((rows + A.ATTN_PAD_ROWS, C), A.PAD, dtype=torch.float32, device=DEV)
    if c["producer"] == "attn_fwd":
        o = full(nq)
        call("npvp_attn_long_fwd" if long_ else "npvp_attn_fwd", P(d["q"]), C, P(d["k"]), C, P(d["v"]), C, P(o), C, *args, P(s["o"]), stream())
        torch.cuda.synchronize()
        assert bool((o[nq:] == A.PAD).all()), "rows beyond the sequence were written"
        return dict(o=o[:nq])
    dq, dk, dv = full(nq), full(nk), full(nk)
    tail = ()
    if long_:
        ws, wsn = ws_of(L().npvp_attn_long_bwd_workspace_bytes(*args[:8]))
        tail = (P(ws), wsn)
    call("npvp_attn_long_bwd" if long_ else "npvp_attn_bwd", P(d["q"]), C, P(d["k"]), C, P(d["v"]), C, P(d["go"]), C, P(dq), C, P(dk), C,
         P(dv), C, *args, P(s["dq"]), P(s["dk"]), P(s["dv"]), *tail, stream())
    torch.cuda.synchronize()
    assert all(bool((t[n:] == A.PAD).all()) for t, n in ((dq, nq), (dk, nk), (dv, nk))), "rows beyond the sequence were written"
    return dict(dq=dq[:nq], dk=dk[:nk], dv=dv[:nk])


RUN = {"layernorm_fwd": run_layernorm, "layernorm_bwd": run_layernorm, "posfuse_fwd": run_posfuse, "ln_posfuse_fwd": run_posfuse,
       "posfuse_instance_fwd": run_posfuse_instance, "frameln_act_fwd": run_frameln, "frameln_act_fwd_parts": run_frameln,
       "frameln_act_bwd": run_frameln, "frameln_act_bwd_apply": run_frameln, "drop_apply": run_drop, "grid_center_pad": run_grid,
       "grid_center_cut": run_grid, "amax": run_amax, "split_weight_f16": run_split, "split_weights_f16": run_split,
       "gemm": run_gemm, "attn_fwd": run_attn, "attn_bwd": run_attn}
ZEROES_ITS_SLOT = ("split_weight_f16", "split_weights_f16")
NEEDS_A_SLOT = ("amax", "split_weight_f16", "split_weights_f16")


# ------------------------------------------------------------------------------------------------------------------- dropout masks
def keep_of(K, c):
    """the keep-scales a dropout case's launch will draw: the same (device seed, salt, keys) through npvp_drop_apply on ones"""
    if not A.has_dropout(c):
        return None
    sp = seed_ptr(K)

    def elem(rows, cols, p, salt, mode=0, g1=1, g2=1):
        ones, out = torch.ones(rows, cols, device=DEV), empty(rows, cols)
        call("npvp_drop_apply", P(ones), P(out), rows, cols, p, mode, g1, g2, sp, salt, None, stream())
        return out
    if c["producer"] == "drop_apply":
        return elem(c["rows"], c["cols"], A.DROP_P, SALT, c["mode"], A.DROP_G1, A.DROP_G2)
    if c["producer"] == "gemm":
        rc = A._route_case(c["shape"])
        return K.drop_apply(torch.ones(rc["M"], rc["N"], device=DEV), c["_drop"])
    if c["producer"] in ("attn_fwd", "attn_bwd"):           # one decision per attention weight, keyed by its flat [G, heads, L, S] index
        G, heads, Lq, S = A.attn_keep_shape(c)
        n = G * heads * Lq * S
        return elem((n + 3) // 4, 4, A.ATTN_DROP_P, SALT).reshape(-1)[:n].reshape(G, heads, Lq, S)
    frames, pf = c["frames"], c["pf"]
    return dict(drop=elem(frames, pf, A.FLN_DROP_P, SALT) if c["drop"] else None,
                dp=elem(frames, 4, A.FLN_DP_P, DP_SALT, 1, A.FLN_FRAMES_PER_SAMPLE, 1 << 20)[:, 0].contiguous() if c["dp"] else None)


# ------------------------------------------------------------------------------------------------------------------- the contract
def to_dev(i):
    def mv(v):
        if torch.is_tensor(v):
            return v.to(DEV)
        if isinstance(v, list):
            return [mv(t) for t in v]
        return v
    return {k: mv(v) for k, v in i.items() if k not in ("at", "keep")}


def slots_for(c, names, fill):
    """fill: the value of all 32 words, one for every slot or {output name: value}"""
    fill = fill if isinstance(fill, dict) else {n: fill for n in names}
    if c["producer"] == "split_weights_f16":
        table = torch.zeros(len(names), A.WORDS * A.STRIDE, dtype=torch.float32, device=DEV)
        for j, n in enumerate(names):
            table[j, ::A.STRIDE] = fill[n]
        s = {n: table[j] for j, n in enumerate(names)}
        s["_table"] = table
        return s
    return {n: new_slot(fill[n]) for n in names}


def plane_values(planes_f, w, slot_value, N, Kk):
    """the forward planes F[2 terms][K/8][N][8 over k] of a weight, undone: (hi + lo) / scale as [N, K]"""
    import math
    e = math.frexp(slot_value)[1] - 1                      # amax in [2^e, 2^(e+1)): the scale puts it into [2^14, 2^15)
    scale = 2.0 ** (14 - e)
    t = planes_f.double().reshape(2, Kk // 8, N, 8).sum(0) / scale
    return t.permute(1, 0, 2).reshape(N, Kk)


def value_bounds(c, i):
    """(whole-tensor rel-L2, worst-row rel-L2) bounds: those of the kernel's existing value test"""
    if c["producer"] == "gemm":
        import gemm_route_cases as T
        return T.TOL[i["mode"]], T.ROW_TOL           # tests/test_hip_gemm_routes.py
    return A.VALUE_BOUND, A.VALUE_BOUND              # tests/test_hip_grid_kernels.py


def contract(K, c):
    if c["producer"] == "gemm":
        c = dict(c, _drop=gemm_drop(K, c))
    keep = keep_of(K, c)
    i, ref = A.build(c, keep)
    d = to_dev(i)
    if "_drop" in c:
        d["_drop"] = c["_drop"]
    run = RUN[c["producer"]]
    names = [n for n in ref if n != "aux_out"]                # (aux_out has no slot; its values are checked below)
    fresh = slots_for(c, names, 0.0)
    out = run(K, c, d, fresh)
    torch.cuda.synchronize()
    maxima = {}
    for n in names:
        o = out[n]
        m, idx, rest = A.planted_ok(o, None)
        maxima[n] = m
        got = read_slot(fresh[n])
        if os.environ.get("NPVP_AMAX_LOG"):
            with open(os.environ["NPVP_AMAX_LOG"], "a") as f:
                f.write(f"{c['id']} {n} slot {got!r} max {m!r} argmax {idx} planted {i['at'].get(n)}\n")
        # (a) exact, and nothing but the 32 words was touched
        assert got == m, f"{c['id']} {n}: slot {got!r} != max|stored| {m!r}"
        pad = fresh[n].clone()
        pad[::A.STRIDE] = 0
        assert not bool(pad.any()), f"{c['id']} {n}: the slot's padding was written"
        # (b) the case probes the region it names
        if n in i["at"]:
            assert idx == i["at"][n], f"{c['id']} {n}: argmax {idx}, planted {i['at'][n]}"
            assert rest < m / 2, f"{c['id']} {n}: second largest {rest} is not below half of {m}"
        # (c) values
        if c["producer"] in ZEROES_ITS_SLOT:
            j = int(n[1:])
            N, Kk, ld = d["recs"][j]
            back = plane_values(out["_planes"][j][0], o, got, N, Kk)
            assert A.rel(back, ref[n]) <= 2.0 ** -20, f"{c['id']} {n}: planes rel-L2 {A.rel(back, ref[n]):.3e}"
        else:
            tol, row_tol = value_bounds(c, i)
            for vn in ([n, "aux_out"] if "aux_out" in ref else [n]):
                e, er = A.rel(out[vn], ref[vn]), max_row_rel_err(out[vn], ref[vn], A.ROW_FLOOR)
                assert e <= tol and er <= row_tol, f"{c['id']} {vn}: rel-L2 {e:.3e} > {tol:.0e} or worst row {er:.3e} > {row_tol:.0e}"
    # pre-set below the maximum (0.3 of it: another exponent): raised to it exactly
    low = slots_for(c, names, {n: 0.3 * maxima[n] for n in names})
    run(K, c, d, low)
    # pre-set above: left as it is (the weight splits zero their slot first)
    high = slots_for(c, names, 3.0e4)
    run(K, c, d, high)
    torch.cuda.synchronize()
    for n in names:
        assert 0 < maxima[n] < 3.0e4
        assert read_slot(low[n]) == maxima[n], f"{c['id']} {n}: pre-set 0.3 max -> {read_slot(low[n])!r}, max {maxima[n]!r}"
        want = maxima[n] if c["producer"] in ZEROES_ITS_SLOT else 3.0e4
        assert read_slot(high[n]) == want, f"{c['id']} {n}: pre-set 3e4 -> {read_slot(high[n])!r}, want {want!r}"
    # a null slot: the stored output is bit-identical
    if c["producer"] not in NEEDS_A_SLOT:
        bare = run(K, c, d, {n: None for n in names})
        torch.cuda.synchronize()
        for n in names:
            assert torch.equal(bare[n], out[n]), f"{c['id']} {n}: the output changes with the slot"


def _param(name):
    return pytest.mark.parametrize("case", A.PRODUCERS[name][0], ids=A.case_id)


@_param("attn_fwd")
def test_attn_fwd(K, case):
    """attn_fwd_mfma_kernel<1|2, 1|2>, attn_fwd_generic_kernel, attn_long_fwd_kernel (the shape beside each case in amax_cases.ATTN_SHAPES):
    o planted through v at the last query row / last key row of a partial tile"""
    contract(K, case)


@_param("attn_bwd")
def test_attn_bwd(K, case):
    """attn_bwd_mfma_kernel<1,1|2>, attn_bwd_staged1_kernel<2,1|2>, attn_bwd_generic_kernel, attn_long_bwd_q / _kv: three separate slots,
    then the packed layout ops uses (dk_amax == dq_amax): the one slot is the maximum over BOTH tensors"""
    contract(K, case)
    keep = keep_of(K, case)
    i, _ = A.build(case, keep)
    d = to_dev(i)
    both, sv = new_slot(), new_slot()
    out = run_attn(K, case, d, dict(dq=both, dk=both, dv=sv))
    m = {n: float(out[n].abs().max()) for n in out}
    assert read_slot(both) == max(m["dq"], m["dk"]), f"packed dq|dk slot {read_slot(both)!r}, dq {m['dq']!r}, dk {m['dk']!r}"
    assert read_slot(sv) == m["dv"]


@_param("gemm")
def test_gemm_c_amax(K, case):
    """every unsplit kernel id x every epilogue, and the split-K launches whose reduce kernel commits the slot; the ldc > N padding of C
    holds 1e30 and must neither count nor change"""
    contract(K, case)


def test_linear_bwd_f16_dx_amax(K):
    """the fused dgrad + weight-gradient launch (npvp_linear_bwd_f16, through ops.linear_bwd: its job records and sinks are built
    there) with act 3 and a residual: dx_amax is max|dx|, the maximum planted in the residual's last element"""
    from oracle import ops as O
    from npvp_amd.trainer import FlatBuffers
    R, N, Kk = 1024, 128, 128
    dev = torch.device(DEV)
    dy, x, aux, res = (O.seeded_randn(sh, sd).to(DEV) for sh, sd in (((R, N), 411), ((R, Kk), 412), ((R, Kk), 413), ((R, Kk), 414)))
    res[R - 1, Kk - 1] = 100.0
    lin = torch.nn.Linear(Kk, N)
    with torch.no_grad():
        lin.weight.copy_(O.seeded_randn((N, Kk), 415) / Kk ** 0.5)
    lin = lin.to(dev)
    fb = FlatBuffers(lin)
    w, b = lin.weight, lin.bias
    sk = K._wb_sink(w, b)
    assert sk is not None and K.FusedLinearBwd.takes(R, N, Kk)
    old = (K.WgradStream.enabled, K.WgradChain.enabled, K.FusedLinearBwd.enabled, K.FusedLinearBwd.with_gradient_stream)
    ref = (dy.double() @ w.detach().double()) * A._gelu_grad(aux.double()) + res.double()
    try:
        K.WgradStream.join()
        K.WgradStream.enabled, K.WgradChain.enabled, K.FusedLinearBwd.enabled, K.FusedLinearBwd.with_gradient_stream = False, True, True, False
        outs = {}
        for what, fill in (("fresh", 0.0), ("low", 30.0), ("high", 3.0e4), ("null", None)):
            slot = None if fill is None else new_slot(fill)
            fb.flat_g.zero_()
            calls = []
            real = L().npvp_linear_bwd_f16_skip          # (the one entry point ops.linear_bwd launches, spec or not)
            L().npvp_linear_bwd_f16_skip = lambda *a: (calls.append(1), real(*a))[1]
            try:
                dx, gw, gb = K.linear_bwd(dy, x, w, b, sk, act=3, aux_in=aux, residual=res, dx_amax=slot)
            finally:
                L().npvp_linear_bwd_f16_skip = real
            assert len(calls) == 1, "the fused entry point was not the one launched"
            K.ReduceQueue.finish()
            torch.cuda.synchronize()
            assert gw is None and gb is None, "the fused launch leaves the gradients in the sink"
            outs[what] = (dx, None if slot is None else read_slot(slot))
    finally:
        K.WgradStream.join()
        K.WgradStream.enabled, K.WgradChain.enabled, K.FusedLinearBwd.enabled, K.FusedLinearBwd.with_gradient_stream = old
    dx, got = outs["fresh"]
    m, idx, rest = A.planted_ok(dx, None)
    assert got == m and idx == R * Kk - 1 and rest < m / 2, (got, m, idx, rest)
    assert A.rel(dx, ref) <= 1e-5 and max_row_rel_err(dx, ref, A.ROW_FLOOR) <= 1e-4
    assert outs["low"][1] == m and outs["high"][1] == 3.0e4
    assert torch.equal(outs["null"][0], dx) and torch.equal(outs["low"][0], dx)


@_param("layernorm_fwd")
def test_layernorm_fwd(K, case):
    """ln_fwd_kernel<1>, <4>, ReLU off / on: one commit per block of 4 rows"""
    contract(K, case)


@_param("layernorm_bwd")
def test_layernorm_bwd(K, case):
    """ln_bwd_kernel<1>, <4>: the maximum through dy, and through dres (added after the normalisation's gradient)"""
    contract(K, case)


@_param("posfuse_fwd")
def test_posfuse_fwd(K, case):
    """posfuse_fwd_frame_kernel (per_frame 32768) and frame_stats_kernel + posfuse_apply_kernel (every other frame size)"""
    contract(K, case)


@_param("ln_posfuse_fwd")
def test_ln_posfuse_fwd_both_slots(K, case):
    """two slots of one kernel: each is right while the other tensor holds the smaller values"""
    contract(K, case)


@_param("posfuse_instance_fwd")
def test_posfuse_instance_fwd(K, case):
    contract(K, case)


@_param("frameln_act_fwd")
def test_frameln_act_fwd(K, case):
    """with and without the residual, dropout and DropPath (planted at an element the masks keep)"""
    contract(K, case)


@_param("frameln_act_fwd_parts")
def test_frameln_act_fwd_parts(K, case):
    contract(K, case)


@_param("frameln_act_bwd")
def test_frameln_act_bwd(K, case):
    """per_frame 1312: (per_frame / 4) % 256 = 72, so the last block's waves 2 and 3 take the early-commit branch and wave 1 is partial"""
    contract(K, case)


@_param("frameln_act_bwd_apply")
def test_frameln_act_bwd_apply(K, case):
    contract(K, case)


@_param("drop_apply")
def test_drop_apply(K, case):
    contract(K, case)


@_param("grid_center_pad")
def test_grid_center_pad(K, case):
    """zero borders and trailing rows: every element of dst is written, the slot is the centre's maximum"""
    contract(K, case)


@_param("grid_center_cut")
def test_grid_center_cut(K, case):
    """the border rows of the source hold 1e30 and are cut away: they must not count"""
    contract(K, case)


@_param("amax")
def test_amax(K, case):
    """contiguous and strided (columns [cols, ld) hold 1e30 and must not count)"""
    contract(K, case)


@_param("split_weight_f16")
def test_split_weight_f16(K, case):
    contract(K, case)


@_param("split_weights_f16")
def test_split_weights_f16(K, case):
    contract(K, case)


# ------------------------------------------------------------------------------------------------------------------- the consumer audit
# One forward + backward (or training step) with EVERY amax slot checked where it reaches a kernel: ops.gemm, the chained
# weight-gradient launch (sched.WgradChainState.launch) and the fused npvp_linear_bwd_f16_skip call of ops.linear_bwd are wrapped here, by
# monkeypatching - the package has no hook for this.  Before each launch: synchronise, read each operand (as its M x K view with its
# row stride, not the whole storage) and its slot.
#   Safety, always: the slot is finite, slot >= max|operand|, and 0 only if the operand is all zero.
#   Exactness, where the operand (or its _base) carries the tag of that very slot at a matching version: slot == max|tag owner|.
# The looseness slot / max|operand| is recorded, not asserted (a view inherits its base's bound).  The audit synchronises, so it checks
# values, not stream ordering: tests/test_hip_golden.py::test_stream_experiments_keep_the_amax_slots_ordered stays the test for that.
class Audit:
    def __init__(self, ops):
        self.ops, self.launches, self.operands, self.exact, self.worst, self.ctx = ops, 0, 0, 0, 1.0, []

    def operand(self, what, t, rows, cols, ld, slot):
        import math
        torch.cuda.synchronize()
        view = torch.as_strided(t, (rows, cols), (ld, 1), t.storage_offset())
        m, sv = float(view.abs().max()), slot.read()
        assert math.isfinite(sv), f"{what}: slot {sv}"
        assert sv >= m, f"{what}: slot {sv!r} below max|operand| {m!r}: the scaled operand can overflow fp16"
        assert sv > 0 or m == 0, f"{what}: slot 0 for an operand with max {m!r}: the GEMM would run unscaled"
        for cand in (t, t._base):
            tag = getattr(cand, "_npvp_amax", None) if cand is not None else None
            if tag is not None and tag[0] is slot and tag[1] == cand._version:
                assert sv == float(cand.abs().max()), f"{what}: tagged slot {sv!r} != max|tag owner| {float(cand.abs().max())!r}"
                self.exact += 1
                break
        self.operands += 1
        if m > 0:
            self.worst = max(self.worst, sv / m)

    def install(self, monkeypatch):
        from npvp_amd import sched
        ops, audit = self.ops, self
        real_gemm, real_chain, real_bwd = ops.gemm, sched.WgradChainState.launch, ops.linear_bwd
        real_fused = L().npvp_linear_bwd_f16_skip

        def gemm(a_kc, b_kc, M, N, Kk, Aop, lda, B, ldb, out, *args, **kw):
            prec = kw.get("precision")
            b_pre = kw.get("b_pre")
            if (ops.GEMM_PRECISION if prec is None else prec) == 6:
                kid = ops._gemm_kernel_id(a_kc, b_kc, M, N, Kk, 6, b_pre is not None)
                what = f"gemm kid {kid} [{M}x{N}x{Kk}]"
                if kid in (5, 7):                   # forward / dgrad: A [M, K] and the weight behind the planes
                    kw["a_amax"] = ops.amax_of(Aop, kw.get("a_amax"))
                    audit.operand(what + " A", Aop, M, Kk, lda, kw["a_amax"])
                    wr, wc = (N, Kk) if b_kc else (Kk, N)
                    audit.operand(what + " W", B, wr, wc, ldb, b_pre[1])
                    audit.launches += 1
                elif kid == 6:                      # weight gradient: dy [K, M], x [K, N]
                    kw["a_amax"], kw["b_amax"] = ops.amax_of(Aop, kw.get("a_amax")), ops.amax_of(B, kw.get("b_amax"))
                    audit.operand(what + " dy", Aop, Kk, M, lda, kw["a_amax"])
                    audit.operand(what + " x", B, Kk, N, ldb, kw["b_amax"])
                    audit.launches += 1
            return real_gemm(a_kc, b_kc, M, N, Kk, Aop, lda, B, ldb, out, *args, **kw)

        def chain(self_, dy, x, dw, db, dy_amax, x_amax, a_drop, flag, row_skip):
            what = f"chained wgrad [{dy.shape[1]}x{x.shape[1]}x{dy.shape[0]}]"
            audit.operand(what + " dy", dy, dy.shape[0], dy.shape[1], dy.stride(0), dy_amax)
            audit.operand(what + " x", x, x.shape[0], x.shape[1], x.stride(0), x_amax)
            audit.launches += 1
            return real_chain(self_, dy, x, dw, db, dy_amax, x_amax, a_drop, flag, row_skip)

        def linear_bwd(dy, x, w, b, sk, *args, **kw):
            audit.ctx.append((dy, x, w, kw.get("dy_amax")))
            try:
                return real_bwd(dy, x, w, b, sk, *args, **kw)
            finally:
                audit.ctx.pop()

        def fused(*a):
            # the entry point gets addresses: the tensors are those of the ops.linear_bwd call in flight, and the slots it passed are
            # the ones amax_of hands back for them
            dy, x, w, dy_amax = audit.ctx[-1]
            R, N, Kk = a[0], a[1], a[2]
            s_dy, s_x, (planes, s_w) = ops.amax_of(dy, dy_amax), ops.amax_of(x), ops._planes(w, "D", R)
            assert (a[3], a[5], a[20], a[22], a[7]) == (dy.data_ptr(), s_dy.data_ptr(), x.data_ptr(), s_x.data_ptr(), s_w.data_ptr())
            what = f"fused linear bwd [{R}x{N}x{Kk}]"
            audit.operand(what + " dy", dy, R, N, a[4], s_dy)
            audit.operand(what + " x", x, R, Kk, a[21], s_x)
            audit.operand(what + " W", w, N, Kk, w.stride(0), s_w)
            audit.launches += 1
            return real_fused(*a)

        monkeypatch.setattr(ops, "gemm", gemm)
        monkeypatch.setattr(sched.WgradChainState, "launch", chain)
        monkeypatch.setattr(ops, "linear_bwd", linear_bwd)
        monkeypatch.setattr(L(), "npvp_linear_bwd_f16_skip", fused)
        return self


def heavy(t, on):
    """one token row (the 512 channels of one pixel of one frame) x 1e3: a heavy tail that makes a stale bound matter"""
    if on:
        t = t.clone()
        (t[0, 0, :, 3, 5] if t.shape[2] == 512 else t[0, 0, 3, 5]).mul_(1e3)
    return t


def backward_into_flat_buffers(impl, m, y, cot):
    (y * cot).sum().backward()
    impl.ops.ReduceQueue.finish()
    impl.ops.WgradStream.join()
    torch.cuda.synchronize()


def audit_mlpdwbn(impl, tail, p):
    """golden_cases.case_mlpdwbn with 4 x 4 frames (1024 token rows: the fp16 forward / dgrad and weight-gradient kernels take them)"""
    from oracle import ops as O
    from npvp_amd.trainer import FlatBuffers
    m = impl.MlpDWBN(8, 8, 512, 2048, 512, drop=p)
    O.key_hashed_fill(m, 41)
    m = m.to(DEV)
    fb = FlatBuffers(m)
    x = heavy(O.seeded_randn((4, 4, 8, 8, 512), 42), tail).to(DEV).requires_grad_()
    backward_into_flat_buffers(impl, m, m(x), O.seeded_randn((4, 4, 8, 8, 512), 43).to(DEV))
    return fb


def audit_block_enc(impl, tail, p, H=8, W=8):
    """golden_cases.case_block_enc with 4 x 4 frames; H x W = 6 x 10: the centre-pad route of tests/window_pad_cases.py"""
    from oracle import ops as O
    from npvp_amd.trainer import FlatBuffers
    N, T = 4, 4
    m = impl.VidHRFormerBlockEnc(H, W, 512, 8, 4, p, p, 4, 1024)
    O.key_hashed_fill(m, 51)
    m = m.to(DEV)
    fb = FlatBuffers(m)
    x = heavy(O.synth_features((N, T, H, W, 512), 52), tail).to(DEV).requires_grad_()
    beta = (0.5 * O.seeded_randn((T * H * W, 512), 53)).to(DEV)
    y = m(x, (beta, None), impl.PosFeatFuser(512, 'layer'))
    backward_into_flat_buffers(impl, m, y, O.seeded_randn((N, T, H, W, 512), 54).to(DEV))
    return fb


def audit_block_dec(impl, tail, p):
    from oracle import ops as O
    from npvp_amd.trainer import FlatBuffers
    N, T2, T1 = 4, 4, 2
    m = impl.VidHRFormerBlockDecNAR(8, 8, 512, 8, 4, p, p, 4, 1024)
    O.key_hashed_fill(m, 61)
    m = m.to(DEV)
    fb = FlatBuffers(m)
    tgt = heavy(0.3 * O.seeded_randn((N, T2, 8, 8, 512), 62), tail).to(DEV).requires_grad_()
    qe = (0.5 * O.seeded_randn((N, 8, 8, 512), 63)).to(DEV).requires_grad_()
    mem = O.synth_features((N, T1, 8, 8, 512), 64).to(DEV).requires_grad_()
    mb, tb = (0.5 * O.seeded_randn((T1 * 64, 512), 65)).to(DEV), (0.5 * O.seeded_randn((T2 * 64, 512), 66)).to(DEV)
    y = m(tgt, qe, mem, (mb, None), (tb, None), impl.PosFeatFuser(512, 'layer'))
    backward_into_flat_buffers(impl, m, y, O.seeded_randn((N, T2, 8, 8, 512), 67).to(DEV))
    return fb


def audit_train_step(impl, tail, p):
    """golden_cases.case_train_step, variant D: two steps of the real training step (its own flat buffers, streams and queues)"""
    import golden_cases as GC
    from oracle import ops as O
    m = GC._small_predictor(impl, False, 101, DEV, dropout=p, drop_path=p)
    past = heavy(O.synth_features((2, 3, 512, 8, 8), 92), tail).to(DEV)
    fut = O.synth_features((2, 4, 512, 8, 8), 93).to(DEV)
    m.train()
    opt = impl.FlatAdamW(m, lr=1e-4, clip_module=m.transformer, max_grad_norm=1.0)
    for _ in range(2):
        impl.predictor_train_step(m, opt, past, fut, 0.01, 1e-6, 1.0)
    torch.cuda.synchronize()


# case -> (runner, dropout = drop-path probability, kwargs, the minimum of launches audited: the count of the first recorded run,
# profiles/amax_slots.txt - the same for the stock and the heavy-tailed input)
AUDIT_CASES = {
    "mlpdwbn": (audit_mlpdwbn, 0.0, {}, 6),
    "block_enc": (audit_block_enc, 0.0, {}, 30),
    "block_dec": (audit_block_dec, 0.0, {}, 46),
    "train_step_D": (audit_train_step, 0.0, {}, 224),
    "mlpdwbn_drop": (audit_mlpdwbn, 0.1, {}, 6),
    "block_enc_drop": (audit_block_enc, 0.1, {}, 30),
    "block_dec_drop": (audit_block_dec, 0.1, {}, 46),
    "block_enc_6x10": (audit_block_enc, 0.0, dict(H=6, W=10), 22),
}
# with one deferred feature off: the smallest count over the four (without a gradient stream the block's ten dgrad + weight-gradient
# pairs are ten fused launches)
FEATURE_OFF_LEAST = {"block_enc": 20, "train_step_D": 224}
FEATURES = ("WgradChain", "FusedLinearBwd", "WgradStream", "ReduceQueue")


def run_audit(impl, monkeypatch, name, tail, tag, least=None):
    ops = impl.ops
    runner, p, kw, least_on = AUDIT_CASES[name]
    least = least_on if least is None else least
    dev = torch.device(DEV)
    ops.set_gemm_precision("f16x3")
    ops.rng.manual_seed(1234, dev)
    ops.rng.begin_step(dev)
    a = Audit(ops).install(monkeypatch)
    try:
        runner(impl, tail, p, **kw)
    finally:
        monkeypatch.undo()
        ops.WgradStream.join()
        torch.cuda.synchronize()
    if os.environ.get("NPVP_AMAX_LOG"):
        with open(os.environ["NPVP_AMAX_LOG"], "a") as f:
            f.write(f"audit {name} {tag} {'heavy' if tail else 'stock'}: launches {a.launches} operands {a.operands} exact-through-tag {a.exact} "
                    f"worst slot/max {a.worst:.4g}\n")
    assert a.launches >= least, f"{name}: {a.launches} launches audited, at least {least} expected"
    assert not ops.WgradChain._pending and not ops.ReduceQueue.pending(), "a deferred reduction was left behind"
    return a


@pytest.fixture
def impl(K):
    import npvp_amd
    return npvp_amd


@pytest.mark.parametrize("tail", [False, True], ids=["stock", "heavy_row"])
@pytest.mark.parametrize("name", list(AUDIT_CASES))
def test_every_slot_a_step_consumes(impl, monkeypatch, name, tail):
    run_audit(impl, monkeypatch, name, tail, "all-on")


@pytest.mark.parametrize("feature", FEATURES)
def test_every_slot_a_step_consumes_with_one_deferred_feature_off(impl, monkeypatch, feature):
    """the same audit with each of the deferred features off in turn (toggled and restored as
    tests/test_hip_ops.py::test_linear_backward_routes_are_bit_identical does)"""
    ops = impl.ops
    knob = getattr(ops, feature)
    old = knob.enabled
    try:
        ops.WgradStream.join()
        knob.enabled = False
        for name in ("block_enc", "train_step_D"):
            run_audit(impl, monkeypatch, name, True, f"{feature}-off", FEATURE_OFF_LEAST[name])
    finally:
        ops.WgradStream.join()
        knob.enabled = old
