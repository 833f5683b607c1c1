"""GPU: the MlpDWBN node leaves out work on the samples its DropPath drops (ops.DROP_PATH_SKIP): its forward frame kernels and
norm1's backward write zeros for their frames (csrc/common.h FrameSkip), its fc1 / fc2 forward and dgrad GEMMs run the tiles inside
them on zero accumulators (GemmParams::rskip).  Skipping omits reads and arithmetic, never a write: a skipped frame or tile gets
what its kernel would produce from a zero input (forward) or a zero gradient (backward), so every tensor of the node stays defined
and the kernels that skip nothing - the fused middle's backward, norm2's parameter-gradient pass, the weight gradients, the bf16x6
routes - stay correct on them.  The node with the switch on against the node with the switch off, same inputs, same mask draws; a
captured training step with DropPath at 0.5 against the eager one; the GEMMs through npvp_gemm_f32_skip / npvp_linear_bwd_f16_skip."""
import functools

import pytest
import torch

import golden_cases as GC
from oracle import ops as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_DROP, P_DP = 0.3, 0.5
NAMES = ["y", "dx", "dres", "dw1", "db1", "dn1w", "dn1b", "ddww", "ddwb", "dn2w", "dn2b", "dw2", "db2", "dn3w", "dn3b"]


@pytest.fixture(scope="module")
def K():
    import npvp_amd
    from npvp_amd import ops
    assert torch.cuda.is_available()
    ops.set_gemm_precision("f16x3")
    assert ops.mlpdwbn_fused_supported(6 * 64, 512, 2048, 512, 8, 8)
    return ops


@functools.lru_cache(maxsize=None)
def _inputs(frames):
    C, hid, P = 512, 2048, 64
    R = frames * P
    mk = lambda shape, seed, sc=1.0, off=0.0: (off + sc * O.seeded_randn(shape, seed)).to(DEV).requires_grad_()
    x, res = mk((R, C), 901), mk((R, C), 902)
    w1, b1 = mk((hid, C), 903, C ** -0.5), mk((hid,), 904, 0.1)
    n1w, n1b = mk((P * hid,), 905, 0.1, 1.0), mk((P * hid,), 906, 0.1)
    dww, dwb = mk((hid, 1, 3, 3), 907, 0.3), mk((hid,), 908, 0.1)
    n2w, n2b = mk((P * hid,), 909, 0.1, 1.0), mk((P * hid,), 910, 0.1)
    w2, b2 = mk((C, hid), 911, hid ** -0.5), mk((C,), 912, 0.1)
    n3w, n3b = mk((P * C,), 913, 0.1, 1.0), mk((P * C,), 914, 0.1)
    cot = O.seeded_randn((R, C), 915).to(DEV)
    return [x, res, w1, b1, n1w, n1b, dww, dwb, n2w, n2b, w2, b2, n3w, n3b], cot


def _forward(K, frames, T, seed):
    dev = torch.device(DEV)
    leaves, _ = _inputs(frames)
    K.rng.manual_seed(seed, dev)
    K.rng.begin_step(dev)
    return K.mlpdwbn(*leaves, frames, T, P_DROP, P_DP)


_SEEDS = {}


def _seeds(K, frames, T):
    """{"mixed" | "kept" | "dropped": (seed, keep flag per sample)}: the first seeds 0, 1, 2, ... whose DropPath mask - replayed on
    the GPU through DropRecorder.mask from the site the node recorded - has both kinds of sample, only kept ones, only dropped ones"""
    if (frames, T) in _SEEDS:
        return _SEEDS[(frames, T)]
    dev = torch.device(DEV)
    K.DropRecorder.sites = []
    try:
        with torch.no_grad():
            _forward(K, frames, T, 0)
        sites = [s for s in K.DropRecorder.sites if s[1] == "group"]
    finally:
        K.DropRecorder.sites = None
    assert len(sites) == 1 and sites[0][2] == frames // T
    found = {}
    for seed in range(400):
        K.rng.manual_seed(seed, dev)
        K.rng.begin_step(dev)
        keep = (K.DropRecorder.mask(sites[0], dev) != 0).cpu()
        kind = "kept" if bool(keep.all()) else "dropped" if not bool(keep.any()) else "mixed"
        found.setdefault(kind, (seed, keep))
        if len(found) == 3:
            break
    assert len(found) == 3, f"no seed below 400 for {set(('mixed', 'kept', 'dropped')) - set(found)}"
    _SEEDS[(frames, T)] = found
    return found


def _run(K, frames, T, seed, skip):
    """-> [y, 14 gradients], (h2, a2) as the node saved them for backward"""
    leaves, cot = _inputs(frames)
    keep = K.DROP_PATH_SKIP
    K.DROP_PATH_SKIP = skip
    try:
        y = _forward(K, frames, T, seed)
        saved = y.grad_fn.saved_tensors
        h2, a2 = saved[2].clone(), saved[3].clone()
        out = [y.detach()] + [t.detach() for t in torch.autograd.grad(y, leaves, cot)]
        torch.cuda.synchronize()
        return out, (h2, a2)
    finally:
        K.DROP_PATH_SKIP = keep


class _Route:
    """the node's backward routes: norm2 inside the fused middle (default), norm2 as kernels of its own, and the bf16x6 weight
    gradients of the range guard's fallback"""

    def __init__(self, K, name):
        self.K, self.name = K, name

    def __enter__(self):
        K = self.K
        self.n2 = K.MID_BWD_N2
        if self.name == "n2_outside":
            K.MID_BWD_N2 = False
        if self.name == "guard_fallback":
            K.RangeGuard.reset()
            K.RangeGuard.fallback = True

    def __exit__(self, *exc):
        self.K.MID_BWD_N2 = self.n2
        if self.name == "guard_fallback":
            self.K.RangeGuard.reset()


@pytest.mark.parametrize("route", ["default", "n2_outside", "guard_fallback"])
@pytest.mark.parametrize("frames,T", [(6, 3), (8, 2)])
def test_node_with_skip_equals_node_without(K, frames, T, route):
    """192-row samples (a sample is one and a half 128-row GEMM tiles) and 128-row samples; p_drop = 0.3, p_dp = 0.5; a mask with
    kept and dropped samples, an all-kept and an all-dropped one.  Rows of dropped samples: y bit-equal to res and dx exactly 0,
    with the switch on and off.  Everything else within rel-L2 2e-6 of the run without skipping - the bound
    test_mlpdwbn_backward_with_norm2_inside_the_fused_middle uses between two routes: the kernels skipped are elementwise, what moves
    is the power-of-two operand scale of a GEMM whose amax slot now sees zeros where it saw a dropped sample's values."""
    leaves, _ = _inputs(frames)
    res = leaves[1].detach()
    rows = T * 64
    for kind, (seed, keep) in _seeds(K, frames, T).items():
        with _Route(K, route):
            ref, (h2r, a2r) = _run(K, frames, T, seed, False)
            got, (h2g, a2g) = _run(K, frames, T, seed, True)
        for n, sample_kept in enumerate(keep.tolist()):
            sl = slice(n * rows, (n + 1) * rows)
            if sample_kept:
                assert float(h2g[sl].abs().max()) > 0 and float(a2g[sl].abs().max()) > 0, (kind, n)
                continue
            for out, tag in ((ref, "off"), (got, "on")):
                assert torch.equal(out[0][sl], res[sl]), f"{kind}, sample {n}, switch {tag}: y differs from res"
                assert float(out[1][sl].abs().max()) == 0.0, f"{kind}, sample {n}, switch {tag}: dx is not zero"
            # the switch does what it says: zeros where the sample was left out, the sample's values where it was not
            assert float(h2g[sl].abs().max()) == 0.0 and float(a2g[sl].abs().max()) == 0.0, (kind, n)
            assert float(h2r[sl].abs().max()) > 0 and float(a2r[sl].abs().max()) > 0, (kind, n)
        for u, v, name in zip(got, ref, NAMES):
            assert bool(torch.isfinite(u).all()), f"{kind}: {name} is not finite"
            e = float((u.double() - v.double()).norm() / v.double().norm().clamp_min(1e-300))
            print(f"[{route} frames={frames} T={T} {kind} seed={seed}] {name}: rel-L2 {e:.3e}")
            assert e < 2e-6, f"{kind} (seed {seed}), {name}: rel-L2 {e:.3e}"
        if kind == "kept":
            for u, v, name in zip(got, ref, NAMES):
                assert torch.equal(u, v), f"nothing dropped, yet {name} differs"


def test_captured_step_with_drop_path_equals_eager():
    """A GraphedTrainStep of a tiny predictor with drop_path = 0.5: the skip decision is taken on the device from the device seed, so
    the captured step replays to the eager step's parameters bit for bit, and the capture holds kernels only (no memset node)."""
    import npvp_amd as impl
    impl.ops.set_gemm_precision("f16x3")
    assert impl.ops.DROP_PATH_SKIP
    dev = torch.device(DEV)
    past = O.synth_features((2, 3, 512, 8, 8), 182).to(DEV); fut = O.synth_features((2, 4, 512, 8, 8), 183).to(DEV)
    runs = {}
    for graphed in (False, True):
        m = GC._small_predictor(impl, False, 181, DEV, evt_layers=1, dec_layers=2, dropout=0.1, drop_path=0.5)
        m.train()
        opt = impl.FlatAdamW(m, lr=1e-4, clip_module=m.transformer, max_grad_norm=1.0)
        impl.ops.rng.manual_seed(77, dev)
        if graphed:
            kinds = {}
            for skip in (False, True):         # (the capture with the switch on is the one replayed below)
                impl.ops.DROP_PATH_SKIP = skip
                try:
                    step = impl.GraphedTrainStep(m, opt, past, fut, 0.01, 1e-6, 1.0, warmup=1 if not skip else 0)
                finally:
                    impl.ops.DROP_PATH_SKIP = True
                kinds[skip] = {k: v for k, v in step.census.items() if v}
            assert kinds[True] == kinds[False], kinds
            assert step.census["kernel"] > 100 and step.census.get("memset", 0) == 0, step.census
            O.key_hashed_fill(m, 181)          # (rewind: the warm-up and the capture executed steps of their own)
            opt.m.zero_(); opt.v.zero_(); opt.hyper[1:2].zero_()
            impl.ops.rng.manual_seed(77, dev)
            for _ in range(3):
                out = step(past, fut, lr=1e-4)
        else:
            for _ in range(3):
                out = impl.predictor_train_step(m, opt, past, fut, 0.01, 1e-6, 1.0, sync=False)
        torch.cuda.synchronize()
        runs[graphed] = (opt.flat_p.clone(), float(out["loss"]))
    (pe, le), (pg, lg) = runs[False], runs[True]
    err = float((pe - pg).norm() / pe.norm())
    print(f"graph replay vs eager after 3 steps: parameters rel-L2 {err:.3e}, loss {le!r} / {lg!r}")
    assert torch.equal(pe, pg), f"graph replay vs eager parameters after 3 steps: rel-L2 {err:.3e}"
    assert le == lg, (le, lg)


# ------------------------------------------------------------------------------------------------ the GEMMs, through npvp_gemm_f32_skip
# ops.gemm(row_skip=...) launches npvp_gemm_f32_skip; ops.linear_bwd(skip=...) npvp_linear_bwd_f16_skip where the fused launch
# takes the shape.  M = 4 row groups of g1 rows: 64 (two groups per 128-row tile), 128 (a group is a tile) and 192 (tiles that
# straddle two groups); tiles are 64 or 128 rows high, so a 128-aligned block of 128 dropped rows lies in skipped tiles whatever the
# variant.
GROUPS = 4


def _group_seeds(K, g1):
    """as _seeds, for a row-group site of GROUPS groups of g1 rows: {kind: (seed, keep flag per group)}; the site is the first one a
    step creates (salt 1), as in _gemm_site"""
    dev = torch.device(DEV)
    found = {}
    for seed in range(400):
        site = _gemm_site(K, seed, g1)
        keep = (K.DropRecorder.mask((site, "group", GROUPS), dev) != 0).cpu()
        kind = "kept" if bool(keep.all()) else "dropped" if not bool(keep.any()) else "mixed"
        found.setdefault(kind, (seed, keep))
        if len(found) == 3:
            break
    assert len(found) == 3
    return found


def _gemm_site(K, seed, g1):
    dev = torch.device(DEV)
    K.rng.manual_seed(seed, dev)
    K.rng.begin_step(dev)
    return K.Drop(0.5, 1, g1, GROUPS)


def _row_keep(keep, g1):
    return keep.repeat_interleave(g1).to(DEV)


@pytest.mark.parametrize("rowstats", [False, True])
@pytest.mark.parametrize("N,Kk", [(256, 64), (256, 512), (512, 64), (512, 512)])
@pytest.mark.parametrize("g1", [64, 128, 192])
def test_forward_gemm_skips_the_tiles_of_dropped_groups(K, g1, N, Kk, rowstats):
    """C = A W^T + bias with and without the row skip, same operands: kept rows bit-equal; a dropped row is either bit-equal (its
    tile touches a kept group) or holds the bias exactly; a 128-aligned block of 128 dropped rows holds the bias; the frame-statistics
    partials and c_amax describe the values stored (4 096 values per partial, fp32 sums: 1e-5 of the block's scale)."""
    M = GROUPS * g1
    gen = torch.Generator(device=DEV).manual_seed(31)
    A = torch.randn(M, Kk, device=DEV, generator=gen) + 0.5
    W = torch.randn(N, Kk, device=DEV, generator=gen) / Kk ** 0.5
    bias = torch.randn(N, device=DEV, generator=gen) + 2.0
    pl = K._planes(W, "F", M)
    assert pl is not None and K._gemm_kernel_id(1, 1, M, N, Kk, 6, True) in (5, 7), "the shape must run on the fp16 forward kernel"
    frames = M // 64

    def run(site):
        C = torch.full((M, N), float("nan"), device=DEV)
        part = torch.full((frames * (N // 64) * 2,), float("nan"), device=DEV) if rowstats else None
        slot = K.AmaxSlot.new(torch.device(DEV))
        K.gemm(1, 1, M, N, Kk, A, A.stride(0), W, W.stride(0), C, bias=bias, b_pre=pl, rowstats=part, c_amax=slot, row_skip=site)
        torch.cuda.synchronize()
        return C, part, slot.read()

    for kind, (seed, keep) in _group_seeds(K, g1).items():
        site = _gemm_site(K, seed, g1)
        ref, _, _ = run(K.NO_DROP)
        got, part, amax = run(site)
        assert bool(torch.isfinite(got).all()), kind
        rk = _row_keep(keep, g1)
        assert torch.equal(got[rk], ref[rk]), f"{kind}: kept rows differ"
        is_bias = (got == bias).all(1)
        same = (got == ref).all(1)
        assert bool((is_bias | same)[~rk].all()), f"{kind}: a dropped row is neither the computed row nor the bias"
        blocks = (~rk).view(-1, 128).all(1) if M % 128 == 0 else (~rk)[: M // 128 * 128].view(-1, 128).all(1)
        for b in torch.nonzero(blocks).flatten().tolist():
            assert bool(is_bias[b * 128:(b + 1) * 128].all()), f"{kind}: rows {b * 128}..{b * 128 + 127} lie in dropped groups but were computed"
        if kind == "kept":
            assert torch.equal(got, ref)
        if kind == "dropped":
            assert bool(is_bias.all())
        assert amax == float(got.abs().max()), f"{kind}: c_amax {amax!r} is not max|C| {float(got.abs().max())!r}"
        if rowstats:
            blk = got.double().view(frames, 64, N // 64, 64).permute(0, 2, 1, 3).reshape(frames, N // 64, 4096)
            p = part.view(frames, N // 64, 2).double()
            mean, m2 = blk.mean(2), ((blk - blk.mean(2, keepdim=True)) ** 2).sum(2)
            scale = blk.abs().amax(2)
            assert float(((p[..., 0] - mean).abs() / scale).max()) < 1e-5, f"{kind}: partial means"
            assert float(((p[..., 1] - m2).abs() / (4096 * scale * scale)).max()) < 1e-5, f"{kind}: partial M2"


@pytest.mark.parametrize("with_a_drop", [False, True])
@pytest.mark.parametrize("N,Kk", [(256, 64), (256, 512), (512, 64), (512, 512)])
@pytest.mark.parametrize("g1", [64, 128, 192])
def test_dgrad_gemm_with_skip_is_bit_equal(K, g1, N, Kk, with_a_drop):
    """dx = dy W (dy [M, Kk], W [Kk, N]) with the rows of dy in dropped groups zero: skipped tiles store the zeros the K loop would
    have summed, so the launch with the row skip equals the launch without it bit for bit - also with a row-group mask a_drop folded
    into the staged rows (a site of its own at p = 0.3: the entry point takes a_drop below 0.5 only)."""
    M = GROUPS * g1
    gen = torch.Generator(device=DEV).manual_seed(37)
    dy0 = torch.randn(M, Kk, device=DEV, generator=gen)
    W = torch.randn(Kk, N, device=DEV, generator=gen) / Kk ** 0.5
    pl = K._planes(W, "D", M)
    assert pl is not None and K._gemm_kernel_id(1, 0, M, N, Kk, 6, True) in (5, 7), "the shape must run on the fp16 dgrad kernel"
    for kind, (seed, keep) in _group_seeds(K, g1).items():
        site = _gemm_site(K, seed, g1)
        a_drop = K.Drop(0.3, 1, g1, GROUPS) if with_a_drop else K.NO_DROP
        rk = _row_keep(keep, g1)
        dy = dy0 * rk[:, None]
        outs = []
        for rs in (K.NO_DROP, site):
            dx = torch.full((M, N), float("nan"), device=DEV)
            slot = K.AmaxSlot.new(torch.device(DEV))
            K.gemm(1, 0, M, N, Kk, dy, dy.stride(0), W, W.stride(0), dx, b_pre=pl, replay=True, a_drop=a_drop, c_amax=slot, row_skip=rs)
            torch.cuda.synchronize()
            outs.append((dx, slot.read()))
        (ref, ra), (got, ga) = outs
        assert torch.equal(got, ref), f"{kind}: dx differs"
        assert ga == ra == float(got.abs().max())
        assert float(got[~rk].abs().max()) == 0.0 if bool((~rk).any()) else True
        if kind != "dropped" and not with_a_drop:
            assert float(got[rk].abs().max()) > 0


@pytest.mark.parametrize("R,g1", [(1024, 128), (1152, 192)])
def test_fused_linear_backward_with_skip_is_bit_equal(K, R, g1):
    """ops.linear_bwd on the fused dgrad + weight-gradient launch (npvp_linear_bwd_f16_skip): dx, and the dw / db the same launch
    leaves in the sink, equal the launch without the row skip bit for bit (dy's dropped rows are zero)."""
    from npvp_amd.trainer import FlatBuffers
    N, Kk = 128, 128
    dev = torch.device(DEV)
    groups = R // g1
    x, dy0 = O.seeded_randn((R, Kk), 412).to(DEV), O.seeded_randn((R, N), 411).to(DEV)
    lin = torch.nn.Linear(Kk, N)
    with torch.no_grad():
        lin.weight.copy_(O.seeded_randn((N, Kk), 415) / Kk ** 0.5)
    lin = lin.to(dev)
    fb = FlatBuffers(lin)
    w, b = lin.weight, lin.bias
    sk = K._wb_sink(w, b)
    assert sk is not None and K.FusedLinearBwd.takes(R, N, Kk)
    for seed in range(50):          # the first seed whose mask drops some groups and keeps some
        K.rng.manual_seed(seed, dev)
        K.rng.begin_step(dev)
        site = K.Drop(0.5, 1, g1, groups)
        keep = (K.DropRecorder.mask((site, "group", groups), dev) != 0)
        if bool(keep.any()) and not bool(keep.all()):
            break
    assert bool(keep.any()) and not bool(keep.all())
    dy = dy0 * keep.repeat_interleave(g1)[:, None]
    old = (K.WgradStream.enabled, K.WgradChain.enabled, K.FusedLinearBwd.enabled, K.FusedLinearBwd.with_gradient_stream)
    outs = []
    try:
        K.WgradStream.join()
        K.WgradStream.enabled, K.WgradChain.enabled, K.FusedLinearBwd.enabled, K.FusedLinearBwd.with_gradient_stream = False, True, True, False
        for rs in (K.NO_DROP, site):
            fb.flat_g.zero_()
            calls = []
            name = "npvp_linear_bwd_f16_skip"                      # (the one entry point of the fused launch; its skip words: a[31:35])
            real = getattr(K.lib(), name)
            setattr(K.lib(), name, lambda *a: (calls.append(a[31:35]), real(*a))[1])
            try:
                dx, gw, gb = K.linear_bwd(dy, x, w, b, sk, skip=K.SampleSkip.of(K.skip_roles("mlpdwbn", True, True), rs, g1, groups, R))
            finally:
                setattr(K.lib(), name, real)
            assert len(calls) == 1 and gw is None and gb is None, "the fused entry point was not the one launched"
            assert calls[0] == (site.p, site.g1, site.g2, site.salt) if rs.on else calls[0][0] == 0, calls
            K.ReduceQueue.finish()
            torch.cuda.synchronize()
            outs.append((dx.clone(), w.grad.clone(), b.grad.clone()))
    finally:
        K.WgradStream.join()
        K.WgradStream.enabled, K.WgradChain.enabled, K.FusedLinearBwd.enabled, K.FusedLinearBwd.with_gradient_stream = old
    for u, v, n in zip(outs[1], outs[0], ("dx", "dw", "db")):
        assert torch.equal(u, v), f"{n} differs"
    assert float(outs[1][0].abs().max()) > 0 and float(outs[1][1].abs().max()) > 0
    assert float(outs[1][0][~keep.repeat_interleave(g1)].abs().max()) == 0.0
