"""GPU: the chained fp16 weight gradient with a ROW SKIP (npvp_wgrad_f16_chained_skip, ops.WGRAD_ROW_SKIP).  dy has exact zeros in the
rows of the row groups a DropPath site dropped; the launch decides the groups on the device from the seed, leaves their K-steps out
(x is not read there) and deals the kept K-steps evenly over its split-K workgroups (csrc/kept_runs.h; its host check is
tools/kept_runs_check.cpp).  dW / db are then what the launch without the skip gives up to the order of the split-K sum.

Shapes: the smallest the chained kernel takes - 8 groups x 256 rows with a one-tile 128 x 256 gradient (8 splits of 16 K-steps: a
group is a split), the same rows with a ragged four-tile 192 x 384 gradient, and 6 groups x 512 rows (8 splits of 24 K-steps over
groups of 32: shares that straddle groups).  Patterns of DROPPED groups: none, the first, the last, two adjacent, alternating, all
but one, all - found by scanning (seed, salt) pairs and reading the mask back through npvp_drop_apply on ones; a pattern that is not
found fails.

The bound is measured, not fixed: the entry point WITHOUT the skip against fp64 on the same inputs, in the same test; the skip form
may exceed that error by a factor 2 - the margin of another split-K order, nothing else differs."""
import collections
import ctypes
import functools

import pytest
import torch

from oracle import ops as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P = 0.45          # below 0.5: the same site also serves as a mask inside the launch (adrop)
SHAPES = {"one_tile": (8, 256, 128, 256), "ragged_tiles": (8, 256, 192, 384), "six_groups": (6, 512, 128, 256)}   # groups, rows per group, dW rows, dW columns
PATTERNS = ["none", "first", "last", "adjacent", "alternating", "all_but_one", "all"]


@pytest.fixture(scope="module")
def K():
    import npvp_amd  # noqa: F401
    from npvp_amd import ops
    from npvp_amd._lib import lib
    L = lib()
    # host code, before anything is launched: the shapes are chainable and split
    for g2, g1, M, N in SHAPES.values():
        assert L.npvp_wgrad_f16_chainable(M, N, g1 * g2) == 1, (M, N, g1 * g2)
        splits = L.npvp_wgrad_f16_chain_workspace_bytes(M, N, g1 * g2) // ((M * N + M) * 4)
        assert splits == 8, (M, N, g1 * g2, splits)
    assert torch.cuda.is_available()
    ops.set_gemm_precision("f16x3")
    return ops


def _site(K, g1, g2, salt):
    d = K.Drop.__new__(K.Drop)
    d.p, d.mode, d.g1, d.g2, d.salt = P, 1, g1, g2, salt
    return d


def _kind(dropped):
    """the pattern names a tuple of per-group `dropped` flags answers to"""
    n, k = len(dropped), sum(dropped)
    out = []
    if k == 0:
        out.append("none")
    if k == n:
        out.append("all")
    if k == 1 and dropped[0]:
        out.append("first")
    if k == 1 and dropped[-1]:
        out.append("last")
    if k == 2 and any(dropped[i] and dropped[i + 1] for i in range(n - 1)):
        out.append("adjacent")
    if all(dropped[i] != dropped[i + 1] for i in range(n - 1)):
        out.append("alternating")
    if k == n - 1:
        out.append("all_but_one")
    return out


@functools.lru_cache(maxsize=None)
def _find_patterns(g2):
    """{pattern: (seed, salt, keep flags)}: the first (seed, salt) pair of the scan whose mask of g2 groups at probability P shows it"""
    from npvp_amd import ops as K
    dev = torch.device(DEV)
    found = {}
    for seed in range(64):
        K.rng.manual_seed(seed, dev)
        ones = torch.ones(g2, 4, device=DEV)
        masks = torch.stack([K.drop_apply(ones, _site(K, 1, g2, salt))[:, 0] for salt in range(1, 65)]).cpu()
        for salt, row in enumerate(masks.tolist(), 1):
            dropped = tuple(v == 0.0 for v in row)
            for name in _kind(dropped):
                found.setdefault(name, (seed, salt, tuple(not d for d in dropped)))
        if len(found) == len(PATTERNS):
            break
    return found


@functools.lru_cache(maxsize=None)
def _operands(name):
    g2, g1, M, N = SHAPES[name]
    R = g1 * g2
    dy = O.seeded_randn((R, M), 700 + g2).to(DEV)
    x = (O.seeded_randn((R, N), 710 + g2) + 0.25).to(DEV)
    return dy, x


def _err(got, ref):
    d, n = float((got.double() - ref).norm()), float(ref.norm())
    return 0.0 if d == 0.0 else d / n if n > 0 else float("inf")


def _launch(K, dy, x, sa, sb, site, skip, adrop=False):
    """one chained launch + its reduction job on NaN-filled outputs and workspace -> dw, db, the split-K slabs"""
    from npvp_amd._lib import lib, check
    L = lib()
    R, M = dy.shape
    N = x.shape[1]
    wsb = L.npvp_wgrad_f16_chain_workspace_bytes(M, N, R)
    ws = torch.full((wsb // 4,), float("nan"), device=DEV)
    dw, db = torch.full((M, N), float("nan"), device=DEV), torch.full((M,), float("nan"), device=DEV)
    job = ctypes.create_string_buffer(64)
    st = torch.cuda.current_stream().cuda_stream
    seed = K.rng.seed_tensor(torch.device(DEV))
    a = (site.p, site.g1, site.g2, site.salt) if adrop else (0.0, 1, 1, 0)
    head = (M, N, R, dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), dw.data_ptr(), dw.stride(0), db.data_ptr(), 0,
            sa.data_ptr(), sb.data_ptr(), None, *a)
    tail = (seed.data_ptr(), None, ctypes.addressof(job), ws.data_ptr(), wsb, st)
    if skip:
        check(L.npvp_wgrad_f16_chained_skip(*head, site.p, site.g1, site.g2, site.salt, *tail), "npvp_wgrad_f16_chained_skip")
    else:
        check(L.npvp_wgrad_f16_chained(*head, *tail), "npvp_wgrad_f16_chained")
    check(L.npvp_splitk_reduce_job(ctypes.addressof(job), st), "npvp_splitk_reduce_job")
    torch.cuda.synchronize()
    return dw, db, ws


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_skip_form_against_fp64_and_the_plain_form(K, shape, pattern):
    """checks 1 - 5 of the module text's entry point, one (shape, pattern) each"""
    g2, g1, M, N = SHAPES[shape]
    found = _find_patterns(g2)
    assert pattern in found, f"no (seed, salt) below (64, 64) drops `{pattern}` of {g2} groups: found {sorted(found)}"
    seed, salt, keep = found[pattern]
    dev = torch.device(DEV)
    K.rng.manual_seed(seed, dev)
    site = _site(K, g1, g2, salt)
    dy0, x = _operands(shape)
    rk = torch.tensor(keep, device=DEV).repeat_interleave(g1)
    dy = dy0 * rk[:, None]
    sa, sb = K.amax_of(dy), K.amax_of(x)
    ref_w, ref_b = dy.double().T @ x.double(), dy.double().sum(0)

    # 1. against fp64, beside the plain entry point's own error on the same inputs
    bw, bb, bws = _launch(K, dy, x, sa, sb, site, skip=False)
    gw, gb, gws = _launch(K, dy, x, sa, sb, site, skip=True)
    assert bool(torch.isfinite(gws).all()), "a slab or a column-sum partial of the skip form was left unwritten"
    e0w, e0b, e1w, e1b = _err(bw, ref_w), _err(bb, ref_b), _err(gw, ref_w), _err(gb, ref_b)
    print(f"[{shape} {pattern} seed={seed} salt={salt} keep={''.join('1' if k else '0' for k in keep)}] "
          f"dW rel-L2 plain {e0w:.3e} skip {e1w:.3e} | db plain {e0b:.3e} skip {e1b:.3e}")
    assert e1w <= 2 * e0w and e1b <= 2 * e0b, (e0w, e1w, e0b, e1b)
    if pattern == "all":
        assert float(gw.abs().max()) == 0.0 and float(gb.abs().max()) == 0.0 and float(gws.abs().max()) == 0.0
    else:
        assert float(gw.abs().max()) > 0
    # 2. nothing dropped: today's chunks, one run each - the slabs themselves are the plain form's
    if pattern == "none":
        assert torch.equal(gws, bws) and torch.equal(gw, bw) and torch.equal(gb, bb)
    # 3. x is not read in dropped groups
    xn = x.clone()
    xn[~rk] = float("nan")
    nw, nb, _ = _launch(K, dy, xn, sa, sb, site, skip=True)
    assert bool(torch.isfinite(nw).all()) and torch.equal(nw, gw) and torch.equal(nb, gb), "rows of x in dropped groups were read"
    # 4. the partition is a function of the mask: a second run gives the same bits
    rw, rb, rws = _launch(K, dy, x, sa, sb, site, skip=True)
    assert torch.equal(rws, gws) and torch.equal(rw, gw) and torch.equal(rb, gb)
    # 5. the mask inside the launch (adrop) on a dy that is NOT masked, with the skip: the masked-and-scaled product; its bound
    # is the plain entry point with the same adrop, same inputs
    dym = K.drop_apply(dy0, site)
    assert torch.equal(dym != 0, (dy0 != 0) & rk[:, None]), "the site's mask is not the one read back"
    ref_wm, ref_bm = dym.double().T @ x.double(), dym.double().sum(0)
    s0 = K.amax_of(dy0)
    aw, ab, _ = _launch(K, dy0, x, s0, sb, site, skip=False, adrop=True)
    cw, cb, _ = _launch(K, dy0, xn, s0, sb, site, skip=True, adrop=True)
    e0w, e0b, e1w, e1b = _err(aw, ref_wm), _err(ab, ref_bm), _err(cw, ref_wm), _err(cb, ref_bm)
    print(f"[{shape} {pattern}] adrop: dW rel-L2 plain {e0w:.3e} skip {e1w:.3e} | db plain {e0b:.3e} skip {e1b:.3e}")
    assert bool(torch.isfinite(cw).all()) and e1w <= 2 * e0w and e1b <= 2 * e0b, (e0w, e1w, e0b, e1b)


def test_a_spec_the_kernel_declines_runs_every_k_step(K):
    """groups of 128 rows (below 256) and groups that do not cover the rows once: the launch is the plain one, bit for bit - also
    where dy is NOT zero in the 'dropped' rows, which such a launch must not leave out"""
    g2, g1, M, N = SHAPES["one_tile"]
    dy, x = _operands("one_tile")
    sa, sb = K.amax_of(dy), K.amax_of(x)
    K.rng.manual_seed(3, torch.device(DEV))
    bw, bb, bws = _launch(K, dy, x, sa, sb, _site(K, g1, g2, 1), skip=False)
    for d1, d2 in ((128, 16), (256, 4), (512, 8), (264, 8)):
        gw, gb, gws = _launch(K, dy, x, sa, sb, _site(K, d1, d2, 1), skip=True)
        assert torch.equal(gws, bws) and torch.equal(gw, bw) and torch.equal(gb, bb), (d1, d2)


def test_fused_linear_backward_hands_the_skip_to_its_weight_gradient(K):
    """check 6: ops.linear_bwd on the fused dgrad + weight-gradient launch (npvp_linear_bwd_f16_skip) at 8 192 rows = 8 groups of
    1 024: dx unchanged to the bit, dw / db within the bound (the launch without the skip against fp64, factor 2)"""
    from npvp_amd.trainer import FlatBuffers
    R, g1, N, Kk = 8192, 1024, 128, 128
    g2 = R // g1
    dev = torch.device(DEV)
    seed, salt, keep = _find_patterns(g2)["adjacent"]
    x, dy0 = O.seeded_randn((R, Kk), 732).to(DEV), O.seeded_randn((R, N), 731).to(DEV)
    lin = torch.nn.Linear(Kk, N)
    with torch.no_grad():
        lin.weight.copy_(O.seeded_randn((N, Kk), 735) / Kk ** 0.5)
    lin = lin.to(dev)
    fb = FlatBuffers(lin)
    w, b = lin.weight, lin.bias
    sk = K._wb_sink(w, b)
    assert sk is not None and K.FusedLinearBwd.takes(R, N, Kk)
    K.rng.manual_seed(seed, dev)
    site = _site(K, g1, g2, salt)
    rk = torch.tensor(keep, device=DEV).repeat_interleave(g1)
    dy = dy0 * rk[:, None]
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
                dx, gw, gb = K.linear_bwd(dy, x, w, b, sk, skip=K.SampleSkip.of(K.skip_roles("mlpdwbn", True, True), rs, g1, g2, R))
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
    (dx0, w0, b0), (dx1, w1, b1) = outs
    assert torch.equal(dx1, dx0), "dx differs"
    ref_w, ref_b = dy.double().T @ x.double(), dy.double().sum(0)
    e0w, e0b, e1w, e1b = _err(w0, ref_w), _err(b0, ref_b), _err(w1, ref_w), _err(b1, ref_b)
    print(f"[fused 8192x128x128 keep={''.join('1' if k else '0' for k in keep)}] dW rel-L2 plain {e0w:.3e} skip {e1w:.3e} | "
          f"db plain {e0b:.3e} skip {e1b:.3e}")
    assert e1w <= 2 * e0w and e1b <= 2 * e0b, (e0w, e1w, e0b, e1b)
    assert float(w1.abs().max()) > 0 and not torch.equal(w1, w0), "another split-K order was expected to move some bits"


# ------------------------------------------------------------------------------------------------ the nodes
# An encoder block (its spatial self-attention sub-layer: _SelfAttnSublayer with a per-sample DropPath; its MlpDWBN: _MlpDwbn) on
# flat gradient buffers, so that the weight gradients go through the chained launches: forward + backward with ops.WGRAD_ROW_SKIP off
# and on, same parameters, same mask draws.  8 clips x 2 frames: samples of 128 token rows, which the kernel declines - nothing
# moves; 8 clips x 4 frames: samples of 256 rows, the skip is taken.
SKIP_PARAMS = ("SLMHSA.attn.in_proj_weight", "SLMHSA.attn.in_proj_bias", "SLMHSA.attn.out_proj.weight", "SLMHSA.attn.out_proj.bias",
               "SpatialFFN.fc1.weight", "SpatialFFN.fc1.bias", "SpatialFFN.fc2.weight", "SpatialFFN.fc2.bias")


@functools.lru_cache(maxsize=None)
def _plain_error():
    """check 1's bound for the nodes: the plain entry point's rel-L2 error against fp64 on the one-tile shape, nothing dropped"""
    from npvp_amd import ops as K
    dy, x = _operands("one_tile")
    g2, g1, M, N = SHAPES["one_tile"]
    w, _, _ = _launch(K, dy, x, K.amax_of(dy), K.amax_of(x), _site(K, g1, g2, 1), skip=False)
    return _err(w, dy.double().T @ x.double())


# entry point -> (index of its four skip words p, g1, g2, salt; operand orientation (a_kc, b_kc): (1, 1) forward, (1, 0) dgrad - the fused
# launch counts as one -, (0, 0) weight gradient)
CHAINED, GEMM, FUSED = "npvp_wgrad_f16_chained_skip", "npvp_gemm_f32_skip", "npvp_linear_bwd_f16_skip"
RECORDED = {CHAINED: (18, lambda a: (0, 0)), GEMM: (37, lambda a: tuple(a[0:2])), FUSED: (31, lambda a: (1, 0))}


def _block_run(impl, m, fb, x, beta, cot, seed, on, single_stream_fused=False):
    """-> parameter gradients, the two sites' keep flags, [(entry point, orientation, skip words)] of every recorded launch.
    single_stream_fused: without the gradient stream and with the fused dgrad + weight-gradient launch on, instead of the schedule in force"""
    K = impl.ops
    dev = torch.device(DEV)
    calls = []
    real = {name: getattr(K.lib(), name) for name in RECORDED}
    keep = (K.WGRAD_ROW_SKIP, K.WgradStream.enabled, K.FusedLinearBwd.enabled)
    K.WgradStream.join()
    K.WGRAD_ROW_SKIP = on
    if single_stream_fused:
        K.WgradStream.enabled, K.FusedLinearBwd.enabled = False, True
    for name, (at, orient) in RECORDED.items():
        setattr(K.lib(), name, lambda *a, name=name, at=at, orient=orient: (calls.append((name, orient(a), a[at:at + 4])), real[name](*a))[1])
    try:
        fb.flat_g.zero_()
        K.rng.manual_seed(seed, dev)
        K.rng.begin_step(dev)
        K.DropRecorder.sites = []
        y = m(x, (beta, None), impl.PosFeatFuser(512, 'layer'))
        sites = [s for s in K.DropRecorder.sites if s[1] == "group"]
        masks = [(K.DropRecorder.mask(s, dev) != 0).cpu().tolist() for s in sites]
        K.DropRecorder.sites = None
        (y * cot).sum().backward()
        K.ReduceQueue.finish()
        K.WgradStream.join()
        torch.cuda.synchronize()
    finally:
        K.DropRecorder.sites = None
        K.WGRAD_ROW_SKIP, K.WgradStream.enabled, K.FusedLinearBwd.enabled = keep
        for name in RECORDED:
            setattr(K.lib(), name, real[name])
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}, masks, calls


def _with_spec(calls):
    """the recorded launches whose skip words are on (p > 0)"""
    return [c for c in calls if c[2][0] > 0]


def _layers(m):
    """(node, N out, K in) of the block's five linear layers, in backward order"""
    hid, C = m.SpatialFFN.fc1.weight.shape[:2]
    return [("self_attn", C, C), ("self_attn", 2 * C, C), ("self_attn", C, C), ("mlpdwbn", C, hid), ("mlpdwbn", hid, C)]


def _expected_launches(K, m, R, on, single_stream_fused):
    """how many launches carry a spec, per (entry point, orientation): ops.skip_roles for the block's five linear layers - out-proj, q|k, v
    of the spatial self-attention, fc2, fc1 of the MlpDWBN - under DROP_PATH_SKIP on and WGRAD_ROW_SKIP = `on`.  The fused launch
    where FusedLinearBwd takes the layer in the single-stream schedule, else a dgrad GEMM and a chained weight gradient"""
    assert K.DROP_PATH_SKIP
    want = collections.Counter()
    for node, N, Kin in _layers(m):
        assert K.WgradChain.takes(N, Kin, R), (N, Kin, R)
        roles = K.skip_roles(node, True, on)
        want[(GEMM, (1, 1))] += int(roles.forward)
        if single_stream_fused and K.FusedLinearBwd.takes(R, N, Kin):
            want[(FUSED, (1, 0))] += int(roles.fused)
        else:
            want[(GEMM, (1, 0))] += int(roles.dgrad)
            want[(CHAINED, (0, 0))] += int(roles.wgrad)
    return +want


@pytest.mark.parametrize("T", [2, 4])
def test_nodes_with_the_switch_off_and_on(K, T):
    """check 7.  Every parameter gradient with the switch on lies within 2 x check 1's error of the one with it off (two roundings
    of one quantity); the gradients of a sub-layer whose site dropped no sample, and of every layer without such a site, are
    bit-equal.  Seeds are scanned for a step in which one of the two sites drops samples and the other keeps all."""
    import npvp_amd as impl
    from npvp_amd.trainer import FlatBuffers
    N, p = 8, 0.25
    m = impl.VidHRFormerBlockEnc(8, 8, 512, 8, 4, 0.0, p, 4, 1024)
    O.key_hashed_fill(m, 751)
    m = m.to(DEV).train()
    fb = FlatBuffers(m)
    x = O.synth_features((N, T, 8, 8, 512), 752).to(DEV).requires_grad_()
    beta = (0.5 * O.seeded_randn((T * 64, 512), 753)).to(DEV)
    cot = O.seeded_randn((N, T, 8, 8, 512), 754).to(DEV)
    bound = 2 * _plain_error()
    dev = torch.device(DEV)
    # the two DropPath sites of a step (their salts are the same every step), then the first seeds in which exactly one of them is full
    K.DropRecorder.sites = []
    try:
        with torch.no_grad():
            K.rng.manual_seed(0, dev)
            K.rng.begin_step(dev)
            m(x, (beta, None), impl.PosFeatFuser(512, 'layer'))
        sites = [s for s in K.DropRecorder.sites if s[1] == "group"]
    finally:
        K.DropRecorder.sites = None
    assert len(sites) == 2
    picked = {}
    for seed in range(400):
        K.rng.manual_seed(seed, dev)
        K.rng.begin_step(dev)
        full = tuple(bool((K.DropRecorder.mask(s, dev) != 0).all()) for s in sites)        # (attention site, MlpDWBN site)
        if full[0] != full[1]:
            picked.setdefault(full, seed)
        if len(picked) == 2:
            break
    assert len(picked) == 2, f"no seed below 400 with one site full and the other not: {picked}"
    seen = set()
    for want, seed in picked.items():
        off, masks, calls0 = _block_run(impl, m, fb, x, beta, cot, seed, False)
        assert len(masks) == 2 and all(len(k) == N for k in masks)
        assert not [c for c in _with_spec(calls0) if c[0] == CHAINED], calls0           # switch off: no chained launch carries a spec
        full = [all(k) for k in masks]
        assert tuple(full) == want
        seen.add(tuple(full))
        on, masks1, calls1 = _block_run(impl, m, fb, x, beta, cot, seed, True)
        assert masks1 == masks
        calls = [c[2] for c in _with_spec(calls1) if c[0] == CHAINED]
        assert len(calls) == 5 and all(c[1:3] == (T * 64, N) for c in calls), calls      # out-proj, q|k, v, fc2, fc1 carry the spec
        # every launch that carries a spec, per entry point and orientation, is the one ops.skip_roles names - in the schedule in
        # force and, at T = 4, single-stream with the fused launch on; every spec is the site's as groups of one sample's rows
        R = N * T * 64
        runs = [(False, False, calls0), (True, False, calls1)]
        if T == 4:
            runs += [(flag, True, _block_run(impl, m, fb, x, beta, cot, seed, flag, single_stream_fused=True)[2]) for flag in (False, True)]
        for flag, fused, rec in runs:
            got = collections.Counter(c[:2] for c in _with_spec(rec))
            assert got == _expected_launches(K, m, R, flag, fused), (T, flag, fused, got)
            assert all(c[2][1:3] == (T * 64, N) for c in _with_spec(rec)), rec
            assert any(c[0] == FUSED for c in rec) == fused, (T, flag, fused)         # (the schedule asked for is the one that ran)
        for name in off:
            e = _err(on[name], off[name].double())
            touched = name in SKIP_PARAMS and not full[0 if name.startswith("SLMHSA") else 1]
            print(f"[T={T} seed={seed} masks={masks}] {name}: rel-L2 on vs off {e:.3e}" + (" (site dropped samples)" if touched else ""))
            assert e <= bound, (name, e, bound)
            if not touched or T * 64 < 256:
                assert torch.equal(on[name], off[name]), f"{name} moved although its site kept every sample"
            elif name.endswith("weight"):
                assert not torch.equal(on[name], off[name]), f"{name}: the skip was expected to move bits of a {T * 64}-row-sample gradient"
    assert len(seen) == 2
