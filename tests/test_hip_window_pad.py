"""GPU: spatial window attention on feature grids the window does not tile (ref/models/VidHRFormer.py:488-511, PadBlock): the two
copy kernels alone through the C ABI, the module against the reference's vectors (tests/golden/window_pad.npz), the blocks in both
of their code paths, the whole predictor at 6 x 10 against predictor_window_pad.npz, attention dropout on the padded layout, and
the captured step.

Shapes are the smallest that reach every branch: odd pads (top < bottom), a pad on one axis only with ws > H, more than one block
per launch (C = 8 puts 128 rows into a block, C = 512 two), trailing rows past F*Hp*Wp, strided sources; windows of 16 rows (MFMA
attention kernels), 64 (the generic 33..128 kernels) and 144 (the streaming kernels)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import golden_cases as GC
import window_pad_cases as WC
from oracle import ops as O
from test_hip_golden import TOL          # the bound of test_slmhsa: the arithmetic is the same kernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (F, H, W, Hp, Wp, top, left)
KERNEL_SHAPES = [(2, 5, 6, 8, 8, 1, 1), (1, 3, 8, 4, 8, 0, 0), (3, 6, 10, 8, 16, 1, 3)]


@pytest.fixture(scope="module")
def npvp():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import npvp_amd
    npvp_amd.ops.set_gemm_precision("f16x3")
    return npvp_amd


def _st():
    return torch.cuda.current_stream().cuda_stream


def _strided(rows, C, seed):
    """[rows, C] with a padded row stride (ld = C + 8); the gap columns are NaN"""
    buf = torch.full((rows, C + 8), float("nan"), device=DEV)
    buf[:, :C] = O.seeded_randn((rows, C), seed).to(DEV)
    return buf[:, :C]


def _pad(L, src, dst, shape, slot=None):
    Fr, H, W, Hp, Wp, top, left = shape
    rc = L.npvp_grid_center_pad(src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), Fr, H, W, Hp, Wp, top, left, src.shape[1],
                                dst.shape[0], None if slot is None else slot.data_ptr(), _st())
    assert rc == 0, L.npvp_last_error()


def _cut(L, src, dst, shape, addend=None, slot=None):
    Fr, H, W, Hp, Wp, top, left = shape
    rc = L.npvp_grid_center_cut(src.data_ptr(), src.stride(0), None if addend is None else addend.data_ptr(),
                                0 if addend is None else addend.stride(0), dst.data_ptr(), dst.stride(0), Fr, H, W, Hp, Wp, top, left,
                                src.shape[1], None if slot is None else slot.data_ptr(), _st())
    assert rc == 0, L.npvp_last_error()


def _slot():
    return torch.zeros(512, device=DEV)          # an amax slot: 2 KB, zero before its tensor is produced


def _nan_out(rows, C):
    """a NaN-filled [rows, C] view with row stride C + 8 and the buffer it lies in"""
    buf = torch.full((rows, C + 8), float("nan"), device=DEV)
    return buf[:, :C], buf


@pytest.mark.parametrize("tail", [0, 32])
@pytest.mark.parametrize("C", [512, 8])
@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_pad_kernel_equals_f_pad(npvp, shape, C, tail):
    from npvp_amd._lib import lib
    L = lib()
    Fr, H, W, Hp, Wp, top, left = shape
    body = Fr * Hp * Wp
    rows_out = -(-body // 32) * 32 + tail
    src = _strided(Fr * H * W, C, 5 + C + H)
    want = torch.zeros(rows_out, C, device=DEV)
    want[:body] = F.pad(src.reshape(Fr, H, W, C), (0, 0, left, Wp - W - left, top, Hp - H - top)).reshape(body, C)
    outs = []
    for _ in range(2):
        dst, buf = _nan_out(rows_out, C)
        slot = _slot()
        _pad(L, src, dst, shape, slot)
        torch.cuda.synchronize()
        assert not torch.isnan(dst).any(), "an element of dst was not written (border and trailing rows included)"
        assert torch.isnan(buf[:, C:]).all(), "the kernel wrote outside the C columns of a row"
        assert torch.equal(dst, want)
        assert float(dst.abs().max()) <= float(slot.max()) <= float(src.abs().max())
        outs.append(dst.clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("with_addend", [False, True])
@pytest.mark.parametrize("C", [512, 8])
@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_cut_kernel_equals_slicing(npvp, shape, C, with_addend):
    from npvp_amd._lib import lib
    L = lib()
    Fr, H, W, Hp, Wp, top, left = shape
    body, rows = Fr * Hp * Wp, Fr * H * W
    src = _strided(-(-body // 32) * 32 + 32, C, 9 + C + H)
    addend = _strided(rows, C, 10 + C + H) if with_addend else None
    want = src[:body].reshape(Fr, Hp, Wp, C)[:, top:top + H, left:left + W].reshape(rows, C)
    if with_addend:
        want = want + addend
    outs = []
    for _ in range(2):
        dst, buf = _nan_out(rows, C)
        slot = _slot()
        _cut(L, src, dst, shape, addend, slot)
        torch.cuda.synchronize()
        assert not torch.isnan(dst).any()
        assert torch.isnan(buf[:, C:]).all()
        assert torch.equal(dst, want)
        assert float(dst.abs().max()) <= float(slot.max())
        if not with_addend:
            assert float(slot.max()) <= float(src.abs().max())
        outs.append(dst.clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_pad_and_cut_are_adjoint(npvp, shape):
    """<pad(x), y> == <x, cut(y)>: both sides sum the same products (the pad rows contribute exact zeros), so in float64 they differ
    by the rounding of the two summation orders only - 2^-53 per addition, bounded here by 1e-12 of the sum of the magnitudes"""
    from npvp_amd._lib import lib
    L = lib()
    Fr, H, W, Hp, Wp, top, left = shape
    C, rows_out = 512, -(-Fr * Hp * Wp // 32) * 32
    x, y = O.seeded_randn((Fr * H * W, C), 21).to(DEV), O.seeded_randn((rows_out, C), 22).to(DEV)
    px, cy = torch.empty(rows_out, C, device=DEV), torch.empty(Fr * H * W, C, device=DEV)
    _pad(L, x, px, shape)
    _cut(L, y, cy, shape)
    a, b = (px.double() * y.double()).sum(), (x.double() * cy.double()).sum()
    assert abs(float(a - b)) <= 1e-12 * float((x.double() * cy.double()).abs().sum())


# ------------------------------------------------------------------ the module
@pytest.mark.parametrize("i", range(len(WC.SLMHSA_CASES)))
def test_module_against_the_reference(npvp, i):
    """ws = 4: the MFMA attention kernels, ws = 8: the generic 33..128 ones"""
    case, seed = WC.fixture_case(i)
    golden = GC.load("window_pad")
    got = WC.case_slmhsa(npvp, DEV, case, seed)
    errs = {k: GC.rel_err(WC.view(got[k]), golden[f"c{i}_{k}"]) for k in WC.SLMHSA_KEYS}
    print(f"window_pad case {case}: {errs}")
    bad = {k: f"{e:.3e}" for k, e in errs.items() if not e < TOL}
    assert not bad, f"rel-L2 above {TOL:.1e}: {bad}"


@pytest.mark.parametrize("case, seed, padded, tail, streaming", [((1, 10, 14, 12), 290, (288, 24), 0, True),
                                                                   ((1, 3, 3, 4), 295, (16, 4), 16, False)])
def test_module_against_the_cpu_restatement(npvp, case, seed, padded, tail, streaming):
    """F = 1, 10 x 14, window 12 -> 12 x 24, windows of 144 rows: the streaming attention kernels.  F = 1, 3 x 3, window 4 -> one
    window of 16 rows: 16 trailing rows up to the weight-gradient GEMM's 32, which must stay out of the bias gradients."""
    Fr, H, W, ws = case
    m = npvp.SpatialLocalMultiheadAttention(512, 8, ws, 0.0)
    cfg = m._cfg(1, Fr, H, W)
    assert not cfg.tiles and (cfg.P, cfg.W) == padded and npvp.ops._attn_long(cfg) == streaming
    assert cfg.padded_rows - cfg.dim0 * cfg.P == tail
    want = WC.case_slmhsa_restated(case, seed)
    got = WC.case_slmhsa(npvp, DEV, case, seed)
    errs = {k: GC.rel_err(got[k], want[k]) for k in WC.SLMHSA_KEYS}
    print(f"window_pad against the restatement {case}: {errs}")
    bad = {k: f"{e:.3e}" for k, e in errs.items() if not e < TOL}
    assert not bad, f"rel-L2 above {TOL:.1e}: {bad}"


# ------------------------------------------------------------------ the blocks, 6 x 10, window 4, N T = 8
BH, BW, BN, BT = 6, 10, 2, 4


def _tables(T, seed, dev):
    beta = (0.5 * O.seeded_randn((T * BH * BW, 512), seed)).to(dev)
    gamma = (0.3 * O.seeded_randn((T * BH * BW, 512), seed + 1)).to(dev)
    return beta, gamma


def _run_block(impl, dev, kind, fuser):
    cls = impl.VidHRFormerBlockEnc if kind == "enc" else impl.VidHRFormerBlockDecNAR
    m = cls(BH, BW, 512, 8, 4, 0.0, 0.0, 4, 1024)
    O.key_hashed_fill(m, 301)
    if dev == "cpu":
        m = WC.restated_oracle(m)
    m = m.to(dev).train()
    x = (0.3 * O.seeded_randn((BN, BT, BH, BW, 512), 302)).to(dev).requires_grad_()
    cot = O.seeded_randn((BN, BT, BH, BW, 512), 303).to(dev)
    tb, tg = _tables(BT, 304, dev)
    if kind == "enc":
        y = m(x, (tb, tg), fuser)
        leaves = [x, m.SLMHSA.attn.in_proj_bias, m.norm1.weight]
    else:
        qe = (0.5 * O.seeded_randn((BN, BH, BW, 512), 306)).to(dev).requires_grad_()
        mem = O.synth_features((BN, BT, BH, BW, 512), 307).to(dev).requires_grad_()          # (480 rows: the weight gradients' 32)
        mb, mg = _tables(BT, 308, dev)
        y = m(x, qe, mem, (mb, mg), (tb, tg), fuser)
        leaves = [x, m.SLMHSA.attn.in_proj_bias, m.norm1.weight, qe, mem]
    g = torch.autograd.grad((y * cot).sum(), leaves)
    return [t.detach().cpu() for t in (y, *g)]


@functools.lru_cache(maxsize=None)
def _block_oracle(kind, norm):
    """the oracle's block (CPU) with its window attention restated for a grid the window does not tile: computed once, never modified"""
    import oracle
    return _run_block(oracle, "cpu", kind, oracle.PosFeatFuser(512, norm))


@pytest.mark.parametrize("kind", ["enc", "dec"])
def test_blocks_in_both_code_paths(npvp, kind):
    """The stock fuser takes the sub-layer nodes; a subclass of it computes the same function through the per-kernel autograd path:
    the two must agree with each other, and each with the CPU oracle.  An 'instance' fuser (per-kernel path, another function)
    is held against the oracle with the same fuser."""
    class OwnFuser(npvp.PosFeatFuser):          # not the stock class: the blocks run their per-kernel path
        pass
    names = ["y", "g_x", "g_slmhsa_in_proj_bias", "g_norm1_w", "g_qe", "g_mem"]
    nodes = _run_block(npvp, DEV, kind, npvp.PosFeatFuser(512, 'layer'))
    kernels = _run_block(npvp, DEV, kind, OwnFuser(512, 'layer'))
    inst = _run_block(npvp, DEV, kind, npvp.PosFeatFuser(512, 'instance'))
    bad = {}
    for tag, got, want in (("nodes-vs-kernels", nodes, kernels), ("nodes-vs-oracle", nodes, _block_oracle(kind, 'layer')),
                           ("kernels-vs-oracle", kernels, _block_oracle(kind, 'layer')),
                           ("instance-vs-oracle", inst, _block_oracle(kind, 'instance'))):
        for n, a, b in zip(names, got, want):
            e = GC.rel_err(a, b)
            print(f"block {kind} {tag} {n}: {e:.3e}")
            if not e < TOL:
                bad[f"{tag}.{n}"] = f"{e:.3e}"
    assert not bad, f"rel-L2 above {TOL:.1e}: {bad}"


# ------------------------------------------------------------------ the whole predictor
def test_predictor_against_the_reference(npvp):
    golden = GC.load("predictor_window_pad")
    m = WC.small_predictor(npvp, int(golden["meta"][5]), DEV)
    past, cot = WC.predictor_inputs(DEV)
    got = WC.run_predictor(m, past, cot)
    errs = {k: GC.rel_err(WC.view(got[k]), g) for k, g in golden.items() if k != "meta"}
    print(f"predictor 6x10: {errs}")
    assert set(errs) == {"y_eval", "y_train", "g_past", "g_tied_norm_w", *WC.PRED_PARAMS}
    bad = {k: f"{e:.3e}" for k, e in errs.items() if not e < TOL}
    assert not bad, f"rel-L2 above {TOL:.1e}: {bad}"


# ------------------------------------------------------------------ attention dropout on the padded layout
def test_attention_dropout_backward_replays_the_mask(npvp):
    """With p > 0 and one seed, o = cut(attn(qk, pad(v))) is linear in v, so <do, o(v')> == <dv(do), v'> for any v' exactly when
    the backward applies the mask the forward drew (on the padded layout: the mask is keyed by the flat index of the padded
    windows' weights).  Bound: both sides are fp32 results of 16-key softmax rows and 64-term dot products, ~100 roundings of 2^-24
    per element at the worst, summed in float64 here: 2e-5 of the sum of the magnitudes.  A mask that differed in one key of 16
    with p = 0.3 would move single terms by their own size."""
    ops = npvp.ops
    dev = torch.device(DEV)
    cfg = ops.AttnCfg.spatial(2, 5, 6, 4, 8, 0.3)
    plain = ops.AttnCfg.spatial(2, 5, 6, 4, 8, 0.0)
    R, Rp, C = 60, cfg.padded_rows, 512
    qk = O.seeded_randn((Rp, 2 * C), 401).to(DEV)
    v = O.seeded_randn((R, C), 402).to(DEV).requires_grad_()
    v2 = O.seeded_randn((R, C), 403).to(DEV)
    do = O.seeded_randn((R, C), 404).to(DEV)

    def fwd(val, c):
        ops.rng.manual_seed(4242, dev)
        return ops.grid_cut(ops.attn_packed(qk, ops.grid_pad(val, c), c), c)

    o = fwd(v, cfg)
    dv, = torch.autograd.grad((o * do).sum(), v)
    with torch.no_grad():
        o2, o_plain = fwd(v2, cfg), fwd(v, plain)
    assert GC.rel_err(o, o_plain) > 0.1, "the dropout mask is not applied"
    lhs, rhs = (do.double() * o2.double()).sum(), (dv.double() * v2.double()).sum()
    scale = float((do.double() * o2.double()).abs().sum())
    print(f"attention dropout on the padded grid: <do, o(v')> {float(lhs):.9e}  <dv, v'> {float(rhs):.9e}  sum of magnitudes {scale:.3e}")
    assert abs(float(lhs - rhs)) <= 2e-5 * scale


# ------------------------------------------------------------------ the captured step
def _eager_step(npvp, m, opt, past, fut):
    """one eager step in the schedule the capture uses (no gradient stream)"""
    ops = npvp.ops
    with ops.use(opt.ctx):
        ops.WgradStream.join()
        two = ops.WgradStream.enabled
        ops.WgradStream.enabled = False
        try:
            return npvp.predictor_train_step(m, opt, past, fut, 0.01, 1e-6, 1.0, sync=False)
        finally:
            ops.WgradStream.enabled = two


def test_captured_step_has_no_memset_node_and_replays_the_eager_step(npvp):
    p = WC.PRED
    past = O.synth_features((p["N"], p["To"], 512, p["H"], p["W"]), 501).to(DEV)
    fut = O.synth_features((p["N"], p["Tp"], 512, p["H"], p["W"]), 502).to(DEV)
    runs = {}
    for graphed in (False, True):
        m = WC.small_predictor(npvp, 503, DEV, evt_layers=1, dec_layers=1)
        m.train()
        opt = npvp.FlatAdamW(m, lr=1e-4, clip_module=m.transformer, max_grad_norm=1.0)
        _eager_step(npvp, m, opt, past, fut)                 # step 1, eager in both runs
        if graphed:
            # warmup = 0: the model has been stepped, the capture executes nothing; step 2 is the first replay
            step = npvp.GraphedTrainStep(m, opt, past, fut, 0.01, 1e-6, 1.0, warmup=0)
            assert step.census["kernel"] > 100 and step.census.get("memset", 0) == 0, step.census
            out = step(past, fut)
        else:
            out = _eager_step(npvp, m, opt, past, fut)
        torch.cuda.synchronize()
        runs[graphed] = (opt.flat_p.clone(), float(out["loss"]))
    (pe, le), (pg, lg) = runs[False], runs[True]
    assert le == lg, (le, lg)
    assert torch.equal(pe, pg), f"replay vs eager parameters: rel-L2 {float((pe - pg).norm() / pe.norm()):.3e}"
