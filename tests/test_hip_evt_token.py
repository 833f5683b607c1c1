"""GPU: the learned event token of the encoder (ref/models/VidHRFormer.py:22-23, 35-42; ref/models/Predictor.py:343-344): the two copy
kernels alone through the C ABI, the encoder and the predictors D / S against the reference's vectors (tests/golden/evt_token_encoder.npz,
predictor_evt_token_{D,S}.npz), both code paths of the blocks, the generic attention route at T + 1 = 33, token independence of the
memory, DropPath on T + 1 frames, the sampler, the captured step and the checkpoint round trip.

Kernel shapes (N, T, P): one clip of one frame; more than one block per launch (C = 8 puts 128 rows into a block, C = 512 two); a row
count per frame that is no power of two (60) with the token frame far from a block boundary; 33 clips (the clip decode past 32)."""
import functools

import pytest
import torch

import evt_token_cases as EC
import golden_cases as GC
from oracle import ops as O
from test_hip_golden import TOL          # 1e-4: the arithmetic is the same kernels as that suite's

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SUM_TOL = 1e-6                           # sums of products, of the sum of the magnitudes (that suite's bound for reductions)
KERNEL_SHAPES = [(1, 1, 16), (3, 2, 64), (2, 5, 60), (33, 1, 16)]
TOKEN_FORMS = ["shared", "per_clip", "none"]


@pytest.fixture(scope="module")
def npvp():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import npvp_amd
    npvp_amd.ops.set_gemm_precision("f16x3")
    return npvp_amd


@pytest.fixture(scope="module")
def own_context(npvp):
    return npvp.ops.StepContext("evt_token_tests")


@pytest.fixture(autouse=True)
def _in_own_context(npvp, own_context):
    """every test of this file runs under a scheduling context of its own (dropout seed, gradient stream, fp16 range guard): what
    its trainers and seeds do stays out of the process's default context, which the other test files share"""
    with npvp.ops.use(own_context):
        yield


def _st():
    return torch.cuda.current_stream().cuda_stream


def _strided(rows, C, seed):
    """[rows, C] with a padded row stride (ld = C + 8); the gap columns are NaN"""
    buf = torch.full((rows, C + 8), float("nan"), device=DEV)
    buf[:, :C] = O.seeded_randn((rows, C), seed).to(DEV)
    return buf[:, :C]


def _nan_out(rows, C):
    """a NaN-filled [rows, C] view with row stride C + 8 and the buffer it lies in"""
    buf = torch.full((rows, C + 8), float("nan"), device=DEV)
    return buf[:, :C], buf


def _slot():
    return torch.zeros(512, device=DEV)          # an amax slot: 2 KB, zero before its tensor is produced


def _ptr(t):
    return None if t is None else t.data_ptr()


def _join(L, x, token, per_clip, y, N, T, P, slot=None):
    C = y.shape[1]
    rc = L.npvp_evt_token_join(_ptr(x), C if x is None else x.stride(0), _ptr(token), C if token is None else token.stride(0),
                               P * token.stride(0) if per_clip else 0, y.data_ptr(), y.stride(0), N, T, P, C, _ptr(slot), _st())
    assert rc == 0, L.npvp_last_error()


def _split(L, y, x, last, N, T, P, sx=None, sl=None):
    C = y.shape[1]
    rc = L.npvp_evt_token_split(y.data_ptr(), y.stride(0), _ptr(x), C if x is None else x.stride(0), _ptr(last),
                                C if last is None else last.stride(0), N, T, P, C, _ptr(sx), _ptr(sl), _st())
    assert rc == 0, L.npvp_last_error()


def _token(form, N, P, C, seed):
    if form == "none":
        return None
    return _strided((N if form == "per_clip" else 1) * P, C, seed)


def _joined(x, token, form, N, T, P, C):
    """torch.cat of the clips' frames and the token frame"""
    if form == "none":
        tok = torch.zeros(N, 1, P, C, device=DEV)
    elif form == "per_clip":
        tok = token.reshape(N, 1, P, C)
    else:
        tok = token.reshape(1, 1, P, C).expand(N, 1, P, C)
    return torch.cat([x.reshape(N, T, P, C), tok], dim=1).reshape(N * (T + 1) * P, C)


@pytest.mark.parametrize("form", TOKEN_FORMS)
@pytest.mark.parametrize("C", [512, 8])
@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_join_kernel_equals_cat(npvp, shape, C, form):
    from npvp_amd._lib import lib
    L = lib()
    N, T, P = shape
    x = _strided(N * T * P, C, 5 + C + P)
    token = _token(form, N, P, C, 6 + C + P)
    want = _joined(x, token, form, N, T, P, C)
    src_max = max(float(x.abs().max()), 0.0 if token is None else float(token.abs().max()))
    outs = []
    for _ in range(2):
        y, buf = _nan_out(N * (T + 1) * P, C)
        slot = _slot()
        _join(L, x, token, form == "per_clip", y, N, T, P, slot)
        torch.cuda.synchronize()
        assert not torch.isnan(y).any(), "an element of y was not written"
        assert torch.isnan(buf[:, C:]).all(), "the kernel wrote outside the C columns of a row"
        assert torch.equal(y, want)
        assert float(y.abs().max()) <= float(slot.max()) <= src_max
        outs.append(y.clone())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("outputs", ["both", "x", "last"])
@pytest.mark.parametrize("C", [512, 8])
@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_split_kernel_equals_slicing(npvp, shape, C, outputs):
    from npvp_amd._lib import lib
    L = lib()
    N, T, P = shape
    y = _strided(N * (T + 1) * P, C, 9 + C + P)
    y4 = y.reshape(N, T + 1, P, C)
    want_x, want_last = y4[:, :T].reshape(N * T * P, C), y4[:, T].reshape(N * P, C)
    outs = []
    for _ in range(2):
        (x, xbuf), (last, lbuf) = _nan_out(N * T * P, C), _nan_out(N * P, C)
        sx, sl = _slot(), _slot()
        _split(L, y, x if outputs != "last" else None, last if outputs != "x" else None, N, T, P, sx, sl)
        torch.cuda.synchronize()
        for name, got, buf, want, slot in (("x", x, xbuf, want_x, sx), ("last", last, lbuf, want_last, sl)):
            if outputs not in ("both", name):
                assert torch.isnan(buf).all() and float(slot.max()) == 0.0, f"{name} was not asked for and was touched"
                continue
            assert not torch.isnan(got).any(), f"an element of {name} was not written"
            assert torch.isnan(buf[:, C:]).all(), "the kernel wrote outside the C columns of a row"
            assert torch.equal(got, want)
            assert float(got.abs().max()) <= float(slot.max()) <= float(y.abs().max())
        outs.append((x.clone(), last.clone()))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))


@pytest.mark.parametrize("form", TOKEN_FORMS)
@pytest.mark.parametrize("shape", KERNEL_SHAPES)
def test_join_and_split_are_adjoint(npvp, shape, form):
    """<join(x, e), y> == <x, split_x(y)> + <e, sum_n split_last(y)> (per clip: no sum; no token: no second term): both sides sum the
    same products - the kernels copy - so accumulated in float64 they differ by the rounding of the summation orders only: 2^-53 per
    addition, bounded here by 1e-12 of the sum of the magnitudes"""
    from npvp_amd._lib import lib
    L = lib()
    N, T, P = shape
    C = 512
    x, y = O.seeded_randn((N * T * P, C), 21).to(DEV), O.seeded_randn((N * (T + 1) * P, C), 22).to(DEV)
    e = None if form == "none" else O.seeded_randn(((N if form == "per_clip" else 1) * P, C), 23).to(DEV)
    jy = torch.empty(N * (T + 1) * P, C, device=DEV)
    sx, sl = torch.empty(N * T * P, C, device=DEV), torch.empty(N * P, C, device=DEV)
    _join(L, x, e, form == "per_clip", jy, N, T, P)
    _split(L, y, sx, sl, N, T, P)
    lhs = (jy.double() * y.double()).sum()
    rhs, scale = (x.double() * sx.double()).sum(), (x.double() * sx.double()).abs().sum()
    if e is not None:
        g = sl.double().reshape(N, P, C) if form == "per_clip" else sl.double().reshape(N, P, C).sum(0, keepdim=True)
        rhs = rhs + (e.double().reshape(g.shape) * g).sum()
        scale = scale + (e.double().reshape(1 if form == "shared" else N, P, C).abs() * sl.double().reshape(N, P, C).abs()).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * float(scale)


def test_shared_token_gradient_is_the_fixed_order_sum(npvp):
    """ops.evt_token_join's backward: dEVT = npvp_reduce_mid over the clips of the split's `last` - against a float64 sum at the
    reductions' bound, and equal in two runs"""
    ops = npvp.ops
    N, T = 5, 2
    x = O.seeded_randn((N, T, 8, 8, 512), 31).to(DEV).requires_grad_()
    tok = O.seeded_randn((1, 8, 8, 512), 32).to(DEV).requires_grad_()
    cot = O.seeded_randn((N, T + 1, 8, 8, 512), 33).to(DEV)
    runs = []
    for _ in range(2):
        y = ops.evt_token_join(x, tok)
        gx, gt = torch.autograd.grad((y * cot).sum(), [x, tok])
        runs.append((y.detach(), gx, gt))
    assert torch.equal(runs[0][0], torch.cat([x.detach(), tok.detach().expand(N, 8, 8, 512).unsqueeze(1)], dim=1))
    assert torch.equal(runs[0][1], cot[:, :T])
    want = cot[:, T].double().sum(0, keepdim=True)
    assert float((runs[0][2].double() - want).abs().sum()) <= SUM_TOL * float(cot[:, T].double().abs().sum())
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))


# ------------------------------------------------------------------ the encoder alone
def _bad(errs, tol=TOL):
    return {k: f"{e:.3e}" for k, e in errs.items() if not e < tol}


@functools.lru_cache(maxsize=None)
def _encoder_on_the_device(fuser_kind):
    """the HIP encoder on the fixture's case, with the stock fuser (sub-layer nodes) or a subclass of it (per-kernel path): computed
    once, never modified"""
    import npvp_amd

    class OwnFuser(npvp_amd.PosFeatFuser):          # not the stock class: the blocks run their per-kernel path
        pass
    fuser = (npvp_amd.PosFeatFuser if fuser_kind == "stock" else OwnFuser)(512, 'layer')
    return {k: v.detach().cpu() for k, v in EC.case_encoder(npvp_amd, DEV, fuser).items()}


def test_encoder_against_the_reference(npvp):
    golden = GC.load("evt_token_encoder")
    got = _encoder_on_the_device("stock")
    errs = {k: GC.rel_err(EC.view(got[k]), golden[k]) for k in EC.ENC_KEYS}
    print(f"evt token encoder: {errs}")
    assert not _bad(errs), f"rel-L2 above {TOL:.1e}: {_bad(errs)}"


def test_encoder_in_both_code_paths(npvp):
    """the stock fuser takes the sub-layer nodes, a subclass of it the per-kernel autograd path: the two agree with each other and each
    with the CPU restatement"""
    want = {k: v.detach() for k, v in EC.case_encoder_restated().items()}
    nodes, kernels = _encoder_on_the_device("stock"), _encoder_on_the_device("own")
    bad = {}
    for tag, a, b in (("nodes-vs-kernels", nodes, kernels), ("nodes-vs-restatement", nodes, want), ("kernels-vs-restatement", kernels, want)):
        errs = {k: GC.rel_err(a[k], b[k]) for k in EC.ENC_KEYS}
        print(f"evt token encoder {tag}: {errs}")
        bad.update({f"{tag}.{k}": v for k, v in _bad(errs).items()})
    assert not bad, f"rel-L2 above {TOL:.1e}: {bad}"


def _generic_case(impl, dev, restated):
    """N 2, T 32 on a 4 x 4 grid, one layer: T + 1 = 33 key rows"""
    N, T, Hh = 2, 32, 4
    enc = impl.VidHRFormerEncoder(1, Hh, Hh, 512, 8, 4, 0.0, 0.0, 4, 1024, torch.nn.LayerNorm(512), not restated)
    if restated:
        enc.register_parameter("EVT", torch.nn.Parameter(torch.zeros(1, Hh, Hh, 512)))
    EC.fill(enc, 641, 642)
    enc = enc.to(dev)
    fuser = impl.PosFeatFuser(512, 'layer')
    x = O.synth_features((N, T, 512, Hh, Hh), 643).to(dev).requires_grad_()
    beta = (0.5 * O.seeded_randn((T * Hh * Hh, 512), 644)).to(dev).requires_grad_()
    cot = O.seeded_randn((N, T + 1, 512, Hh, Hh), 645).to(dev)
    if restated:
        mem, evt = EC.restated_encode(EC._Holder(enc, fuser), x, (beta, None), enc.EVT)
    else:
        y = enc(x, (beta, None), fuser)
        mem, evt = y[:, :-1], y[:, -1]
    g = torch.autograd.grad((mem * cot[:, :T]).sum() + (evt * cot[:, T]).sum(), [x, enc.EVT, beta])
    return dict(zip(("memory", "evt", "g_x", "g_EVT", "g_beta"), (t.detach().cpu() for t in (mem, evt, *g))))


def test_generic_attention_route_at_33_frames(npvp):
    """T + 1 = 33 is past the MFMA temporal kernels' 32 rows, and a 4 x 4 grid is not the fused MlpDWBN's: the generic attention route and
    the per-kernel MlpDWBN route carry the token too"""
    import oracle
    ops = npvp.ops
    assert not ops.mlpdwbn_fused_supported(2 * 33 * 16, 512, 2048, 512, 4, 4)
    assert (L_route(ops, 32), L_route(ops, 33)) == ("mfma", "generic")
    want = _generic_case(oracle, "cpu", True)
    got = _generic_case(npvp, DEV, False)
    errs = {k: GC.rel_err(got[k], want[k]) for k in want}
    print(f"evt token encoder, 33 frames on 4 x 4: {errs}")
    assert not _bad(errs), f"rel-L2 above {TOL:.1e}: {_bad(errs)}"


def L_route(ops, T):
    """which temporal attention kernels take T key rows: "mfma" up to 32, "generic" 33 .. 128, "streaming" above"""
    cfg = ops.AttnCfg(1, 2, 16, 4, 0, T, T, 8, 1, 0.0)
    return "streaming" if ops._attn_long(cfg) else ("mfma" if max(ops._attn_len(cfg)) <= 32 else "generic")


def test_memory_hardly_depends_on_the_token(npvp):
    """the frames never see the token: EVT -> 3 EVT + 1 moves the memory by less than TOL (it need not be zero: the per-tensor operand
    scales of the fp16 GEMMs see the token's rows) and the event coding by more than 10 x TOL"""
    e = EC.ENC
    m = npvp.VidHRFormerEncoder(e["layers"], 8, 8, 512, 8, 4, 0.0, 0.0, 4, 1024, torch.nn.LayerNorm(512), True)
    EC.fill(m, e["fill"], e["token"])
    m = m.to(DEV)
    x, beta, gamma, _, _ = EC.encoder_inputs(DEV)
    fuser = npvp.PosFeatFuser(512, 'layer')
    with torch.no_grad():
        y1 = m(x, (beta, gamma), fuser)
        m.EVT.mul_(3.0).add_(1.0)
        y2 = m(x, (beta, gamma), fuser)
    e_mem, e_evt = GC.rel_err(y2[:, :-1], y1[:, :-1]), GC.rel_err(y2[:, -1], y1[:, -1])
    print(f"EVT -> 3 EVT + 1: memory moves by {e_mem:.3e}, event coding by {e_evt:.3e}")
    assert e_mem < TOL and e_evt > 10 * TOL


# ------------------------------------------------------------------ DropPath on T + 1 frames
def test_drop_path_sites_and_sample_skip_see_all_frames(npvp):
    """drop_path = 0.5, a fixed seed, 4 clips: the block's row-group Drop (the object the backward replays) keys one decision per clip
    over (T + 1) P rows, the MlpDWBN node is told T + 1 frames per sample, and the run that leaves out the dropped samples' work (frame counts per sample in
    the MlpDWBN node, its GEMM tiles) equals the run that does not within 2e-6, the bound tests/test_hip_droppath_skip.py holds the
    same pair to (what moves is a power-of-two operand scale that now sees zeros), in the output and every gradient"""
    ops = npvp.ops
    dev = torch.device(DEV)
    N, T, P = 4, 2, 64
    m = npvp.VidHRFormerEncoder(1, 8, 8, 512, 8, 4, 0.0, 0.5, 4, 1024, torch.nn.LayerNorm(512), True)
    EC.fill(m, 651, 652)
    m = m.to(DEV).train()
    fuser = npvp.PosFeatFuser(512, 'layer')
    x = O.synth_features((N, T, 512, 8, 8), 653).to(DEV).requires_grad_()
    beta = (0.5 * O.seeded_randn((T * P, 512), 654)).to(DEV).requires_grad_()
    cot = O.seeded_randn((N, T + 1, 512, 8, 8), 655).to(DEV)
    leaves = [x, m.EVT, beta, m.layers[0].SpatialFFN.fc1.weight, m.layers[0].SLMHSA.attn.in_proj_bias]

    def run(skip, seed=77):
        keep = ops.DROP_PATH_SKIP
        ops.DROP_PATH_SKIP = skip
        try:
            ops.rng.manual_seed(seed, dev)
            ops.rng.begin_step(dev)
            y = m(x, (beta, None), fuser)
            out = [y.detach()] + [t.detach().clone() for t in torch.autograd.grad((y * cot).sum(), leaves)]
            ops.ReduceQueue.finish()
            ops.WgradStream.join()
            torch.cuda.synchronize()
            return out
        finally:
            ops.DROP_PATH_SKIP = keep

    # what the block hands down: its row-group Drop objects (the ones the backward replays) and the MlpDWBN node's frame counts
    import npvp_amd.models.VidHRFormer as V
    seen, real_drop, real_mlp = [], V.Drop, ops.mlpdwbn

    class RecordingDrop(real_drop):
        def __init__(self, p=0.0, mode=0, g1=1, g2=1):
            super().__init__(p, mode, g1, g2)
            if mode == 1:
                seen.append(("drop", p, g1, g2))

    def recording_mlpdwbn(*a):
        seen.append(("mlpdwbn", a[-4], a[-3], a[-1]))          # frames, frames per sample, drop-path probability
        return real_mlp(*a)

    V.Drop, ops.mlpdwbn = RecordingDrop, recording_mlpdwbn
    ops.DropRecorder.sites = []
    try:
        off = run(False)
        sites = [s for s in ops.DropRecorder.sites if s[1] == "group"]
        masks = [ops.DropRecorder.mask(s, dev).cpu() for s in sites]
    finally:
        ops.DropRecorder.sites = None
        V.Drop, ops.mlpdwbn = real_drop, real_mlp
    assert seen == [("drop", 0.5, (T + 1) * P, N), ("mlpdwbn", N * (T + 1), T + 1, 0.5)], seen
    assert len(sites) == 2 and all(count == N for _, _, count in sites), "one decision per clip at the layer's two DropPath sites"
    kept = torch.stack(masks) != 0
    assert bool(kept.any()) and not bool(kept.all()), "seed 77 must keep some samples and drop some (choose another seed)"
    on = run(True)
    again = run(True)
    for name, a, b, c in zip(["y", "g_x", "g_EVT", "g_beta", "g_fc1_w", "g_slmhsa_b"], on, off, again):
        e = float((a.double() - b.double()).norm() / b.double().norm())
        print(f"drop_path 0.5, skip on vs off, {name}: rel-L2 {e:.3e}")
        assert e < 2e-6, f"{name}: rel-L2 {e:.3e}"
        assert torch.equal(a, c), f"{name}: two runs with one seed differ"
    # a sample dropped at both sites only passes through the temporal attention and the token FFN: its input gradient is not zero, but
    # the mask did act - against drop_path = 0 the output moves
    plain = [t for t in run(False, seed=78)]
    assert GC.rel_err(plain[0], off[0]) > 1e-3


# ------------------------------------------------------------------ the whole predictor
@pytest.mark.parametrize("variant", ["D", "S"])
def test_predictor_against_the_reference(npvp, variant):
    golden = GC.load(f"predictor_evt_token_{variant}")
    stochastic = variant == "S"
    m = EC.small_predictor(npvp, stochastic, int(golden["meta"][3]), DEV)
    got = EC.run_predictor(m, stochastic, *EC.predictor_inputs(DEV), npvp.Div_KL(1e-2))
    keys = EC.PRED_KEYS + (EC.PRED_KEYS_S if stochastic else ())
    errs = {k: GC.rel_err(EC.view(got[k]), golden[k]) for k in keys}
    print(f"predictor[{variant}] with the token: {errs}")
    assert set(golden) - {"meta"} == set(errs)
    assert not _bad(errs), f"rel-L2 above {TOL:.1e}: {_bad(errs)}"


@pytest.mark.parametrize("variant", ["D", "S"])
def test_token_gradient_reaches_the_flat_gradient_buffer(npvp, variant):
    """under FlatAdamW the parameter's .grad is a slice of the flat gradient buffer: after the trainer's own sequence (zero_grad,
    forward, backward) the slice holds the reference's gradient - for S the sum of the context and the target pass"""
    ops = npvp.ops
    stochastic = variant == "S"
    golden = GC.load(f"predictor_evt_token_{variant}")
    m = EC.small_predictor(npvp, stochastic, int(golden["meta"][3]), DEV).train()
    opt = npvp.FlatAdamW(m, lr=1e-4, clip_module=m.transformer, max_grad_norm=1.0)
    past, fut, eps, cot = EC.predictor_inputs(DEV)
    if stochastic:
        m.evt_prior.eps_fn = m.evt_posterior.eps_fn = lambda shape: eps
    with ops.use(opt.ctx):
        opt.zero_grad()
        o = m(past, fut) if stochastic else m(past)
        yt = o[0] if stochastic else o
        loss = (yt * yt * cot).sum() + (npvp.Div_KL(1e-2)(*o[1:]) if stochastic else 0.0)
        loss.backward()
        ops.ReduceQueue.finish()
        ops.WgradStream.join()
    torch.cuda.synchronize()
    tok = m.EVT_Former.EVT
    off, n = opt.offsets[[id(p) for p in opt.params].index(id(tok))]
    assert n == tok.numel() and tok.grad.data_ptr() == opt.flat_g.data_ptr() + 4 * off and tok.data_ptr() == opt.flat_p.data_ptr() + 4 * off
    errs = {"g_EVT": GC.rel_err(EC.view(opt.flat_g[off:off + n]), golden["g_EVT"]), "y_train": GC.rel_err(EC.view(yt), golden["y_train"]),
            "g_nrmlp_B": GC.rel_err(EC.view(m.nrmlp.B.grad), golden["g_nrmlp_B"])}
    print(f"predictor[{variant}] under FlatAdamW: {errs}")
    assert not _bad(errs), f"rel-L2 above {TOL:.1e}: {_bad(errs)}"


def test_evt_coding_forward_keeps_the_reference_signature(npvp):
    """(N,T,C,H,W) -> the memory (N,T,C,H,W) and the event coding (N,C,H,W): the first T frames and the last one of what the encoder's
    own forward returns (ref/models/Predictor.py:342-344) - copies, so equal to the bit"""
    m = EC.small_predictor(npvp, False, 681, DEV, evt_layers=1, dec_layers=1).eval()
    past = EC.predictor_inputs(DEV)[0]
    N, To = past.shape[:2]
    with torch.no_grad():
        beta, gamma = m.nrmlp(m.observed_coor)
        mem, evt = m.evt_coding_forward(past, beta, gamma)
        y = m.EVT_Former(past, (beta, gamma), m.fuser)
    assert mem.shape == (N, To, 512, 8, 8) and evt.shape == (N, 512, 8, 8) and y.shape == (N, To + 1, 512, 8, 8)
    assert torch.equal(mem, y[:, :-1]) and torch.equal(evt, y[:, -1])


def test_sample_equals_eval_forwards_given_the_drawn_eps(npvp):
    """Predictor.sample(S = 2) against per-sample eval forwards with the eps it drew (tests/test_hip_sampling.py's method)"""
    golden = GC.load("predictor_evt_token_S")
    m = EC.small_predictor(npvp, True, int(golden["meta"][3]), DEV).eval()
    past = EC.predictor_inputs(DEV)[0]
    out, eps = m.sample(past, 2, seed=4321, return_eps=True)
    assert out.shape == (EC.PRED["N"], 2, EC.PRED["Tp"], 512, 8, 8) and eps.shape == (2, EC.PRED["N"], 64, 512)
    try:
        for s in range(2):
            e_s = eps[s].transpose(1, 2).reshape(eps.shape[1], 512, 8, 8).contiguous()
            m.evt_prior.eps_fn = lambda shape: e_s
            with torch.no_grad():
                want = m(past)
            e = GC.rel_err(out[:, s], want)
            print(f"sample {s} with the token: rel-L2 {e:.3e}")
            assert e <= TOL
    finally:
        m.evt_prior.eps_fn = None


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


@pytest.mark.parametrize("variant", ["D", "S"])
def test_captured_step_has_no_memset_node_and_replays_the_eager_step(npvp, variant):
    p = EC.PRED
    dev = torch.device(DEV)
    past = O.synth_features((p["N"], p["To"], 512, 8, 8), 661).to(DEV)
    fut = O.synth_features((p["N"], p["Tp"], 512, 8, 8), 662).to(DEV)
    eps = O.seeded_randn((p["N"], 512, 8, 8), 664).to(DEV)
    runs = {}
    for graphed in (False, True):
        m = EC.small_predictor(npvp, variant == "S", 663, DEV, evt_layers=1, dec_layers=1)
        m.train()
        opt = npvp.FlatAdamW(m, lr=1e-4, clip_module=m.transformer, max_grad_norm=1.0)
        if variant == "S":                                   # (one eps for every step of both runs: a read of static memory in the capture)
            m.evt_prior.eps_fn = m.evt_posterior.eps_fn = lambda shape: eps
        npvp.ops.rng.manual_seed(665, dev)
        _eager_step(npvp, m, opt, past, fut)                 # step 1, eager in both runs
        if graphed:
            # warmup = 0: the model has been stepped, the capture executes nothing; step 2 is the first replay
            step = npvp.GraphedTrainStep(m, opt, past, fut, 0.01, 1e-6, 1.0, warmup=0)
            assert step.census["kernel"] > 100 and step.census.get("memset", 0) == 0, step.census
            out = step(past, fut)
        else:
            out = _eager_step(npvp, m, opt, past, fut)
        torch.cuda.synchronize()
        tok = m.EVT_Former.EVT
        runs[graphed] = (opt.flat_p.clone(), float(out["loss"]), tok.detach().clone())
    (pe, le, te), (pg, lg, tg) = runs[False], runs[True]
    fresh = EC.small_predictor(npvp, variant == "S", 663, "cpu", evt_layers=1, dec_layers=1).EVT_Former.EVT
    assert not torch.equal(te.cpu(), fresh.detach()), "two optimiser steps left the token where it was"
    assert le == lg, (le, lg)
    assert torch.equal(pe, pg), f"replay vs eager parameters: rel-L2 {float((pe - pg).norm() / pe.norm()):.3e}"
    assert torch.equal(te, tg)


# ------------------------------------------------------------------ checkpoints
def test_lightning_checkpoint_round_trip_carries_the_token(npvp, tmp_path):
    m = EC.small_predictor(npvp, False, 671, DEV, evt_layers=1, dec_layers=1).train()
    opt = npvp.FlatAdamW(m, lr=1e-4, clip_module=m.transformer, max_grad_norm=1.0)
    past = O.synth_features((1, 2, 512, 8, 8), 672).to(DEV); fut = O.synth_features((1, 2, 512, 8, 8), 673).to(DEV)
    for _ in range(2):
        npvp.predictor_train_step(m, opt, past, fut, 0.01, 1e-6, 1.0)
    sd = opt.state_dict(m)
    names = [n for n, q in m.named_parameters() if q.requires_grad]
    i = names.index("EVT_Former.EVT")
    assert sd["state"][i]["exp_avg"].shape == (1, 8, 8, 512) and float(sd["state"][i]["exp_avg"].abs().sum()) > 0
    assert float(sd["state"][i]["exp_avg_sq"].abs().sum()) > 0 and float(sd["state"][i]["step"]) == 2.0
    stock = torch.optim.AdamW(m.parameters(), lr=1e-4)
    stock.load_state_dict(sd)                                # module.parameters() order: the token's moments land on the token
    assert stock.state[m.EVT_Former.EVT]["exp_avg"].shape == m.EVT_Former.EVT.shape
    path = str(tmp_path / "evt_token.ckpt")
    npvp.save_lightning_checkpoint(path, m, opt=opt, epoch=1, global_step=2, scheduler_T0=150)
    assert "EVT_Former.EVT" in "".join(torch.load(path, weights_only=True)["state_dict"].keys())
    m2 = EC.small_predictor(npvp, False, 999, DEV, evt_layers=1, dec_layers=1)
    opt2 = npvp.FlatAdamW(m2, lr=3e-4, clip_module=m2.transformer, max_grad_norm=1.0)
    assert npvp.load_lightning_checkpoint(path, m2, opt=opt2) == (1, 2)
    assert torch.equal(m2.EVT_Former.EVT, m.EVT_Former.EVT)
    assert torch.equal(opt2.flat_p, opt.flat_p) and torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v)
    a = npvp.predictor_train_step(m, opt, past, fut, 0.01, 1e-6, 1.0)
    b = npvp.predictor_train_step(m2, opt2, past, fut, 0.01, 1e-6, 1.0)
    assert abs(a["loss"] - b["loss"]) <= 1e-6 * abs(a["loss"]) and torch.equal(opt2.flat_p, opt.flat_p)
    # a module without the token refuses the checkpoint's extra key, as torch's strict loading does
    plain = EC.small_predictor(npvp, False, 999, DEV, learn_evt_token=False, evt_layers=1, dec_layers=1)
    with pytest.raises(RuntimeError, match="EVT"):
        npvp.load_lightning_checkpoint(path, plain)
