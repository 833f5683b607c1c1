"""GPU: the stochastic predictor as a sampler - S futures per clip, the context encoded once.
  * npvp_reparam_samples (csrc/sample.hip) against a numpy restatement of its header comment, its bit-level contracts (seed, salt,
    chunking) and the statistics of 2^20 draws;
  * npvp_attn_samples_fwd (csrc/attn.hip) against npvp_attn_fwd on every sample's slab with the same K / V: equal to the bit;
  * ops.cross_attn_samples against the existing sub-layer on replicated key / memory, the long routes included;
  * Predictor.sample against the CPU oracle and against S eval forwards, chunked sampling, one encoder pass, best-of-S metrics.
All shapes are 8 x 8 grids or smaller."""
import math

import numpy as np
import pytest
import torch

import golden_cases as GC
from oracle import ops as O
from sampling_cases import gauss_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-4          # the suite's bar (tests/test_hip_golden.py::test_predictor)
C, HEADS = 512, 8


@pytest.fixture(scope="module")
def K():
    import npvp_amd  # noqa: F401
    from npvp_amd import ops
    assert torch.cuda.is_available()
    ops.rng.manual_seed(1234, torch.device(DEV))
    ops.set_gemm_precision("f16x3")
    return ops


def seed_t(v):
    return torch.full((1,), v, dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------- 1. - 4. the latent sampler
@pytest.mark.parametrize("numel", [1000, 1003, 3])       # 1000: vector stores; 1003: scalar stores and a 3-element tail; 3: tail only
def test_sampler_formula(K, numel):
    """max |eps - formula| <= 1e-5: fp32 rounding of 2 pi u2 (<= 3.7e-7) times the largest radius 5.77 = 2.2e-6, a few ulp of a value
    <= 5.77 another 2e-6, doubled"""
    S, base, seed, salt = 3, 2, 0x1234567887654321, 77
    z0 = torch.zeros(numel, device=DEV)
    z, eps = K.reparam_samples(z0, z0, S, seed_t(seed), salt, sample_base=base, return_eps=True)
    assert z.shape == eps.shape == (S, numel)
    want = gauss_ref(seed, salt, numel, S, base)
    got = eps.double().cpu().numpy()
    assert np.isfinite(got).all() and np.abs(got).max() <= 5.78
    err = np.abs(got - want).max()
    print(f"numel {numel}: max abs error {err:.3e}")
    assert err <= 1e-5


@pytest.mark.parametrize("numel", [4096, 1003])
def test_sampler_bits(K, numel):
    mu = torch.zeros(numel, device=DEV)
    a = K.reparam_samples(mu, mu, 8, seed_t(5), 9, return_eps=True)
    b = K.reparam_samples(mu, mu, 8, seed_t(5), 9, return_eps=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                       # the same seed twice
    assert torch.equal(a[0], a[1])                                                   # mu = 0, logvar = 0: z is eps
    assert not torch.equal(a[1], K.reparam_samples(mu, mu, 8, seed_t(6), 9, return_eps=True)[1])      # another seed
    assert not torch.equal(a[1], K.reparam_samples(mu, mu, 8, seed_t(5 + (1 << 32)), 9, return_eps=True)[1])      # ... in its high word
    assert not torch.equal(a[1], K.reparam_samples(mu, mu, 8, seed_t(5), 10, return_eps=True)[1])     # another salt
    part = K.reparam_samples(mu, mu, 2, seed_t(5), 9, sample_base=3, return_eps=True)
    assert torch.equal(part[1], a[1][3:5]) and torch.equal(part[0], a[0][3:5])       # samples 3..4, whatever S and the cut
    assert torch.equal(K.reparam_samples(mu, mu, 8, seed_t(5), 9), a[0])             # eps_out is optional


def test_sampler_relation(K):
    """|z - (mu + exp(0.5 logvar) eps)| <= 1e-6 (|mu| + |exp(0.5 logvar) eps|): exp with its argument rounding <= 2 ulp, one multiply,
    one add, together <= 4 * 2^-24 = 2.4e-7, rounded up"""
    shape = (3, 37, 512)
    mu = O.seeded_randn(shape, 11).to(DEV)
    lv = (torch.rand(shape, generator=torch.Generator().manual_seed(12)) * 6 - 4).to(DEV)
    z, eps = K.reparam_samples(mu, lv, 4, seed_t(99), 3, return_eps=True)
    assert z.shape == (4,) + shape
    m, s = mu.double(), torch.exp(0.5 * lv.double())
    want = m + s * eps.double()
    bound = 1e-6 * (m.abs() + (s * eps.double()).abs())
    excess = ((z.double() - want).abs() - bound).max().item()
    print(f"largest |z - want| - bound: {excess:.3e}")
    assert excess <= 0


def test_sampler_statistics(K):
    """2^20 draws; every bound is 5 sigma of its estimator at n = 2^20"""
    numel, S = 1 << 18, 4
    n = float(numel * S)
    z0 = torch.zeros(numel, device=DEV)
    eps = K.reparam_samples(z0, z0, S, seed_t(2024), 1, return_eps=True)[1].double()
    mean, var = eps.mean().item(), eps.var(unbiased=False).item()
    tail = (eps.abs() > 3).double().mean().item()
    p3 = math.erfc(3 / math.sqrt(2))                       # 0.0027
    cs = (eps[:-1] * eps[1:]).mean().item()                # sample s against s + 1, same element
    ce = (eps[:, :-1] * eps[:, 1:]).mean().item()          # element i against i + 1, same sample
    print(f"mean {mean:.3e} var-1 {var - 1:.3e} tail {tail:.5f} corr_s {cs:.3e} corr_e {ce:.3e}")
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)
    assert abs(tail - p3) <= 5 * math.sqrt(p3 * (1 - p3) / n)
    assert abs(cs) <= 5 / math.sqrt(n) and abs(ce) <= 5 / math.sqrt(n)


# ------------------------------------------------------------------------------- 5. attention on shared K / V
def _attn_inputs(N, S, P, Tq, Tk, wide):
    """q [S N Tq P, C], k, v [N Tk P, C] (wide: column slices of [rows, 3C] buffers, as the packed projections are) and two outputs"""
    rq, rk = S * N * Tq * P, N * Tk * P
    if wide:
        bq = O.seeded_randn((rq, 3 * C), 31).to(DEV)
        bk = O.seeded_randn((rk, 3 * C), 32).to(DEV)
        q, k, v = bq[:, C:2 * C], bk[:, :C], bk[:, 2 * C:]
        o1, o2 = (torch.full((rq, 3 * C), 7.0, device=DEV)[:, C:2 * C] for _ in range(2))
    else:
        q = O.seeded_randn((rq, C), 31).to(DEV)
        k, v = O.seeded_randn((rk, C), 32).to(DEV), O.seeded_randn((rk, C), 33).to(DEV)
        o1, o2 = (torch.full((rq, C), 7.0, device=DEV) for _ in range(2))
    return q, k, v, o1, o2


def _check_samples_attn(K, N, S, P, Tq, Tk, chunk=0, wide=False):
    from npvp_amd._lib import lib, check
    from npvp_amd.sched import AmaxSlot, _stream
    L = lib()
    q, k, v, o_new, o_old = _attn_inputs(N, S, P, Tq, Tk, wide)
    s_new, s_old = AmaxSlot.new(torch.device(DEV)), AmaxSlot.new(torch.device(DEV))
    check(L.npvp_attn_samples_fwd(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), o_new.data_ptr(),
                                  o_new.stride(0), S, N, P, Tq, Tk, HEADS, 64, chunk, s_new.data_ptr(), _stream()), "npvp_attn_samples_fwd")
    rows = N * Tq * P
    for s in range(S):          # the existing kernel on this sample's slab, the same K / V, one slot for all the launches
        check(L.npvp_attn_fwd(q.data_ptr() + 4 * s * rows * q.stride(0), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                              o_old.data_ptr() + 4 * s * rows * o_old.stride(0), o_old.stride(0), 1, N, P, P, 0, Tq, Tk, HEADS, 64, 0, 0.0,
                              None, 0, s_old.data_ptr(), _stream()), "npvp_attn_fwd")
    for s in range(S):
        assert torch.equal(o_new[s * rows:(s + 1) * rows], o_old[s * rows:(s + 1) * rows]), f"sample {s} differs"
    assert s_new.read() == s_old.read() == float(o_old.abs().max())
    if wide:                    # nothing outside the column slice was written
        assert bool((o_new._base[:, :C] == 7.0).all()) and bool((o_new._base[:, 2 * C:] == 7.0).all())


SHAPES = [(1, 1, 6, 4, 3), (2, 3, 6, 4, 3), (2, 5, 6, 17, 16), (1, 4, 5, 32, 32), (2, 2, 6, 1, 1), (1, 3, 6, 20, 10)]


@pytest.mark.parametrize("N,S,P,Tq,Tk", SHAPES)
def test_attn_samples_equals_existing_kernel(K, N, S, P, Tq, Tk):
    _check_samples_attn(K, N, S, P, Tq, Tk)


def test_attn_samples_forced_ragged_chunk(K):
    _check_samples_attn(K, 2, 5, 6, 17, 16, chunk=2)


def test_attn_samples_library_chunks_above_one(K):
    """enough waves for the library's own rule to put several samples on a wave (N P heads S / 4096 > 1), ragged last chunk"""
    _check_samples_attn(K, 2, 11, 64, 4, 3)


def test_attn_samples_column_slices(K):
    _check_samples_attn(K, 2, 3, 6, 4, 3, wide=True)


@pytest.mark.parametrize("Tq,Tk", [(33, 3), (3, 33)])
def test_attn_samples_refuses_long_sequences(K, Tq, Tk):
    from npvp_amd._lib import lib, check
    from npvp_amd.sched import _stream
    q, k, v, o, _ = _attn_inputs(1, 2, 6, Tq, Tk, False)
    with pytest.raises(RuntimeError, match=r"attn_samples: sequence length must be in \[1,32\]"):
        check(lib().npvp_attn_samples_fwd(q.data_ptr(), C, k.data_ptr(), C, v.data_ptr(), C, o.data_ptr(), C, 2, 1, 6, Tq, Tk, HEADS, 64, 0,
                                          None, _stream()), "npvp_attn_samples_fwd")
    assert bool((o == 7.0).all())


# ------------------------------------------------------------------------------- 6. the sub-layer against replication
@pytest.fixture(scope="module")
def dec_block(K):
    import npvp_amd
    m = npvp_amd.VidHRFormerBlockDecNAR(8, 8, 512, 8, 4, 0.0, 0.0, 4, 1024)
    O.key_hashed_fill(m, 61)
    return m.to(DEV).eval()


@pytest.mark.parametrize("N,S,Tq,Tk,H", [(2, 3, 4, 3, 8), (1, 2, 33, 5, 2), (1, 2, 129, 3, 2)])
def test_cross_attn_samples_vs_replication(K, dec_block, N, S, Tq, Tk, H):
    """(.., 33, 5) takes the generic kernels, (.., 129, 3) the streaming ones, each through the per-sample loop"""
    from npvp_amd.ops import AttnCfg, Drop
    P = H * H
    x = (0.3 * O.seeded_randn((S * N, Tq, H, H, C), 41)).to(DEV)
    add = (0.5 * O.seeded_randn((S * N, H, H, C), 42)).to(DEV)
    key = O.seeded_randn((N, Tk, H, H, C), 43).to(DEV)
    mem = O.seeded_randn((N, Tk, H, H, C), 44).to(DEV)
    beta = (0.5 * O.seeded_randn((Tq * P, C), 45)).to(DEV)
    with torch.no_grad():
        got = K.cross_attn_samples(x, dec_block.norm5, beta, None, add, key, mem, dec_block.EncDecAttn,
                                   AttnCfg(1, N, P, H, 0, Tq, Tk, HEADS, 0, 0.0), S, N, Tq)
        want = K.cross_attn_sublayer(x, dec_block.norm5, beta, None, add, key.repeat(S, 1, 1, 1, 1), mem.repeat(S, 1, 1, 1, 1),
                                     dec_block.EncDecAttn, AttnCfg(1, S * N, P, H, 0, Tq, Tk, HEADS, 0, 0.0), Drop(0.0), S * N, Tq)
    assert got.shape == want.shape == x.shape
    e = GC.rel_err(got, want)
    print(f"rel-L2 {e:.3e}")
    assert e <= TOL


def test_cross_attn_samples_refuses_grad(K, dec_block):
    from npvp_amd.ops import AttnCfg
    x = torch.zeros(2, 2, 8, 8, C, device=DEV, requires_grad=True)
    z = torch.zeros(1, 2, 8, 8, C, device=DEV)
    with pytest.raises(RuntimeError, match="forward only"):
        K.cross_attn_samples(x, dec_block.norm5, torch.zeros(2 * 64, C, device=DEV), None, None, z, z, dec_block.EncDecAttn,
                             AttnCfg(1, 1, 64, 8, 0, 2, 2, HEADS, 0, 0.0), 2, 1, 2)


# ------------------------------------------------------------------------------- 7. - 10. end to end
N_, TO, TP, S_ = 2, 3, 4, 3


@pytest.fixture(scope="module")
def sampled(K):
    """the HIP predictor, its input and ONE Predictor.sample(S = 3) with the calls of _encode / the prior head counted: shared, unchanged"""
    import npvp_amd
    m = GC._small_predictor(npvp_amd, True, 91, DEV)
    past = O.synth_features((N_, TO, 512, 8, 8), 92)
    calls = {"encode": 0, "prior": 0}
    enc0, pri0 = m._encode, m.evt_prior.forward_canonical

    def enc(*a, **k):
        calls["encode"] += 1
        return enc0(*a, **k)

    def pri(*a, **k):
        calls["prior"] += 1
        return pri0(*a, **k)

    m._encode, m.evt_prior.forward_canonical = enc, pri
    m.evt_prior.eps_fn = lambda shape: pytest.fail("Predictor.sample consulted eps_fn")
    m.train()
    try:
        out, eps = m.sample(past.to(DEV), S_, seed=4321, return_eps=True)
        was_training = m.training
    finally:
        del m._encode, m.evt_prior.forward_canonical
        m.evt_prior.eps_fn = None
    m.eval()
    return m, past, out, eps, dict(calls), was_training


def _oracle_layout(eps_s):
    """[N, H*W, C] canonical -> the reference's (N, C, H, W)"""
    return eps_s.transpose(1, 2).reshape(eps_s.shape[0], 512, 8, 8).contiguous()


def test_sample_vs_oracle(K, sampled):
    import oracle
    m, past, out, eps, calls, was_training = sampled
    assert out.shape == (N_, S_, TP, 512, 8, 8) and eps.shape == (S_, N_, 64, 512)
    assert was_training, "the module's training flag is restored"
    ref = GC._small_predictor(oracle, True, 91, "cpu").eval()
    for s in range(S_):
        e_s = _oracle_layout(eps[s].cpu())
        ref.evt_prior.eps_fn = lambda shape: e_s
        with torch.no_grad():
            want = ref(past)
        worst = GC.compare({"y": out[:, s]}, {"y": want.numpy()}, TOL, tag=f"sample{s}")
        print(f"sample {s}: rel-L2 {worst:.3e}")


def test_sample_refuses_deterministic_predictor(K):
    import npvp_amd
    m = GC._small_predictor(npvp_amd, False, 91, DEV, evt_layers=1, dec_layers=1)
    with pytest.raises(ValueError, match="stochastic"):
        m.sample(torch.zeros(1, TO, 512, 8, 8, device=DEV), 2)


def test_sample_vs_eval_forwards(K, sampled):
    m, past, out, eps, calls, _ = sampled
    p = past.to(DEV)
    try:
        for s in range(S_):
            e_s = _oracle_layout(eps[s])
            m.evt_prior.eps_fn = lambda shape: e_s
            with torch.no_grad():
                want = m(p)
            e = GC.rel_err(out[:, s], want)
            print(f"sample {s}: rel-L2 {e:.3e}")
            assert e <= TOL
    finally:
        m.evt_prior.eps_fn = None


def test_one_encoder_pass(K, sampled):
    assert sampled[4] == {"encode": 1, "prior": 1}


def test_sample_is_reproducible_and_seeded(K, sampled):
    m, past, out, eps, _, _ = sampled
    p = past.to(DEV)
    again, eps2 = m.sample(p, S_, seed=4321, return_eps=True)
    assert torch.equal(eps2, eps) and torch.equal(again, out)
    assert not torch.equal(m.sample(p, 1, seed=4322, return_eps=True)[1], eps[:1])
    ctx_seed = K.current().rng.seed_tensor(torch.device(DEV)).clone()
    a = m.sample(p, 1, return_eps=True)[1]                      # seed None: the scheduling context's device seed ...
    assert torch.equal(K.current().rng.seed_tensor(torch.device(DEV)), ctx_seed)        # ... read, not changed
    z0 = torch.zeros(N_, 64, 512, device=DEV)
    assert torch.equal(a, K.reparam_samples(z0, z0, 1, ctx_seed, m.SAMPLE_SALT, return_eps=True)[1])


def test_chunked_sampling(K, sampled):
    import npvp_amd
    m, past, _, _, _, _ = sampled
    p = past.to(DEV)
    calls = []
    enc0 = m._encode
    m._encode = lambda *a, **k: (calls.append(1), enc0(*a, **k))[1]
    try:
        whole = npvp_amd.predictor_sample_step(m, p, 4, seed=77, return_eps=True)
        n_whole = len(calls)
        cut = npvp_amd.predictor_sample_step(m, p, 4, seed=77, chunk=2, return_eps=True)
        ragged = npvp_amd.predictor_sample_step(m, p, 4, seed=77, chunk=3, return_eps=True)
    finally:
        del m._encode
    assert n_whole == 1 and len(calls) == 3, "the encoder runs once per step, whatever the cut"
    assert whole[0].shape == cut[0].shape == (N_, 4, TP, 512, 8, 8)
    for other in (cut, ragged):
        assert torch.equal(other[1], whole[1]) and torch.equal(other[2], whole[2])          # eps and z: equal to the bit
        e = GC.rel_err(other[0], whole[0])
        print(f"rel-L2 {e:.3e}")
        assert e <= 1e-4
    assert torch.equal(npvp_amd.predictor_sample_step(m, p, 4, seed=77), whole[0])
    assert not m.training


# ------------------------------------------------------------------------------- 11. - 12. best of S
def _planted():
    """N = 2, S = 3, T = 2: sample 1 of clip 0 and sample 2 of clip 1 are the target"""
    g = torch.Generator().manual_seed(5)
    target = torch.rand((2, 2, 3, 32, 32), generator=g)
    pred = (target[:, None] + 0.2 * torch.randn((2, 3, 2, 3, 32, 32), generator=g)).clamp(0, 1)
    pred[0, 1], pred[1, 2] = target[0], target[1]
    return pred.to(DEV), target.to(DEV)


def _metric_cases():
    from npvp_amd import metrics as M
    return [(M.SSIM(), True), (M.PSNR, True), (M.MSEScore, False)]


def test_best_of_samples(K):
    from npvp_amd import metrics as M
    pred, target = _planted()
    for fn, hib in _metric_cases():
        idx, best, every = M.best_of_samples(pred, target, fn, higher_is_better=hib)
        assert idx.is_cuda and best.is_cuda and every.is_cuda
        assert idx.tolist() == [1, 2] and best.shape == (2, 2) and every.shape == (2, 3, 2)
        for s in range(3):
            for t in range(2):          # the existing per-image call on the same slab
                assert torch.equal(every[:, s, t], fn(pred[:, s, t], target[:, t], mean_flag=False))
        assert torch.equal(best[0], every[0, 1]) and torch.equal(best[1], every[1, 2])
    tie = pred.clone()
    tie[:, 2] = tie[:, 0]                                       # two identical samples, neither the planted one ...
    tie[:, 1] = 1.0 - tie[:, 1]                                 # ... which is made worse than both (the negative image)
    idx, _, every = M.best_of_samples(tie, target, M.PSNR)
    assert torch.equal(every[:, 0], every[:, 2]) and idx.tolist() == [0, 0]


def test_pred_best_metrics(K):
    from npvp_amd import metrics as M
    pred, target = _planted()
    seen = []

    class Stub(torch.nn.Module):
        def sample(self, past, n_samples, seed=None, sample_base=0):
            seen.append((n_samples, seed, sample_base))
            return pred[int(past[0, 0]):int(past[0, 0]) + 1]

    loader = [(torch.full((1, 1), float(i)), target[i:i + 1].cpu()) for i in range(2)]
    for fn, hib in _metric_cases():
        got = M.pred_best_metrics(Stub(), loader, fn, lambda x: x, 2, 3, 11, higher_is_better=hib, device=DEV)
        _, best, _ = M.best_of_samples(pred, target, fn, higher_is_better=hib)
        assert got.shape == (2,) and np.allclose(got, best.double().mean(0).cpu().numpy(), rtol=1e-6, atol=0)
    assert seen[:2] == [(3, 11, 0), (3, 11, 3)]
