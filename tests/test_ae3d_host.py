"""CPU: the learn_3d=True autoencoder without a GPU - state-dict keys against the reference's, the stock modules and the float64
restatements of tests/ae3d_cases.py against the reference fixtures (tests/golden/ae3d_*.npz), deliberately wrong references rejected,
the convolution view of the temporal Conv1d, the C ABI's refusals, the frozen pair's folds and the synchronised BatchNorm swap."""
import copy
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import ae3d_cases as AC
import golden_cases as GC
from oracle import ops as O

TOL = 1e-5          # the project's oracle-versus-reference bar (measured worst: tests/golden/AE3D_VS_REFERENCE.txt)
BLOCK_SEED, PAIR_SEED = 310, 410
BLOCKS = [pytest.param(N, T, H, W, cf, id=AC.block_tag(N, T, H, W, cf)) for (N, T, H, W) in AC.BLOCK_CASES for cf in (True, False)]


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    build.build(verbose=False)
    from npvp_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def keys():
    with open(os.path.join(GC.GOLDEN_DIR, "ae3d_keys.json")) as f:
        return json.load(f)


def _block(cf):
    from npvp_amd.models import Factorized3DConvAttn
    return O.key_hashed_fill(Factorized3DConvAttn(AC.BLOCK_C, conv_first=cf, learn_3d=True), BLOCK_SEED)


def _small_pair(npvp_amd, build=None):
    enc, dec = (build or npvp_amd.build_autoencoder)(AC.AE_SMALL, 1)
    O.key_hashed_fill(npvp_amd.AEPair(enc, dec), PAIR_SEED)
    return enc, dec


# ------------------------------------------------------------------------------------------------------------------------ keys
@pytest.mark.parametrize("name,AE", [("small", AC.AE_SMALL), ("ae64", AC.AE64_3D)])
def test_state_dict_keys_are_the_references(keys, name, AE):
    import npvp_amd
    enc, _ = npvp_amd.build_autoencoder(AE, 1)
    sd = enc.state_dict()
    assert {k: list(v.shape) for k, v in sd.items()} == keys[name] and list(sd) == list(keys[name])
    ref_keyed = {k: torch.full(s, 0.25) if not k.endswith("num_batches_tracked") else torch.tensor(3) for k, s in keys[name].items()}
    enc.load_state_dict(ref_keyed, strict=True)
    assert float(enc.res_3dConvAttn_0.attn1d.gamma.detach()) == 0.25 and enc.res_3dConvAttn_0.temporal_conv[0].weight.shape[-1] == 3


def test_modules_follow_the_reference_constructor():
    from npvp_amd.models import NonLocalAttenion1D, Factorized3DConvAttn
    import npvp_amd.models.ResNetAutoEncoder as M
    assert M.NonLocalAttenion1D is NonLocalAttenion1D
    a = NonLocalAttenion1D(64, 8, 2, True, True, nn.BatchNorm1d(64), nn.ReLU())
    assert (a.attn_dim, a.value_dim, a.in_channels, a.bias, a.learn_gamma) == (8, 32, 64, True, True) and float(a.gamma.detach()) == 0.0
    assert all(float(l.bias.detach().abs().max()) == 0 for l in (a.Wq, a.Wk, a.Wv, a.out_proj))
    b = Factorized3DConvAttn(64)                                  # the reference's default: learn_3d=True
    assert isinstance(b.temporal_conv[0], nn.Conv1d) and b.temporal_conv[0].padding == 'same' and isinstance(b.temporal_conv[1], nn.BatchNorm1d)
    assert isinstance(b.attn1d, NonLocalAttenion1D) and isinstance(b.attn1d.norm_func, nn.BatchNorm1d)


def test_learn_3d_false_is_unchanged():
    import npvp_amd
    from npvp_amd.models import Factorized3DConvAttn
    b = Factorized3DConvAttn(64, learn_3d=False)
    assert b.temporal_conv is None and b.attn1d is None
    assert not any("temporal" in k or "attn1d" in k for k in b.state_dict())
    enc, dec = npvp_amd.build_autoencoder(dict(AC.AE64_3D, learn_3d=False), 1)
    assert len(npvp_amd.AEPair(enc, dec).state_dict()) == 152          # (tests/test_ae_train_host.py's count)


def test_ae_checkpoint_round_trip(tmp_path):
    import npvp_amd
    enc, dec = _small_pair(npvp_amd)
    path = str(tmp_path / "ae3d.ckpt")
    npvp_amd.save_ae_checkpoint(path, enc, dec, epoch=1, global_step=7)
    e2, d2 = npvp_amd.build_autoencoder(AC.AE_SMALL, 1)
    assert npvp_amd.load_ae_checkpoint(path, e2, d2) == (1, 7)
    fe, fd = npvp_amd.build_frozen_autoencoder(AC.AE_SMALL, 1)
    assert npvp_amd.load_lightning_checkpoint(path, None, fe, fd) == (1, 7)
    for m in (e2, fe):
        sa, sb = m.state_dict(), enc.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert any("attn1d" in k for k in enc.state_dict()) and any("temporal_conv" in k for k in enc.state_dict())


# --------------------------------------------------------------------------------------------------------------------- goldens
def _zero_bound(cot):
    """a gradient that is exactly 0 comes out of fp32 as rounding noise: a sum over the cotangent's elements of O(1) terms that cancel,
    each rounded at 2^-24 - a random walk of sqrt(numel) such steps (the step tests' 1e-6 is this bound at their mean-loss cotangent)"""
    return 1e-6 * cot.numel() ** 0.5


def _check(name, got, want, worst):
    e = AC.rel(got, want)
    worst.append((e, name))
    assert e < TOL, (name, e)


@pytest.mark.parametrize("N,T,H,W,cf", BLOCKS)
def test_stock_block_matches_the_reference(N, T, H, W, cf):
    gold, tag = GC.load(AC.block_file(N, T, H, W)), AC.block_tag(N, T, H, W, cf)
    x, cot = AC.block_input(N, T, H, W)
    blk, worst = _block(cf), []
    blk.eval()
    with torch.no_grad():
        _check("eval", blk(x, T), gold[f"{tag}.eval"], worst)
    blk.train()
    xi = x.clone().requires_grad_()
    y = blk(xi, T)
    (y * cot).sum().backward()
    _check("y", y, gold[f"{tag}.y"], worst)
    _check("dx", xi.grad, gold[f"{tag}.dx"], worst)
    for n, p in blk.named_parameters():
        if n.endswith(AC.ZERO_GRAD):
            assert float(p.grad.abs().max()) < _zero_bound(cot) and float(abs(gold[f"{tag}.grad.{n}"]).max()) < _zero_bound(cot), n
        else:
            _check("grad." + n, p.grad, gold[f"{tag}.grad.{n}"], worst)
    for k, v in blk.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            _check("stat." + k, v, gold[f"{tag}.stat.{k}"], worst)
        elif k.endswith("num_batches_tracked"):
            assert int(v) == 1
    print("worst", max(worst))


@pytest.mark.parametrize("N,T,H,W,cf", BLOCKS)
def test_float64_restatement_matches_the_reference(N, T, H, W, cf):
    gold, tag = GC.load(AC.block_file(N, T, H, W)), AC.block_tag(N, T, H, W, cf)
    x, cot = AC.block_input(N, T, H, W)
    blk, worst = _block(cf), []
    p = AC.block_params(blk)
    with torch.no_grad():
        _check("eval", AC.block_ref(p, x.double(), T, cf, False)[0], gold[f"{tag}.eval"], worst)
    xd = x.double().requires_grad_()
    y, stats = AC.block_ref(p, xd, T, cf, True)
    names = [n for n, _ in blk.named_parameters()]
    gs = torch.autograd.grad((y * cot.double()).sum(), [xd] + [p[n] for n in names])
    _check("y", y, gold[f"{tag}.y"], worst)
    _check("dx", gs[0], gold[f"{tag}.dx"], worst)
    for n, g in zip(names, gs[1:]):
        if n.endswith(AC.ZERO_GRAD):
            assert float(g.abs().max()) < 1e-6, n
        else:
            _check("grad." + n, g, gold[f"{tag}.grad.{n}"], worst)
    assert len(stats) == 8
    for k, v in stats.items():
        _check("stat." + k, v, gold[f"{tag}.stat.{k}"], worst)
    print("worst", max(worst))


def test_stock_pair_matches_the_reference():
    import npvp_amd
    gold = GC.load("ae3d_pair")
    frames = AC.pair_frames()
    enc, dec = _small_pair(npvp_amd)
    worst = []
    enc.eval()
    with torch.no_grad():
        _check("enc_eval", enc(frames), gold["enc_eval"], worst)
    enc.train()
    feat = enc(frames)
    rec = dec(feat)
    loss = (rec - frames).abs().mean()
    loss.backward()
    _check("enc", feat, gold["enc"], worst)
    _check("rec", rec, gold["rec"], worst)
    _check("loss", loss, gold["loss"], worst)
    seen = 0
    for n, p in npvp_amd.AEPair(enc, dec).named_parameters():
        if n.endswith(AC.ZERO_GRAD):
            assert float(p.grad.abs().max()) < 1e-6, n
        else:
            _check("grad." + n, p.grad, gold["grad." + n], worst)
            seen += 1
    assert seen == sum(k.startswith("grad.") and not k.endswith(AC.ZERO_GRAD) for k in gold)
    print("worst", max(worst))


@pytest.mark.parametrize("wrong", AC.WRONG)
def test_wrong_references_are_rejected(wrong):
    """each deliberate mistake of tests/ae3d_cases.py misses a fixture by >= 10x the bar, in both orders of the block"""
    for (N, T, H, W), cf in (((2, 3, 4, 4), True), ((2, 5, 3, 5), False)):
        gold, tag = GC.load(AC.block_file(N, T, H, W)), AC.block_tag(N, T, H, W, cf)
        x, _ = AC.block_input(N, T, H, W)
        p = AC.block_params(_block(cf), grad=False)
        y, stats = AC.block_ref(p, x.double(), T, cf, True, wrong=wrong)
        errs = [AC.rel(y, gold[f"{tag}.y"])] + [AC.rel(v, gold[f"{tag}.stat.{k}"]) for k, v in stats.items()]
        assert max(errs) >= 10 * TOL, (wrong, tag, max(errs))
        good = AC.block_ref(p, x.double(), T, cf, True)
        assert AC.rel(good[0], gold[f"{tag}.y"]) < TOL


@pytest.mark.parametrize("wrong", ["scaled", "softmax_query", "across_pixels", "swap_t_hw"])
def test_wrong_attention_is_rejected_by_the_kernel_cases(wrong):
    """the kernel's float64 reference against its own mistakes, at a shape of tests/test_hip_ae3d.py"""
    N, T, HW = 2, 3, 5
    q, k, v, _ = AC.kernel_inputs(8, 32, N, T, HW)
    good = AC.temporal_attn_ref(q.double(), k.double(), v.double(), N, T, HW)
    assert AC.rel(AC.temporal_attn_ref(q.double(), k.double(), v.double(), N, T, HW, wrong), good) >= 10 * TOL
    # the reference itself: NonLocalAttenion1D's own matmuls on the (N*HW, C, T) view
    qs, ks, vs = (t.double().reshape(N, T, HW, -1).permute(0, 2, 1, 3).reshape(N * HW, T, -1) for t in (q, k, v))
    o = (torch.softmax(qs @ ks.transpose(1, 2), -1) @ vs).reshape(N, HW, T, -1).permute(0, 2, 1, 3).reshape(N * T * HW, -1)
    assert AC.rel(good, o) < 1e-12


# ------------------------------------------------------------------------------------------------------------------- conv view
def test_temporal_conv_is_a_conv2d_on_a_view():
    from npvp_amd.models.ResNetAutoEncoder import _temporal_view, _temporal_view_back
    N, T, C, H, W = 2, 5, 16, 3, 5
    x = O.seeded_randn((N * T, C, H, W), 21).contiguous(memory_format=torch.channels_last)
    view = _temporal_view(x, T)
    assert view.shape == (N, C, T, H * W) and view.untyped_storage().data_ptr() == x.untyped_storage().data_ptr()
    assert view.is_contiguous(memory_format=torch.channels_last)
    assert float(view[1, 3, 2, 7]) == float(x[1 * T + 2, 3, 7 // W, 7 % W])
    conv = nn.Conv1d(C, C, 3, padding='same')
    # the reference's route (ref/models/submodules.py:63-66): permute to (N*H*W, C, T), Conv1d, permute back
    seq = x.reshape(N, T, C, H, W).permute(0, 3, 4, 2, 1).flatten(0, 2)
    want = conv(seq).reshape(N, H, W, C, T).permute(0, 4, 3, 1, 2).flatten(0, 1)
    gw, gb = torch.autograd.grad(want.square().sum(), [conv.weight, conv.bias])
    got = _temporal_view_back(F.conv2d(view, conv.weight.unsqueeze(-1), conv.bias, 1, (1, 0)), x.shape)
    hw, hb = torch.autograd.grad(got.square().sum(), [conv.weight, conv.bias])
    assert got.shape == want.shape and (torch.equal(got, want) or AC.rel(got, want) < 1e-6)
    assert AC.rel(hw, gw) < 1e-6 and AC.rel(hb, gb) < 1e-6 and hw.shape == conv.weight.shape
    # the padding is per clip: frame 0 of clip 1 does not see frame T-1 of clip 0
    x2 = x.clone()
    x2[T - 1] += 1.0
    got2 = _temporal_view_back(F.conv2d(_temporal_view(x2, T), conv.weight.unsqueeze(-1), conv.bias, 1, (1, 0)), x.shape)
    assert torch.equal(got2[T:], got[T:]) and not torch.equal(got2[T - 2], got[T - 2])


# ------------------------------------------------------------------------------------------------------------------ C ABI
def _fwd(N=2, T=5, HW=5, A=8, V=32, ld=48, ptr=4096):
    return (ptr, ld, ptr + 4 * A, ld, ptr + 8 * A, ld, 8192, V, 8192, N, T, HW, A, V, None)


def _bwd(N=2, T=5, HW=5, A=8, V=32, ld=48, ptr=4096):
    return (ptr, ld, ptr + 4 * A, ld, ptr + 8 * A, ld, 8192, V, 8192, 1 << 20, ld, (1 << 20) + 4 * A, ld, (1 << 20) + 8 * A, ld, N, T, HW, A, V, None)


@pytest.mark.parametrize("name,args", [("npvp_temporal_attn_fwd", _fwd), ("npvp_temporal_attn_bwd", _bwd)])
def test_argument_errors_do_not_need_a_gpu(L, name, args):
    """every refusal is made on the host before anything is launched: -1 and the entry point's name in npvp_last_error"""
    from npvp_amd import _npvp_fast as Fast
    fn = getattr(L, name)
    assert hasattr(L._cdll, name) and fn is getattr(Fast, name)
    for kw, what in ((dict(T=0), b"T = 0"), (dict(T=33), b"T = 33"), (dict(A=12, V=48), b"(12, 48)"), (dict(A=8, V=64), b"(8, 64)"),
                     (dict(ld=50), b"50"), (dict(ptr=4100), b"aligned"), (dict(N=1 << 16, T=32, HW=1 << 10), b"2147483648"),
                     (dict(HW=0), b"HW = 0"), (dict(ptr=0), b"null")):
        assert fn(*args(**kw)) == -1, kw
        err = L.npvp_last_error()
        assert name.encode() in err and what in err, (kw, err)


def test_op_argument_checks():
    from npvp_amd import ops
    with pytest.raises(RuntimeError, match="T = 33"):
        ops.temporal_attn_packed(torch.zeros(33 * 4, 48), 1, 33, 4, 8, 32)
    with pytest.raises(RuntimeError, match=r"\(12, 48\)"):
        ops.temporal_attn_packed(torch.zeros(20, 72), 1, 5, 4, 12, 48)
    with pytest.raises(RuntimeError, match="qkv must be"):
        ops.temporal_attn_packed(torch.zeros(19, 48), 1, 5, 4, 8, 32)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.temporal_attn_packed(torch.zeros(20, 50), 1, 5, 4, 8, 32)
    with pytest.raises(RuntimeError, match="MI355X"):          # a CPU tensor never reaches a kernel
        ops.temporal_attn(torch.zeros(4, 5, 8), torch.zeros(4, 5, 8), torch.zeros(4, 5, 32), 5)


def test_prepare_refusals():
    import npvp_amd
    enc, dec = npvp_amd.build_autoencoder(AC.AE_SMALL, 1)
    enc.res_3dConvAttn_0.temporal_conv[1].momentum = None
    with pytest.raises(NotImplementedError, match="BatchNorm1d"):
        npvp_amd.prepare_trainable_autoencoder(enc, dec)
    from npvp_amd.models import ResnetEncoder
    odd = ResnetEncoder(1, ngf=24, n_downsampling=1, num_res_blocks=1, learn_3d=True)          # C = 48: (6, 24)
    with pytest.raises(NotImplementedError, match=r"\(6, 24\)"):
        npvp_amd.prepare_trainable_autoencoder(odd, dec)


# ------------------------------------------------------------------------------------------------------------------ frozen pair
def test_fold_of_the_temporal_half():
    import npvp_amd
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, FoldedTemporalConvAct
    enc, dec = _small_pair(npvp_amd, npvp_amd.build_frozen_autoencoder)
    ref = copy.deepcopy(enc).double().res_3dConvAttn_0
    fuse_frozen_autoencoder(enc, dec)
    blk = enc.res_3dConvAttn_0
    assert isinstance(blk.temporal_conv, FoldedTemporalConvAct) and isinstance(blk.attn1d.norm_func, nn.Identity)
    conv, bn = ref.temporal_conv[0], ref.temporal_conv[1]
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    assert blk.temporal_conv.weight.shape == (64, 64, 3, 1) and blk.temporal_conv.act == 1
    assert AC.rel(blk.temporal_conv.weight.squeeze(-1), conv.weight * s.view(-1, 1, 1)) < 1e-6
    assert AC.rel(blk.temporal_conv.bias, (conv.bias - bn.running_mean) * s + bn.bias) < 1e-6
    # as a function: folded conv + bias on the view == eval BatchNorm1d(Conv1d) of the reference's route, before the ReLU
    N, T, H, W = 2, 3, 4, 4
    x = O.seeded_randn((N * T, 64, H, W), 31).double()
    seq = x.reshape(N, T, 64, H, W).permute(0, 3, 4, 2, 1).flatten(0, 2)
    want = bn(conv(seq)).reshape(N, H, W, 64, T).permute(0, 4, 3, 1, 2).flatten(0, 1)
    got = F.conv2d(x.reshape(N, T, 64, H * W).permute(0, 2, 1, 3), blk.temporal_conv.weight.double(), blk.temporal_conv.bias.double(), 1,
                   (1, 0)).permute(0, 2, 1, 3).reshape(N * T, 64, H, W)
    assert AC.rel(got, want) < 1e-6
    a, bn = ref.attn1d, ref.attn1d.norm_func
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    assert AC.rel(blk.attn1d.out_proj.weight, a.out_proj.weight * s.view(-1, 1)) < 1e-6
    assert AC.rel(blk.attn1d.out_proj.bias, (a.out_proj.bias - bn.running_mean) * s + bn.bias) < 1e-6
    assert not any(p.requires_grad for p in enc.parameters())


# ---------------------------------------------------------------------------------------------------------- synchronised BatchNorm
def test_convert_sync_batchnorm_swaps_the_blocks_batchnorm1d_only():
    import npvp_amd
    from npvp_amd import dp

    class Holder(nn.Module):
        def __init__(self, enc):
            super().__init__()
            self.enc, self.free = enc, nn.Sequential(nn.Linear(4, 4), nn.BatchNorm1d(4))

    enc, _ = npvp_amd.build_autoencoder(AC.AE64_3D, 1)
    h = Holder(enc)
    before = {k: v.data_ptr() for k, v in h.state_dict().items()}
    n2d = sum(type(m) is nn.BatchNorm2d for m in enc.modules())
    n1d = sum(type(m) is nn.BatchNorm1d for m in enc.modules())
    blocks = [m for m in enc.modules() if type(m).__name__ == "Factorized3DConvAttn"]
    assert n1d == 2 * len(blocks) == 8
    dp.convert_sync_batchnorm(h)
    assert {k: v.data_ptr() for k, v in h.state_dict().items()} == before
    assert sum(type(m) is dp.SyncBatchNorm2d for m in enc.modules()) == n2d and not any(type(m) is nn.BatchNorm2d for m in enc.modules())
    assert all(type(b.temporal_conv[1]) is dp.SyncBatchNorm1d and type(b.attn1d.norm_func) is dp.SyncBatchNorm1d for b in blocks)
    assert type(h.free[1]) is nn.BatchNorm1d
    # outside data parallelism the twin is a BatchNorm1d
    x = O.seeded_randn((6, 64 * 2, 3), 41)
    twin, plain = blocks[0].temporal_conv[1], nn.BatchNorm1d(128)
    plain.load_state_dict(twin.state_dict())
    assert torch.equal(twin(x), plain(x))
