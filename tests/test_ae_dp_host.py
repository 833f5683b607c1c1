"""CPU: data-parallel Stage-1 training - the C ABI of synchronised BatchNorm (exported, fast-wrapped, host-side argument checks),
which BatchNorm layers of a prepared pair are handed a process group, ae_data_parallel without a process group, ae_train_step's
refusal of a foreign GradSync and the checkpoint of a converted pair - no GPU needed."""
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

NEW = ["npvp_bn_act_apply_sync", "npvp_bn_bwd_sums", "npvp_bn_act_bwd_apply"]
AE64 = dict(ngf=64, n_downsampling=3, num_res_blocks=2, out_layer='Tanh', learn_3d=False)
SMALL = dict(ngf=8, n_downsampling=2, num_res_blocks=1, out_layer='Tanh', learn_3d=False)


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    build.build(verbose=False)
    from npvp_amd._lib import lib
    return lib()


def test_new_symbols_exported_and_fast_wrapped(L):
    from npvp_amd import _npvp_fast as Fast
    for n in NEW:
        assert hasattr(L._cdll, n), n
        assert getattr(L, n) is getattr(Fast, n), n


def test_c_argument_checks(L):
    """every call fails its host-side check: nothing is launched (16 stands for an aligned, non-null address)"""
    ws = L.npvp_bn_workspace_bytes(64)
    # apply_sync(x, w, b, residual, stat, eps, momentum, running_mean, running_var, outer, inner, C, layout, act, y, mean, rstd, stream)
    assert L.npvp_bn_act_apply_sync(16, 16, 16, None, None, 1e-5, 0.1, None, None, 16, 64, 64, 0, 1, 16, 16, 16, None) == -1
    assert b"null stat" in L.npvp_last_error()
    assert L.npvp_bn_act_apply_sync(16, 16, 16, None, 16, 1e-5, 0.1, None, None, 16, 64, 64, 0, 2, 16, 16, 16, None) == -1
    assert b"act" in L.npvp_last_error()
    assert L.npvp_bn_act_apply_sync(16, 16, 16, None, 16, 1e-5, 0.1, None, None, 16, 48, 48, 0, 1, 16, 16, 16, None) == -1
    assert b"power of two" in L.npvp_last_error()
    # bwd_sums(g, x, mean, rstd, w, b, outer, inner, C, layout, act, sums, dw, db, workspace, ws_bytes, stream)
    assert L.npvp_bn_bwd_sums(16, 16, 16, 16, 16, 16, 16, 64, 64, 0, 1, None, 16, 16, 16, ws, None) == -1
    assert b"null sums" in L.npvp_last_error()
    assert L.npvp_bn_bwd_sums(16, 16, 16, 16, 16, 16, 16, 64, 64, 0, 1, 16, 16, 16, 16, ws - 8, None) == -1
    assert b"workspace" in L.npvp_last_error()
    assert L.npvp_bn_bwd_sums(16, 16, 16, 16, 16, 16, 16, 64, 64, 0, 2, 16, 16, 16, 16, ws, None) == -1
    assert b"act" in L.npvp_last_error()
    # bwd_apply(g, x, mean, rstd, w, b, sums, count, outer, inner, C, layout, act, dx, stream)
    assert L.npvp_bn_act_bwd_apply(16, 16, 16, 16, 16, 16, None, 16, 16, 64, 64, 0, 1, 16, None) == -1
    assert b"null sums" in L.npvp_last_error()
    assert L.npvp_bn_act_bwd_apply(16, 16, 16, 16, 16, 16, 16, None, 16, 64, 64, 0, 1, 16, None) == -1
    assert b"null count" in L.npvp_last_error()
    assert L.npvp_bn_act_bwd_apply(16, 16, 16, 16, 16, 16, 16, 16, 16, 64, 64, 0, 2, 16, None) == -1
    assert b"act" in L.npvp_last_error()
    assert L.npvp_bn_act_bwd_apply(16, 16, 16, 16, 16, 16, 16, 16, 8, 18, 4, 1, 1, 16, None) == -1
    assert b"% 4" in L.npvp_last_error()


GROUP = object()        # stands for the SyncBatchNorm process group


def _stub_ops(monkeypatch, calls):
    """the HIP ops of the prepared forward replaced by shape-preserving CPU stand-ins; bn_act_train records what it is handed"""
    from npvp_amd import ops

    def bn_act_train(x, w, b, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, act=0, train=True, residual=None, group=None):
        calls.append((train, group))
        return x if residual is None else x + residual
    monkeypatch.setattr(ops, "bn_act_train", bn_act_train)
    monkeypatch.setattr(ops, "reflect_pad", lambda x, p: F.pad(x, (p, p, p, p), mode="reflect"))
    monkeypatch.setattr(ops, "linear", lambda x, w, b=None: F.linear(x, w, b))
    monkeypatch.setattr(ops, "nonlocal_attn_packed", lambda qkv, N, H, W, A, V: qkv[:, 2 * A:2 * A + V])


def _forward(enc, dec):
    with torch.no_grad():
        return dec(enc(torch.zeros(1, 2, 1, 16, 16)))


def test_only_training_sync_layers_under_data_parallelism_get_a_group(monkeypatch):
    import npvp_amd
    from npvp_amd import dp
    calls = []
    _stub_ops(monkeypatch, calls)
    monkeypatch.setattr(dp, "syncbn_group", lambda: GROUP)
    enc, dec = npvp_amd.build_autoencoder(SMALL, 1)
    npvp_amd.prepare_trainable_autoencoder(enc, dec, channels_last=False)
    layers = [m for m in list(enc.modules()) + list(dec.modules()) if isinstance(m, nn.BatchNorm2d)]
    in_attn = [m.norm_func for m in enc.modules() if isinstance(m, npvp_amd.models.ResNetAutoEncoder.NonLocalAttenion2D)]
    assert in_attn and all(isinstance(m, nn.BatchNorm2d) for m in in_attn)
    n = len(layers)

    def groups(active):
        monkeypatch.setattr(dp, "active", lambda group=None: active)
        del calls[:]
        _forward(enc, dec)
        assert len(calls) == n                                        # every BatchNorm layer once, the attention's norm_func included
        return [g for _, g in calls]

    # a plain BatchNorm2d never gets one, data parallel or not
    assert groups(True) == [None] * n and groups(False) == [None] * n
    before = list(npvp_amd.AEPair(enc, dec).state_dict())
    dp.convert_sync_batchnorm(enc); dp.convert_sync_batchnorm(dec)
    assert list(npvp_amd.AEPair(enc, dec).state_dict()) == before
    assert all(isinstance(m.norm_func, dp.SyncBatchNorm2d) for m in enc.modules()
               if isinstance(m, npvp_amd.models.ResNetAutoEncoder.NonLocalAttenion2D))
    assert groups(True) == [GROUP] * n                                # converted, training, data parallel: all of them
    assert groups(False) == [None] * n                                # no process group: this rank's own statistics
    enc.eval(); dec.eval()
    assert groups(True) == [None] * n and all(not t for t, _ in calls)        # eval mode is untouched
    enc.train(); dec.eval()
    got = groups(True)
    n_enc = sum(isinstance(m, nn.BatchNorm2d) for m in enc.modules())
    assert got == [GROUP] * n_enc + [None] * (n - n_enc)


def test_ae_data_parallel_without_a_process_group():
    import npvp_amd
    from npvp_amd import dp
    assert not dp.active()
    enc, dec = npvp_amd.build_autoencoder(SMALL, 1)
    npvp_amd.prepare_trainable_autoencoder(enc, dec)
    opt = types.SimpleNamespace(ae_pair=npvp_amd.AEPair(enc, dec), ctx=object())
    assert npvp_amd.ae_data_parallel(enc, dec, opt) is None
    assert not any(isinstance(m, dp.SyncBatchNorm2d) for m in list(enc.modules()) + list(dec.modules()))


def test_ae_train_step_refuses_a_grad_sync_on_another_context():
    import npvp_amd
    mod = types.SimpleNamespace(_npvp_trainable=True)
    opt = types.SimpleNamespace(ctx=object())
    gs = types.SimpleNamespace(on=True, ctx=object(), finish=lambda: None)
    with pytest.raises(RuntimeError, match="another scheduling context"):
        npvp_amd.ae_train_step(mod, mod, opt, None, None, grad_sync=gs)


def test_converted_pair_checkpoint_loads_into_plain_and_frozen_pairs(tmp_path, monkeypatch):
    import npvp_amd
    from npvp_amd import dp
    from oracle import ops as O
    monkeypatch.setattr(dp, "syncbn_group", lambda: GROUP)
    enc, dec = npvp_amd.build_autoencoder(AE64, 1)
    O.key_hashed_fill(npvp_amd.AEPair(enc, dec), 5)
    keys = list(npvp_amd.AEPair(enc, dec).state_dict())
    dp.convert_sync_batchnorm(enc); dp.convert_sync_batchnorm(dec)
    assert any(isinstance(m, dp.SyncBatchNorm2d) for m in enc.modules()) and any(isinstance(m, dp.SyncBatchNorm2d) for m in dec.modules())
    assert list(npvp_amd.AEPair(enc, dec).state_dict()) == keys
    path = str(tmp_path / "ae_dp.ckpt")
    npvp_amd.save_ae_checkpoint(path, enc, dec, epoch=1, global_step=7)
    e2, d2 = npvp_amd.build_autoencoder(AE64, 1)
    assert npvp_amd.load_ae_checkpoint(path, e2, d2) == (1, 7)
    fe, fd = npvp_amd.build_frozen_autoencoder(AE64, 1)
    assert npvp_amd.load_lightning_checkpoint(path, None, fe, fd) == (1, 7)
    for a, b in ((e2, enc), (d2, dec), (fe, enc), (fd, dec)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
