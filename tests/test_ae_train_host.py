"""CPU: the Stage-1 training path's C ABI (exported, fast-wrapped, host-side argument checks), its op-level argument checks, the
trainable pair's state-dict keys and the LitAE checkpoint layout - no GPU needed."""
import pytest
import torch

NEW = ["npvp_bn_workspace_bytes", "npvp_bn_stats", "npvp_bn_act_apply", "npvp_bn_act_bwd", "npvp_reflect_pad", "npvp_nonlocal_attn_fwd",
       "npvp_nonlocal_attn_bwd"]
AE64 = dict(ngf=64, n_downsampling=3, num_res_blocks=2, out_layer='Tanh', learn_3d=False)
AE128 = dict(ngf=32, n_downsampling=4, num_res_blocks=3, out_layer='Tanh', learn_3d=False)


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    build.build(verbose=False)
    from npvp_amd._lib import lib
    return lib()


def test_new_symbols_exported_and_fast_wrapped(L):
    from npvp_amd import _npvp_fast as F
    for n in NEW:
        assert hasattr(L._cdll, n), n
        assert getattr(L, n) is getattr(F, n), n


def test_c_argument_checks(L):
    assert L.npvp_bn_workspace_bytes(64) == 1025 * 2 * 64 * 8 and L.npvp_bn_workspace_bytes(0) == -1
    assert L.npvp_bn_stats(None, 16, 64, 64, 0, None, None, 0, None) == -1
    assert L.npvp_bn_stats(16, 16, 48, 48, 0, 16, 16, 1 << 20, None) == -1 and b"power of two" in L.npvp_last_error()
    assert L.npvp_bn_stats(16, 8, 18, 4, 1, 16, 16, 1 << 20, None) == -1 and b"% 4" in L.npvp_last_error()
    assert L.npvp_bn_act_apply(16, 16, 16, None, 16, 10, 1e-5, 0.1, None, None, 16, 64, 64, 0, 2, 16, 16, 16, None) == -1
    assert b"act" in L.npvp_last_error()
    assert L.npvp_bn_act_apply(16, 16, 16, None, None, 0, 1e-5, 0.1, None, None, 16, 64, 64, 0, 1, 16, 16, 16, None) == -1
    assert L.npvp_bn_act_bwd(16, 16, 16, 16, 16, 16, 16, 64, 64, 0, 1, 1, 16, 16, 16, 16, 8, None) == -1
    assert b"workspace" in L.npvp_last_error()
    assert L.npvp_reflect_pad(16, 16, 1, 4, 4, 3, 4, 1, 0, None) == -1 and b"pad" in L.npvp_last_error()
    assert L.npvp_reflect_pad(16, 16, 1, 4, 4, 3, 1, 2, 0, None) == -1
    args = lambda A, V, H, W: (16, 64, 16, 64, 16, 64, 16, 64, 16, 2, H, W, A, V, None)
    # (every call here fails its host-side check: nothing is launched)
    assert L.npvp_nonlocal_attn_fwd(*args(12, 48, 8, 8)) == -1 and b"attn dim" in L.npvp_last_error()
    assert L.npvp_nonlocal_attn_fwd(*args(8, 32, 32, 32)) == -1 and b"grid" in L.npvp_last_error()
    assert L.npvp_nonlocal_attn_fwd(*args(64, 256, 8, 6)) == -1
    assert L.npvp_nonlocal_attn_bwd(*([None, 64] * 4 + [None, None] + [None, 64] * 3 + [2, 8, 8, 64, 256, None])) == -1


def test_op_argument_checks():
    from npvp_amd import ops
    x = torch.zeros(2, 8, 4, 4)
    with pytest.raises(RuntimeError, match="act"):
        ops.bn_act_train(x, torch.ones(8), torch.zeros(8), act=2)
    with pytest.raises(RuntimeError, match="momentum"):
        ops.bn_act_train(x, torch.ones(8), torch.zeros(8), torch.zeros(8), torch.ones(8), momentum=None)
    with pytest.raises(RuntimeError, match="go together"):
        ops.bn_act_train(x, torch.ones(8), torch.zeros(8), torch.zeros(8), None)
    with pytest.raises(RuntimeError, match="AE configs"):
        ops.nonlocal_attn_packed(torch.zeros(64, 72), 1, 8, 8, 12, 48)
    with pytest.raises(RuntimeError, match="grid"):
        ops.nonlocal_attn_packed(torch.zeros(2048, 48), 2, 32, 32, 8, 32)
    with pytest.raises(RuntimeError, match="MI355X"):          # a CPU tensor never reaches a kernel
        ops.reflect_pad(x, 1)


@pytest.mark.parametrize("AE,ch,nkeys", [(AE64, 1, 152), (AE128, 3, 218)])
def test_trainable_pair_keeps_reference_keys(AE, ch, nkeys):
    import npvp_amd
    enc, dec = npvp_amd.build_autoencoder(AE, ch)
    assert enc.training and dec.training and all(p.requires_grad for p in list(enc.parameters()) + list(dec.parameters()))
    fe, fd = npvp_amd.build_frozen_autoencoder(AE, ch)
    before = list(npvp_amd.AEPair(enc, dec).state_dict())
    npvp_amd.prepare_trainable_autoencoder(enc, dec)
    after = list(npvp_amd.AEPair(enc, dec).state_dict())
    assert before == after == list(npvp_amd.AEPair(fe, fd).state_dict()) and len(after) == nkeys
    assert after[0].startswith("VPTR_Enc.") and after[-1].startswith("VPTR_Dec.")
    with pytest.raises(RuntimeError):
        npvp_amd.ae_train_step(*npvp_amd.build_autoencoder(AE, ch), None, None, None)


def test_ae_checkpoint_layout_loads_on_the_stage2_side(tmp_path):
    """save_ae_checkpoint writes LitAE's layout; Stage 2's load_lightning_checkpoint(path, None, enc, dec) and
    build_frozen_autoencoder read it with equal key lists"""
    import npvp_amd
    from oracle import ops as O
    enc, dec = npvp_amd.build_autoencoder(AE64, 1)
    O.key_hashed_fill(npvp_amd.AEPair(enc, dec), 5)
    path = str(tmp_path / "ae.ckpt")
    npvp_amd.save_ae_checkpoint(path, enc, dec, epoch=3, global_step=42)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert set(ck) >= {"state_dict", "epoch", "global_step"} and (ck["epoch"], ck["global_step"]) == (3, 42)
    assert list(ck["state_dict"]) == list(npvp_amd.AEPair(enc, dec).state_dict())
    fe, fd = npvp_amd.build_frozen_autoencoder(AE64, 1)
    assert npvp_amd.load_lightning_checkpoint(path, None, fe, fd) == (3, 42)
    for a, b in ((fe, enc), (fd, dec)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    e2, d2 = npvp_amd.build_autoencoder(AE64, 1)
    assert npvp_amd.load_ae_checkpoint(path, e2, d2) == (3, 42)
    assert torch.equal(e2.res_3dConvAttn_1.attn2d.gamma, enc.res_3dConvAttn_1.attn2d.gamma)
