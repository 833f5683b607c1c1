"""CPU: the Stage-1 fixtures (tests/golden/ae_train_{64,128}.npz, written from the reference's LitAE by
tests/golden/make_ae_train_golden.py) are reproduced in-process by this package's ResnetEncoder / ResnetDecoder on stock torch with
LitAE's step (x = cat(past, future), L1, Adam betas=(0.5, 0.999)), and LitAE's state-dict keys are the AEPair's."""
import numpy as np
import pytest
import torch

import ae_train_cases as AC
import golden_cases as GC

TOL = 1e-5        # the same CPU arithmetic as the reference's modules


@pytest.mark.parametrize("tag", ["64", "128"])
def test_regenerate_ae_train_fixture(tag):
    import npvp_amd
    gold = GC.load(f"ae_train_{tag}")
    ci, AE, B, T, S = AC.CASES[tag]
    torch.manual_seed(0)
    enc, dec = npvp_amd.build_autoencoder(AE, ci)
    pair = npvp_amd.AEPair(enc, dec)
    AC.fill(pair)
    assert list(AC.state_keys(pair)) == list(gold["state_keys"])          # LitAE's keys (152 / 218)
    assert list(AC.param_names(pair)) == list(gold["param_names"])       # LitAE.configure_optimizers' order
    opt = torch.optim.Adam(list(enc.parameters()) + list(dec.parameters()), lr=AC.LR, betas=(0.5, 0.999))

    def step(past, fut):
        opt.zero_grad()
        x = torch.cat([past, fut], 1)
        loss = (dec(enc(x)) - x).abs().mean()
        loss.backward()
        opt.step()
        return loss.detach()
    res = AC.record(pair, step, tag)
    for k in ("loss_0", "loss_1", "grad_norm", "grad_head", "running", "param_head_0", "param_head_1"):
        assert GC.rel_err(res[k], gold[k]) < TOL, (k, GC.rel_err(res[k], gold[k]))


def test_checkpoint_keys_are_litae_keys(tmp_path):
    """save_ae_checkpoint's state_dict keys are exactly the reference LitAE's (from the fixture), in LitAE's order"""
    import npvp_amd
    for tag in ("64", "128"):
        ci, AE = AC.CASES[tag][:2]
        enc, dec = npvp_amd.build_autoencoder(AE, ci)
        path = str(tmp_path / f"ae{tag}.ckpt")
        npvp_amd.save_ae_checkpoint(path, enc, dec)
        ck = torch.load(path, map_location="cpu", weights_only=True)
        assert list(ck["state_dict"]) == list(GC.load(f"ae_train_{tag}")["state_keys"])
