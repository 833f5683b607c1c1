"""CPU: the rectangular Stage-1 fixture (tests/golden/ae_train_rect.npz, written from the reference's LitAE at 48x80 frames by
tests/golden/make_ae_rect_golden.py) is reproduced in-process by this package's ResnetEncoder / ResnetDecoder on stock torch with
LitAE's step, as tests/test_ae_train_golden.py does for the config sizes; LitAE's state-dict keys are the AEPair's."""
import torch

import ae_rect_cases as RC
import golden_cases as GC

TOL = 1e-5        # the same CPU arithmetic as the reference's modules (tests/test_ae_train_golden.py)


def test_regenerate_ae_rect_fixture():
    import npvp_amd
    gold = GC.load(RC.NAME)
    torch.manual_seed(0)
    enc, dec = npvp_amd.build_autoencoder(RC.AE, RC.CI)
    pair = npvp_amd.AEPair(enc, dec)
    RC.fill(pair)
    assert list(RC.state_keys(pair)) == list(gold["state_keys"])
    assert list(RC.param_names(pair)) == list(gold["param_names"])
    opt = torch.optim.Adam(list(enc.parameters()) + list(dec.parameters()), lr=RC.LR, betas=(0.5, 0.999))

    def step(past, fut):
        opt.zero_grad()
        x = torch.cat([past, fut], 1)
        loss = (dec(enc(x)) - x).abs().mean()
        loss.backward()
        opt.step()
        return loss.detach()
    res = RC.record(pair, step)
    for k in ("loss_0", "loss_1", "grad_norm", "grad_head", "running", "param_head_0", "param_head_1"):
        assert GC.rel_err(res[k], gold[k]) < TOL, (k, GC.rel_err(res[k], gold[k]))
