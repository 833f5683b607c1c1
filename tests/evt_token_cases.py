"""The learned-event-token cases of tests/golden/evt_token_encoder.npz and predictor_evt_token_{D,S}.npz (tests/golden/
make_evt_token_golden.py): shapes and seeds, the fill, an implementation run on the re-created inputs, and the CPU restatement of
what the reference computes with learn_evt_token=True (ref/models/VidHRFormer.py:22-23, 35-42; ref/models/Predictor.py:343-344),
built from unchanged oracle blocks:

    append the token to every clip as frame T+1 -> positional tables with a zero frame -> the oracle's encoder layers on T+1 frames
    (their temporal mask: no query but the last sees the last key) -> the shared norm -> the first T frames are the memory, the last
    is the event coding.
"""
import contextlib

import torch
import torch.nn as nn

from oracle import ops as O

H = W = 8
C = 512
ENC = dict(N=2, T=2, layers=2, fill=611, token=612, x=613, tables=614, cot_mem=616, cot_evt=617)
ENC_BIAS = "layers.0.temporal_MHSA.in_proj_bias"
ENC_KEYS = ("memory", "evt", "g_x", "g_EVT", "g_in_proj_bias", "g_beta", "g_gamma")
PRED = dict(N=2, To=2, Tp=2, evt_layers=2, dec_layers=2, token=622, past=623, fut=624, eps=625, cot=626)      # (the fill seed: fixture meta)
PRED_PARAMS = {"g_EVT": "EVT_Former.EVT", "g_enc_tmhsa_b": "EVT_Former.layers.0.temporal_MHSA.in_proj_bias", "g_nrmlp_B": "nrmlp.B",
               "g_dec_encdec_b": "transformer.layers.1.EncDecAttn.in_proj_bias"}
PRED_KEYS = ("y_eval", "y_train", "g_past", "g_tied_norm_w", *PRED_PARAMS)
PRED_KEYS_S = ("mu_o", "logvar_o", "mu_p", "logvar_p")
# the wrong readings of the reference's branch that the restatement must tell apart (each differs from the reference's event coding by
# 0.19 .. 0.95 rel-L2), and a mask-less encoder: the frames then see the token
WRONG_VARIANTS = ("prepend", "last_pos", "clip0", "mean_T1", "mean_T", "no_mask")


def view(t):
    """how a tensor of these cases is stored in / compared with the fixtures: whole up to 16 384 elements, else every 5th"""
    return O.golden_view(t, limit=16384)


def full_predictor(impl, learn_evt_token, **kw):
    """the predictor at the depth of the shipped configs (4 encoder + 8 decoder layers, stochastic, 'Add'): the module whose state-dict
    has 603 keys, 604 with the token"""
    return build_predictor(impl, True, learn_evt_token, 4, 8, fuse='Add', **kw)


def fill(module, seed, token_seed):
    """O.key_hashed_fill, then the token at UNIT scale: the hashed fill treats `EVT` as a weight (magnitude 0.004 - next to O(1)
    sub-layer outputs a wrong token would hardly show); the reference initialises it randn.  -> module"""
    O.key_hashed_fill(module, seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name == "EVT" or name.endswith(".EVT"):
                p.copy_(O.seeded_randn(p.shape, token_seed))
    return module


@contextlib.contextmanager
def _no_encoder_mask():
    """the oracle's encoder blocks without their temporal mask (the 'no_mask' variant only)"""
    import oracle.model as OM
    real = OM.ops.encoder_temporal_mask
    OM.ops.encoder_temporal_mask = lambda T: torch.zeros(T, T, dtype=torch.bool)
    try:
        yield
    finally:
        OM.ops.encoder_temporal_mask = real


def restated_encode(pred, feats, tables, token, variant=None):
    """pred: anything with `.EVT_Former` (an oracle encoder: layers, norm) and `.fuser`; feats (N,T,C,H,W); tables (beta, gamma or None),
    each [T*H*W, C]; token (1,H,W,C) -> memory (N,T,C,H,W), event coding (N,C,H,W).  variant: None (the reference's function) or one
    of WRONG_VARIANTS."""
    N, T, Cc, Hh, Ww = feats.shape
    P = Hh * Ww
    x = feats.permute(0, 1, 3, 4, 2)
    tok = token.unsqueeze(0).repeat(N, 1, 1, 1, 1)                                     # ref VidHRFormer.py:36
    if variant == "clip0":
        tok = torch.cat([tok[:1], torch.zeros_like(tok[1:])], dim=0)
    x = torch.cat([tok, x] if variant == "prepend" else [x, tok], dim=1).contiguous()

    def padded(t):
        if t is None:
            return None
        extra = t[(T - 1) * P:] if variant == "last_pos" else torch.zeros(P, Cc, dtype=t.dtype)
        return torch.cat([extra, t] if variant == "prepend" else [t, extra], dim=0)     # ref :40-41

    pos = (padded(tables[0]), padded(tables[1]))
    enc = pred.EVT_Former
    with (_no_encoder_mask() if variant == "no_mask" else contextlib.nullcontext()):
        for layer in enc.layers:
            x = layer(x, pos, pred.fuser)
    if enc.norm is not None:
        x = O.layernorm(x, enc.norm.weight, enc.norm.bias, enc.norm.eps)
    if variant == "prepend":
        mem, evt = x[:, 1:], x[:, 0]
    else:
        mem, evt = x[:, :T], x[:, -1]                                                   # ref Predictor.py:344
    if variant == "mean_T1":
        evt = x.mean(dim=1)
    elif variant == "mean_T":
        evt = mem.mean(dim=1)
    return mem.permute(0, 1, 4, 2, 3), evt.permute(0, 3, 1, 2)


# ------------------------------------------------------------------ the encoder alone
class _Holder(nn.Module):
    """an encoder with the fuser it is called with (what restated_encode takes)"""

    def __init__(self, enc, fuser):
        super().__init__()
        self.EVT_Former, self.fuser = enc, fuser


def encoder_inputs(dev="cpu", dtype=torch.float32):
    e = ENC
    x = O.synth_features((e["N"], e["T"], C, H, W), e["x"]).to(dev, dtype).requires_grad_()
    beta = (0.5 * O.seeded_randn((e["T"] * H * W, C), e["tables"])).to(dev, dtype).requires_grad_()
    gamma = (0.3 * O.seeded_randn((e["T"] * H * W, C), e["tables"] + 1)).to(dev, dtype).requires_grad_()
    cot_m = O.seeded_randn((e["N"], e["T"], C, H, W), e["cot_mem"]).to(dev, dtype)
    cot_e = O.seeded_randn((e["N"], C, H, W), e["cot_evt"]).to(dev, dtype)
    return x, beta, gamma, cot_m, cot_e


def encoder_results(mem, evt, x, beta, gamma, token, bias, cot_m, cot_e):
    g = torch.autograd.grad((mem * cot_m).sum() + (evt * cot_e).sum(), [x, token, bias, beta, gamma])
    return dict(zip(ENC_KEYS, (mem, evt, *g)))


def case_encoder(impl, dev, fuser=None, **kw):
    """VidHRFormerEncoder(evt_token=True) of an implementation (the reference's classes, or npvp_amd on the device), called with its
    reference signature, split as ref/models/Predictor.py:344 does -> {key: tensor}"""
    e = ENC
    m = impl.VidHRFormerEncoder(e["layers"], H, W, C, 8, 4, 0.0, 0.0, 4, 1024, nn.LayerNorm(C), True, **kw)
    fill(m, e["fill"], e["token"])
    m = m.to(dev)
    fuser = impl.PosFeatFuser(C, 'layer') if fuser is None else fuser
    x, beta, gamma, cot_m, cot_e = encoder_inputs(dev)
    y = m(x, (beta, gamma), fuser)
    mem, evt = y[:, 0:-1, ...], y[:, -1, ...]
    return encoder_results(mem, evt, x, beta, gamma, m.EVT, dict(m.named_parameters())[ENC_BIAS], cot_m, cot_e)


def case_encoder_restated(dtype=torch.float32, variant=None):
    """the CPU restatement on the encoder case, with the same fill"""
    import oracle
    e = ENC
    enc = oracle.VidHRFormerEncoder(e["layers"], H, W, C, 8, 4, 0.0, 0.0, 4, 1024, nn.LayerNorm(C), False)
    enc.register_parameter("EVT", nn.Parameter(torch.zeros(1, H, W, C)))
    fill(enc, e["fill"], e["token"])
    holder = _Holder(enc, oracle.PosFeatFuser(C, 'layer')).to(dtype)
    x, beta, gamma, cot_m, cot_e = encoder_inputs("cpu", dtype)
    mem, evt = restated_encode(holder, x, (beta, gamma), enc.EVT, variant)
    return encoder_results(mem, evt, x, beta, gamma, enc.EVT, dict(enc.named_parameters())[ENC_BIAS], cot_m, cot_e)


# ------------------------------------------------------------------ the whole predictor, 8 x 8 (the fused sub-layer path), 'SPADE'
def build_predictor(impl, stochastic, learn_evt_token=True, evt_layers=PRED["evt_layers"], dec_layers=PRED["dec_layers"], To=PRED["To"],
                    Tp=PRED["Tp"], Hh=H, Ww=W, fuse='SPADE', **kw):
    to, tp = torch.linspace(0, To - 1, To), torch.linspace(To, To + Tp - 1, Tp)
    args = dict(evt_former=True, learn_evt_token=learn_evt_token, evt_former_num_layers=evt_layers, rand_context=False, dropout=0.0,
                drop_path=0.0)
    args.update(kw)
    return impl.Predictor(Hh, Ww, To + Tp, torch.linspace(0, Hh - 1, Hh), torch.linspace(0, Ww - 1, Ww), to, tp, C, fuse, 'layer', 256, 1,
                          stochastic, dec_layers, **args)


def small_predictor(impl, stochastic, seed, dev, learn_evt_token=True, **kw):
    """2 + 2 layers, 'SPADE', filled -> module on dev"""
    return fill(build_predictor(impl, stochastic, learn_evt_token, **kw), seed, PRED["token"]).to(dev)


def restated_predictor(stochastic, seed, dtype=torch.float32, variant=None, **kw):
    """the oracle's Predictor with the token: its encoder pass is restated_encode on its own (unchanged) blocks, `EVT_Former.EVT` is
    registered where the reference has it (state-dict and parameter order included)"""
    import oracle

    class EvtTokenPredictor(oracle.Predictor):
        def evt_coding_forward(self, x, pos_beta, pos_gamma):
            return restated_encode(self, x, (pos_beta, pos_gamma), self.EVT_Former.EVT, variant)

    ns = type("impl", (), {"Predictor": EvtTokenPredictor})
    m = small_predictor(ns, stochastic, seed, "cpu", learn_evt_token=False, **kw)
    m.EVT_Former.register_parameter("EVT", nn.Parameter(torch.zeros(1, H, W, C)))
    return fill(m, seed, PRED["token"]).to(dtype)


def predictor_inputs(dev="cpu", dtype=torch.float32):
    p = PRED
    past = O.synth_features((p["N"], p["To"], C, H, W), p["past"]).to(dev, dtype)
    fut = O.synth_features((p["N"], p["Tp"], C, H, W), p["fut"]).to(dev, dtype)
    eps = O.seeded_randn((p["N"], C, H, W), p["eps"]).to(dev, dtype)
    cot = O.seeded_randn((p["N"], p["Tp"], C, H, W), p["cot"]).to(dev, dtype)
    return past, fut, eps, cot


@contextlib.contextmanager
def _randn_returns(eps):
    """the reference draws eps with torch.randn (the golden maker's injection, as make_golden.py's predictor_S)"""
    real = torch.randn
    torch.randn = lambda *a, **k: eps
    try:
        yield
    finally:
        torch.randn = real


def run_predictor(m, stochastic, past, fut, eps, cot, div_kl, patch_randn=False):
    """-> the arrays of predictor_evt_token_{D,S}.npz from a filled module (the reference's, the restatement's or the implementation's).
    eps is injected through `eps_fn` of the event encoders (oracle, implementation) or, patch_randn, through torch.randn (reference)."""
    res = {}
    if stochastic and not patch_randn:
        m.evt_prior.eps_fn = m.evt_posterior.eps_fn = lambda shape: eps
    inject = (lambda: _randn_returns(eps)) if (stochastic and patch_randn) else contextlib.nullcontext
    m.eval()
    with torch.no_grad(), inject():
        res["y_eval"] = m(past)
    m.train()
    p = past.clone().requires_grad_()
    with inject():
        o = m(p, fut) if stochastic else m(p)
    yt = o[0] if stochastic else o
    loss = (yt * yt * cot).sum()          # smooth at the final ReLU's kink (see make_golden.py)
    if stochastic:
        loss = loss + div_kl(*o[1:])
        res.update(zip(PRED_KEYS_S, o[1:]))
    m.zero_grad()
    loss.backward()
    sd = dict(m.named_parameters())
    res.update(y_train=yt, g_past=p.grad, g_tied_norm_w=m.transformer.norm.weight.grad)
    for key, name in PRED_PARAMS.items():
        res[key] = sd[name].grad
    return res
