"""The centre-pad cases of tests/golden/window_pad.npz and predictor_window_pad.npz (tests/golden/make_window_pad_golden.py):
inputs re-created from their seeds, an implementation run on them, and the CPU restatement of what the reference computes when the
window does not tile the grid (ref/models/VidHRFormer.py:287-305, 488-511) built from unchanged oracle.ops functions:

    pad the q|k source and the value source with zero rows -> in-projection of ALL padded rows (a pad token's q, k, v are the
    biases) -> attention over the windows of the padded grid, pad tokens being ordinary keys (NO key mask) -> cut the centre ->
    out-projection.
"""
import math

import torch
import torch.nn.functional as F

from oracle import ops as O

# (frames, H, W, window): pads of 3 / 2 (odd: top 1, bottom 2), of 2 / 6 with the 64-row window, and on one axis only with ws > H
SLMHSA_CASES = ((2, 5, 6, 4), (2, 6, 10, 8), (1, 3, 8, 4))
SLMHSA_KEYS = ("y", "gx", "gv", "gb", "gW_rows")
SEED0 = 210                      # case i: seed = SEED0 + 10 i (weights), seed + 1 / 2 / 3: x, value, cotangent
PRED = dict(N=2, To=4, Tp=4, H=6, W=10, past=252, fut=253, cot=255)       # (the fill seed is in the fixture's meta)
PRED_PARAMS = {"g_enc_slmhsa_b": "EVT_Former.layers.0.SLMHSA.attn.in_proj_bias",
               "g_dec_slmhsa_b": "transformer.layers.1.SLMHSA.attn.in_proj_bias"}


def view(t):
    """how a tensor of these cases is stored in / compared with the fixtures: whole up to 16 384 elements, else every 5th"""
    return O.golden_view(t, limit=16384)


def padblock_geometry(H, W, ws):
    """ref PadBlock's own formulas (:493-498, :510), restated: -> (Hp, Wp, top, left)"""
    pad_h = math.ceil(H / ws) * ws - H
    pad_w = math.ceil(W / ws) * ws - W
    return H + pad_h, W + pad_w, pad_h // 2, pad_w // 2


def restated_slmhsa(w_in, b_in, w_out, b_out, x, v, ws, heads=8):
    """x, v: (Fr, H, W, C) -> (Fr, H, W, C); differentiable in every argument"""
    Fr, H, W, C = x.shape
    Hp, Wp, top, left = padblock_geometry(H, W, ws)
    pad = (0, 0, left, Wp - W - left, top, Hp - H - top)
    xp, vp = F.pad(x, pad).reshape(-1, C), F.pad(v, pad).reshape(-1, C)
    q = xp @ w_in[:C].t() + b_in[:C]
    k = xp @ w_in[C:2 * C].t() + b_in[C:2 * C]
    vv = vp @ w_in[2 * C:].t() + b_in[2 * C:]
    rows = O.spatial_groups(Fr, Hp, Wp, ws)
    o = O.attn_core(q, k, vv, rows, rows, heads)
    o = o.view(Fr, Hp, Wp, C)[:, top:top + H, left:left + W].reshape(-1, C)
    return (o @ w_out.t() + b_out).view(Fr, H, W, C)


def fixture_case(i):
    """-> ((frames, H, W, window), seed) of case i of window_pad.npz"""
    return SLMHSA_CASES[i], SEED0 + 10 * i


def slmhsa_inputs(case, seed, dev="cpu", dtype=torch.float32):
    Fr, H, W, ws = case
    x = O.seeded_randn((1, Fr, H, W, 512), seed + 1).to(dev, dtype).requires_grad_()
    v = O.seeded_randn((1, Fr, H, W, 512), seed + 2).to(dev, dtype).requires_grad_()
    cot = O.seeded_randn((1, Fr, H, W, 512), seed + 3).to(dev, dtype)
    return x, v, cot


def slmhsa_results(y, x, v, cot, w_in, b_in):
    gx, gv, gw, gb = torch.autograd.grad((y * cot).sum(), [x, v, w_in, b_in])
    return dict(y=y, gx=gx, gv=gv, gb=gb, gW_rows=gw[::64])


def case_slmhsa(impl, dev, case, seed):
    """the implementation's SpatialLocalMultiheadAttention (with value= given) on a case -> {key: tensor}"""
    m = impl.SpatialLocalMultiheadAttention(512, 8, case[3], 0.0)
    O.key_hashed_fill(m, seed)
    m = m.to(dev)
    x, v, cot = slmhsa_inputs(case, seed, dev)
    return slmhsa_results(m(x, value=v), x, v, cot, m.attn.in_proj_weight, m.attn.in_proj_bias)


def case_slmhsa_restated(case, seed, dtype=torch.float32):
    """the CPU restatement on a case, with the same key-hashed weights"""
    import oracle
    m = oracle.SpatialLocalMultiheadAttention(512, 8, case[3], 0.0)
    O.key_hashed_fill(m, seed)
    m = m.to(dtype)
    x, v, cot = slmhsa_inputs(case, seed, "cpu", dtype)
    a = m.attn
    y = restated_slmhsa(a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, x[0], v[0], case[3])[None]
    return slmhsa_results(y, x, v, cot, a.in_proj_weight, a.in_proj_bias)


def restated_oracle(module):
    """an oracle module (a block, a predictor) whose spatial window attentions centre-pad: every oracle SLMHSA in it computes
    restated_slmhsa on its own parameters (the oracle's class asserts that the window tiles the grid).  -> module"""
    import oracle

    class PaddedSLMHSA(oracle.SpatialLocalMultiheadAttention):
        def forward(self, x, value=None):
            N, T, H, W, C = x.shape
            a = self.attn
            xv = x if value is None else value
            return restated_slmhsa(a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias, x.reshape(N * T, H, W, C),
                                   xv.reshape(N * T, H, W, C), self.window_size, self.num_heads).view(N, T, H, W, C)

    for m in module.modules():
        if type(m) is oracle.SpatialLocalMultiheadAttention:
            m.__class__ = PaddedSLMHSA
    return module


def small_predictor(impl, seed, dev, evt_layers=2, dec_layers=2, H=PRED["H"], W=PRED["W"], To=PRED["To"], Tp=PRED["Tp"], **kw):
    """Predictor(H, W, ...), window 4, 'Add', 'layer', deterministic"""
    to, tp = torch.linspace(0, To - 1, To), torch.linspace(To, To + Tp - 1, Tp)
    args = dict(evt_former=True, learn_evt_token=False, evt_former_num_layers=evt_layers, rand_context=False, dropout=0.0, drop_path=0.0)
    args.update(kw)
    m = impl.Predictor(H, W, To + Tp, torch.linspace(0, H - 1, H), torch.linspace(0, W - 1, W), to, tp, 512, 'Add', 'layer', 256, 1,
                       False, dec_layers, **args)
    O.key_hashed_fill(m, seed)
    return m.to(dev)


def predictor_inputs(dev):
    p = PRED
    past = O.synth_features((p["N"], p["To"], 512, p["H"], p["W"]), p["past"]).to(dev)
    cot = O.seeded_randn((p["N"], p["Tp"], 512, p["H"], p["W"]), p["cot"]).to(dev)
    return past, cot


def run_predictor(m, past, cot):
    """-> the arrays of predictor_window_pad.npz from a filled module (the reference's or the implementation's)"""
    res = {}
    m.eval()
    with torch.no_grad():
        res["y_eval"] = m(past)
    m.train()
    p = past.clone().requires_grad_()
    yt = m(p)
    m.zero_grad()
    (yt * yt * cot).sum().backward()          # smooth at the final ReLU's kink (see make_golden.py)
    sd = dict(m.named_parameters())
    res.update(y_train=yt, g_past=p.grad, g_tied_norm_w=m.transformer.norm.weight.grad)
    for key, name in PRED_PARAMS.items():
        res[key] = sd[name].grad
    return res
