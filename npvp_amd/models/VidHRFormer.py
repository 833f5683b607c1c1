"""HIP-backed VidHRFormer blocks: drop-in for ref/models/VidHRFormer.py (same class names,
constructor signatures, forward signatures, attribute names and state-dict keys).

Everything runs on ONE canonical activation layout, x[N*T, H*W, C] (a contiguous (N,T,H,W,C)
tensor); the reference's permute/reshape/rearrange round trips (ref :34,50,94,114,217,240,
283-307,379,392) become index math inside the kernels.  Residual adds, dropout and drop-path
are epilogues of the GEMM / frame-LN kernels, never separate passes.
"""
import copy

import torch
import torch.nn as nn

from .. import ops
from ..ops import Drop, AttnCfg


class _OutProj(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(C, C))
        self.bias = nn.Parameter(torch.zeros(C))
        nn.init.xavier_uniform_(self.weight)


class MultiheadAttention(nn.Module):
    """Parameter container with torch.nn.MultiheadAttention's layout (in_proj_weight [3C,C], in_proj_bias
    [3C], out_proj.{weight,bias}) - the reference instantiates nn.MultiheadAttention at
    ref/models/VidHRFormer.py:70,180,192,270.  The arithmetic (its key-is-not-value slow path) is:
    q|k projection as ONE [R,2C] GEMM when q and k share their input, v projection, attention core
    kernel, out-projection GEMM with the residual/dropout epilogue."""

    def __init__(self, embed_dim, num_heads, dropout=0.0):
        super().__init__()
        assert embed_dim // num_heads == 64, "the gfx950 attention core is built for head_dim 64 (embed_dim 512, 8 heads)"
        self.embed_dim, self.num_heads, self.dropout = embed_dim, num_heads, dropout
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = _OutProj(embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)

    def self_attention(self, x_qk, x_v, cfg, residual=None, drop=ops.NO_DROP):
        """q = k source x_qk [R,C], value source x_v [R,C] -> residual + drop(out_proj(core))."""
        C = self.embed_dim
        w, b = self.in_proj_weight, self.in_proj_bias
        if not cfg.tiles:
            # the window does not tile the grid: centre-pad both sources BEFORE the in-projection (ref :287,295 - a pad token is a
            # zero row, so its q, k, v are the biases and it is an ordinary key of its window), cut the centre back out (ref :305)
            x_qk, x_v = ops.grid_pad(x_qk, cfg), ops.grid_pad(x_v, cfg)
        qk = ops.linear(x_qk, w[:2 * C], b[:2 * C])
        v = ops.linear(x_v, w[2 * C:], b[2 * C:])
        o = ops.attn_packed(qk, v, cfg)
        if not cfg.tiles:
            o = ops.grid_cut(o, cfg)
            if residual is None and not drop.on:
                # the module called on its own: the real rows of a few frames of such a grid are seldom a multiple of the 32 the
                # out-projection's weight gradient sums in (inside a block the residual stream has the whole batch's rows)
                return ops.linear_any_rows(o, self.out_proj.weight, self.out_proj.bias)
        return ops.linear(o, self.out_proj.weight, self.out_proj.bias, residual=residual, drop=drop)

    def cross_attention(self, x_q, x_k, x_v, cfg, residual=None, drop=ops.NO_DROP):
        C = self.embed_dim
        w, b = self.in_proj_weight, self.in_proj_bias
        q = ops.linear(x_q, w[:C], b[:C])
        k = ops.linear(x_k, w[C:2 * C], b[C:2 * C])
        v = ops.linear(x_v, w[2 * C:], b[2 * C:])
        o = ops.attn(q, k, v, cfg)
        return ops.linear(o, self.out_proj.weight, self.out_proj.bias, residual=residual, drop=drop)


class SpatialLocalMultiheadAttention(nn.Module):
    """ref/models/VidHRFormer.py:247-307."""

    def __init__(self, embed_dim, num_heads, window_size=7, dropout=0.):
        super().__init__()
        self.dim, self.num_heads, self.window_size, self.dropout = embed_dim, num_heads, window_size, dropout
        self.attn = MultiheadAttention(embed_dim, num_heads, dropout=dropout)

    def _cfg(self, N, T, H, W):
        if H % self.window_size or W % self.window_size:
            # ref PadBlock (:488-511): the grid is centre-padded to the next multiple of the window and the centre cut back out
            return AttnCfg.spatial(N * T, H, W, self.window_size, self.num_heads, self.dropout if self.training else 0.0)
        return AttnCfg(0, N * T, H * W, W, self.window_size, 0, 0, self.num_heads, 0,
                       self.dropout if self.training else 0.0)

    def fused(self, x, value, residual, drop):
        N, T, H, W, C = x.shape
        xv = x if value is None else value
        y = self.attn.self_attention(x.reshape(-1, C), xv.reshape(-1, C), self._cfg(N, T, H, W),
                                     None if residual is None else residual.reshape(-1, C), drop)
        return y.view(N, T, H, W, C)

    def forward(self, x, value=None):
        """x, value: (N,T,H,W,C) -> (N,T,H,W,C)"""
        return self.fused(x, value, None, ops.NO_DROP)

    def extra_repr(self):
        return f"dim={self.dim}, window_size={self.window_size}, num_heads={self.num_heads}"


class FrameLayerNorm(nn.Module):
    """Parameter holder for MlpDWBN's nn.LayerNorm((Ch,H,W)) (ref/models/VidHRFormer.py:347,359,366).  The activations
    on this path are channels-last [frame][H*W][Ch], so the per-element affine is STORED channels-last ([H*W*Ch] flat):
    the kernels read it coalesced, its gradient is accumulated in place in the flat gradient buffer, and the 352
    transpose launches per step of the first version (parameter re-layout forward, gradient re-layout backward) are
    gone.  AdamW / weight decay / the gradient norm are element-wise, i.e. layout independent.  The state-dict still
    shows the reference's (Ch,H,W) tensors - as strided VIEWS of the same storage, so checkpoints load / save
    unchanged and in-place fills through state_dict() reach the parameter."""

    def __init__(self, normalized_shape, eps=1e-5):
        super().__init__()
        self.normalized_shape = tuple(normalized_shape)
        self.eps = eps
        n = self.normalized_shape[0] * self.normalized_shape[1] * self.normalized_shape[2]
        self.weight = nn.Parameter(torch.ones(n))
        self.bias = nn.Parameter(torch.zeros(n))

    def ref_view(self, flat):
        """channels-last flat [H*W*Ch] -> the reference's (Ch,H,W) as a view"""
        Ch, H, W = self.normalized_shape
        return flat.view(H, W, Ch).permute(2, 0, 1)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        for name in ("weight", "bias"):
            p = getattr(self, name)
            destination[prefix + name] = self.ref_view(p if keep_vars else p.detach())

    def _load_from_state_dict(self, state_dict, prefix, *args):
        local = state_dict
        for name in ("weight", "bias"):
            k = prefix + name
            if k in state_dict and tuple(state_dict[k].shape) == self.normalized_shape:
                if local is state_dict:
                    local = dict(state_dict)            # never rewrite the caller's dict
                local[k] = state_dict[k].permute(1, 2, 0).reshape(-1)
        super()._load_from_state_dict(local, prefix, *args)

    def forward(self, h, residual=None, frames=None, p_drop=0.0, p_dp=0.0, frames_per_sample=1):
        """GELU(LayerNorm(h)) (+dropout, +residual, +drop-path) on channels-last h [frames, H*W*Ch] - the form the
        reference uses it in (always followed by the activation, ref :381-390)."""
        frames = h.shape[0] if frames is None else frames
        return ops.frameln_act(h, self.weight, self.bias, residual, frames, p_drop, p_dp, frames_per_sample)

    def extra_repr(self):
        return "{}, eps={}, storage=channels-last".format(self.normalized_shape, self.eps)


class MlpDWBN(nn.Module):
    """ref/models/VidHRFormer.py:326-392 (AR_model=True: LayerNorm((C,H,W)) variant).
    fc1/fc2 are GEMMs over the channels-last rows; each LayerNorm((Ch,H,W))+GELU(+dropout) is one
    statistics pass + one fused apply pass; the depthwise 3x3 works on [F, H*W, Ch] directly."""

    def __init__(self, encH, encW, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU,
                 dw_act_layer=nn.GELU, drop=0.0, AR_model=True):
        super().__init__()
        if not AR_model:
            raise NotImplementedError("only the AR_model=True (LayerNorm) variant is on the hot path")
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.encH, self.encW = encH, encW
        self.fc1 = nn.Conv2d(in_features, hidden_features, kernel_size=1)
        self.act1 = act_layer()
        self.norm1 = FrameLayerNorm((hidden_features, encH, encW))
        self.dw3x3 = nn.Conv2d(hidden_features, hidden_features, kernel_size=3, stride=1, groups=hidden_features, padding=1)
        self.act2 = dw_act_layer()
        self.norm2 = FrameLayerNorm((hidden_features, encH, encW))
        self.fc2 = nn.Conv2d(hidden_features, out_features, kernel_size=1)
        self.act3 = act_layer()
        self.norm3 = FrameLayerNorm((out_features, encH, encW))
        self.drop = nn.Dropout(drop)
        self.out_features = out_features

    def fused(self, x, residual, p_dp):
        N, T, H, W, C = x.shape
        F_, R = N * T, N * T * H * W
        pd = self.drop.p if self.training else 0.0
        hid = self.fc1.out_channels
        if ops.mlpdwbn_fused_supported(R, C, hid, self.out_features, H, W) and self.fc1.bias is not None:
            # one autograd node, fused middle (norm1 + GELU + depthwise 3x3 + norm2 statistics in one pass)
            out = ops.mlpdwbn(x.reshape(R, C), None if residual is None else residual.reshape(R, self.out_features),
                              self.fc1.weight.flatten(1), self.fc1.bias, self.norm1.weight, self.norm1.bias,
                              self.dw3x3.weight, self.dw3x3.bias, self.norm2.weight, self.norm2.bias,
                              self.fc2.weight.flatten(1), self.fc2.bias, self.norm3.weight, self.norm3.bias, F_, T, pd, p_dp)
            return out.view(N, T, H, W, self.out_features)
        # fc1 / the depthwise conv / fc2 hand the frame LayerNorm that follows them its statistics (no pass over h)
        if ops.linear_frame_stats_supported(R, hid) and H * W == 64:
            h, m1, r1 = ops.linear(x.reshape(R, C), self.fc1.weight.flatten(1), self.fc1.bias, frame_stats=True)
            a = ops.frameln_act(h, self.norm1.weight, self.norm1.bias, None, F_, stats=(m1, r1))
        else:
            h = ops.linear(x.reshape(R, C), self.fc1.weight.flatten(1), self.fc1.bias)
            a = ops.frameln_act(h, self.norm1.weight, self.norm1.bias, None, F_)
        wtb = torch.cat([ops._Transpose.apply(self.dw3x3.weight.reshape(1, hid, 9)).reshape(9, hid),
                         self.dw3x3.bias.reshape(1, hid)], dim=0)
        if H == 8 and W == 8 and hid % 1024 == 0:      # the convolution hands norm2 its frame statistics
            h, m2, r2 = ops.dwconv3x3(a, wtb, F_, H, W, want_stats=True)
            a = ops.frameln_act(h, self.norm2.weight, self.norm2.bias, None, F_, pd, stats=(m2, r2))
        else:
            h = ops.dwconv3x3(a, wtb, F_, H, W)
            a = ops.frameln_act(h, self.norm2.weight, self.norm2.bias, None, F_, pd)
        st3 = None
        if ops.linear_frame_stats_supported(R, self.out_features) and H * W == 64:
            h, m3, r3 = ops.linear(a.reshape(R, hid), self.fc2.weight.flatten(1), self.fc2.bias, frame_stats=True)
            st3 = (m3, r3)
        else:
            h = ops.linear(a.reshape(R, hid), self.fc2.weight.flatten(1), self.fc2.bias)
        out = ops.frameln_act(h, self.norm3.weight, self.norm3.bias,
                              None if residual is None else residual.reshape(R, self.out_features), F_, pd, p_dp, T, stats=st3)
        return out.view(N, T, H, W, self.out_features)

    def forward(self, x):
        """x: (N,T,H,W,C)"""
        return self.fused(x, None, 0.0)


class DropPath(nn.Module):
    """ref/models/VidHRFormer.py:528-542; kept for API parity.  Inside the blocks drop-path is fused
    into the producing kernel's epilogue, this module only records the probability."""

    def __init__(self, drop_prob=None):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        if not self.drop_prob or not self.training:
            return x
        x2 = x.reshape(x.shape[0], -1)
        pad = (-x2.shape[1]) % 4
        if pad:
            raise NotImplementedError("standalone DropPath needs a row length that is a multiple of 4")
        return ops.drop_apply(x2.contiguous(), Drop(self.drop_prob, 1, 1, x.shape[0])).view(x.shape)

    def extra_repr(self):
        return "drop_prob={}".format(self.drop_prob)


def _stock_fuser(pos_fuser):
    """the sub-layer nodes call the positional-fuse kernels directly: only for the stock PosFeatFuser('layer') (an 'instance'
    fuser or a user's own module goes through the per-kernel autograd path below)"""
    from .submodules import PosFeatFuser
    return type(pos_fuser) is PosFeatFuser and pos_fuser.norm_type == 'layer'


def _get_clones(module, N):
    return nn.ModuleList([copy.deepcopy(module) for _ in range(N)])


class VidHRFormerBlockEnc(nn.Module):
    """ref/models/VidHRFormer.py:54-116."""

    def __init__(self, encH, encW, embed_dim, num_heads, window_size=7, dropout=0., drop_path=0.,
                 Spatial_FFN_hidden_ratio=4, dim_feedforward=1024):
        super().__init__()
        self.embed_dim, self.num_heads, self.window_size, self.dropout = embed_dim, num_heads, window_size, dropout
        self.Spatial_FFN_hidden_ratio = Spatial_FFN_hidden_ratio
        self.SLMHSA = SpatialLocalMultiheadAttention(embed_dim, num_heads, window_size, dropout)
        self.SpatialFFN = MlpDWBN(encH, encW, embed_dim, hidden_features=int(Spatial_FFN_hidden_ratio * embed_dim),
                                  out_features=embed_dim, drop=dropout)
        self.norm1 = nn.LayerNorm(embed_dim)
        self.norm2 = nn.LayerNorm(embed_dim)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm3 = nn.LayerNorm(embed_dim)
        self.temporal_MHSA = MultiheadAttention(embed_dim, num_heads, dropout=dropout)
        self.linear1 = nn.Linear(embed_dim, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, embed_dim)
        self.activation = nn.GELU()
        self.drop1 = nn.Dropout(dropout) if dropout > 0. else nn.Identity()
        self.drop2 = nn.Dropout(dropout) if dropout > 0. else nn.Identity()
        self.drop3 = nn.Dropout(dropout) if dropout > 0. else nn.Identity()
        self.norm4 = nn.LayerNorm(embed_dim)
        self._dp = float(drop_path)

    def forward(self, x, memory_pos, pos_fuser):
        """x: (N,T,H,W,C) contiguous -> (N,T,H,W,C)."""
        N, T, H, W, C = x.shape
        P = H * W
        tr = self.training
        pd, dp = (self.dropout if tr else 0.0), (self._dp if tr else 0.0)
        beta, gamma = memory_pos
        x = x.contiguous()
        if _stock_fuser(pos_fuser):
            # one autograd node per residual sub-layer (ops._SelfAttnSublayer / _MlpDwbn / _FfnSublayer)
            x = ops.self_attn_sublayer(x, self.norm1, beta, gamma, None, self.SLMHSA.attn, self.SLMHSA._cfg(N, T, H, W),
                                       Drop(dp, 1, T * P, N), N, T)                                              # ref :87-88
            x, x1 = ops.layernorm_res(x, self.norm2.weight, self.norm2.bias, self.norm2.eps)
            x = self.SpatialFFN.fused(x1, x, dp)                                                                  # ref :91
            x = ops.self_attn_sublayer(x, self.norm3, beta, gamma, None, self.temporal_MHSA,
                                       AttnCfg(1, N, P, W, 0, T, T, self.num_heads, 1, pd), Drop(pd), N, T)       # ref :94-107
            return ops.ffn_sublayer(x, self.norm4, self.linear1, self.linear2, pd)                                # ref :110-112
        # spatial window attention: x += drop_path(SLMHSA(fuse(LN1 x), value = LN1 x))           ref :87-88
        x, x1 = ops.layernorm_res(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        x = self.SLMHSA.fused(pos_fuser(x1, beta, gamma), x1, x, Drop(dp, 1, T * P, N))
        # conv feed-forward: x += drop_path(MlpDWBN(LN2 x))                                       ref :91
        x, x1 = ops.layernorm_res(x, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        x = self.SpatialFFN.fused(x1, x, dp)
        # temporal attention with the encoder mask: x += drop1(tMHA(q=k=fuse(LN3 x), v=LN3 x))    ref :94-107
        x, x1 = ops.layernorm_res(x, self.norm3.weight, self.norm3.bias, self.norm3.eps)
        temp = pos_fuser(x1, beta, gamma)
        cfg = AttnCfg(1, N, P, W, 0, T, T, self.num_heads, 1, pd)
        x = self.temporal_MHSA.self_attention(temp.reshape(-1, C), x1.reshape(-1, C), cfg, x.reshape(-1, C),
                                              Drop(pd)).view(N, T, H, W, C)
        # token FFN: x += drop3(linear2(drop2(GELU(linear1(LN4 x)))))                             ref :110-112
        x, x1 = ops.layernorm_res(x, self.norm4.weight, self.norm4.bias, self.norm4.eps)
        return ops.ffn(x1, x, self.linear1.weight, self.linear1.bias, self.linear2.weight, self.linear2.bias, pd)


class VidHRFormerEncoder(nn.Module):
    """ref/models/VidHRFormer.py:11-52.  evt_token=True (ref :22-23, :35-42): the learned parameter EVT (1,H,W,C) is appended to every
    clip as frame T+1, with zero positional rows for that frame; the layers and the shared norm run on T+1 frames.  The temporal mask
    of the blocks (ref :99-102: no query but the last sees the last key) is this token's mask: the frames never see the token, the
    token sees every frame."""

    def __init__(self, num_layers, enc_H, enc_W, d_model, num_heads, window_size=7, dropout=0., drop_path=0.,
                 Spatial_FFN_hidden_ratio=4, dim_feedforward=1024, norm=None, evt_token=False):
        super().__init__()
        self.layers = _get_clones(VidHRFormerBlockEnc(enc_H, enc_W, d_model, num_heads, window_size, dropout, drop_path,
                                                      Spatial_FFN_hidden_ratio, dim_feedforward), num_layers)
        self.num_layers, self.norm, self.evt_token = num_layers, norm, evt_token
        if self.evt_token:
            self.EVT = nn.Parameter(torch.randn(1, enc_H, enc_W, d_model), requires_grad=True)          # ref :23

    def forward_canonical(self, x, memory_pos, pos_fuser):
        """x: (N,T,H,W,C) canonical -> (N,T,H,W,C) canonical (after the shared final LayerNorm); with the event token (N,T+1,H,W,C),
        frame T being the token's."""
        if self.evt_token:
            N, T, H, W, C = x.shape
            if N * (T + 1) * H * W % 32:
                raise ValueError(f"VidHRFormerEncoder(evt_token=True): the residual stream has N*(T+1)*H*W = {N}*{T + 1}*{H}*{W} token "
                                 "rows, and the weight-gradient GEMMs sum over them in steps of 32: N*(T+1)*H*W % 32 must be 0")
            x = ops.evt_token_join(x, self.EVT)                                                          # ref :36
            beta, gamma = memory_pos
            memory_pos = (ops.evt_pad_table(beta, T), ops.evt_pad_table(gamma, T))                       # ref :39-42
        for layer in self.layers:
            x = layer(x, memory_pos, pos_fuser)
        if self.norm is not None:
            x = ops.layernorm(x, self.norm.weight, self.norm.bias, self.norm.eps)
        return x

    def forward(self, src, memory_pos, pos_fuser):
        """src: (N,T,C,H,W) -> (N,T,C,H,W), or (N,T+1,C,H,W) with the event token   (reference signature)"""
        N, T, C, H, W = src.shape
        x = ops.nchw_to_canonical(src).view(N, T, H, W, C)
        x = self.forward_canonical(x, memory_pos, pos_fuser)
        return ops.canonical_to_nchw(x, N, x.shape[1], H, W)


class VidHRFormerBlockDecNAR(nn.Module):
    """ref/models/VidHRFormer.py:163-245."""

    def __init__(self, encH, encW, embed_dim, num_heads, window_size=7, dropout=0., drop_path=0.,
                 Spatial_FFN_hidden_ratio=4, dim_feedforward=1024):
        super().__init__()
        self.embed_dim, self.num_heads, self.window_size, self.dropout = embed_dim, num_heads, window_size, dropout
        self.Spatial_FFN_hidden_ratio = Spatial_FFN_hidden_ratio
        hid = int(Spatial_FFN_hidden_ratio * embed_dim)
        self.SLMHSA = SpatialLocalMultiheadAttention(embed_dim, num_heads, window_size, dropout)
        self.SpatialFFN = MlpDWBN(encH, encW, embed_dim, hidden_features=hid, out_features=embed_dim, drop=dropout)
        self.norm1 = nn.LayerNorm(embed_dim)
        self.norm2 = nn.LayerNorm(embed_dim)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm3 = nn.LayerNorm(embed_dim)
        self.temporal_MHSA = MultiheadAttention(embed_dim, num_heads, dropout=dropout)
        self.drop1 = nn.Dropout(dropout) if dropout > 0. else nn.Identity()
        self.linear1 = nn.Linear(embed_dim, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, embed_dim)
        self.activation = nn.GELU()
        self.drop2 = nn.Dropout(dropout) if dropout > 0. else nn.Identity()
        self.drop3 = nn.Dropout(dropout) if dropout > 0. else nn.Identity()
        self.norm4 = nn.LayerNorm(embed_dim)
        self.EncDecAttn = MultiheadAttention(embed_dim, num_heads, dropout=dropout)
        self.SpatialFFN1 = MlpDWBN(encH, encW, embed_dim, hidden_features=hid, out_features=embed_dim, drop=dropout)
        self.norm5 = nn.LayerNorm(embed_dim)
        self.norm6 = nn.LayerNorm(embed_dim)
        self.drop_path1 = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self._dp = float(drop_path)

    def forward(self, tgt, query_evt, memory, memory_pos, tgt_pos, pos_fuser, fused_memory=None):
        """tgt (N,T2,H,W,C); query_evt (N,H,W,C) = z (the reference repeats it over T2, ref Predictor.py:317:
        a (N,T2,H,W,C) tensor whose time-steps are identical is accepted too); memory (N,T1,H,W,C).
        fused_memory = pos_fuser(memory, *memory_pos), layer invariant (ref :232), hoisted by the decoder."""
        N, T2, H, W, C = tgt.shape
        T1, P = memory.shape[1], H * W
        if query_evt.dim() == 5:
            if query_evt.shape[1] > 1 and not torch.equal(query_evt[:, 1:], query_evt[:, :1].expand_as(query_evt[:, 1:])):
                raise NotImplementedError("VidHRFormerBlockDecNAR: query_evt differs between time-steps (see VidHRformerDecoderNAR.forward)")
            query_evt = query_evt[:, 0]
        query_evt = query_evt.contiguous()
        tr = self.training
        pd, dp = (self.dropout if tr else 0.0), (self._dp if tr else 0.0)
        tb, tg = tgt_pos
        tgt = tgt.contiguous()
        if _stock_fuser(pos_fuser):
            x = ops.self_attn_sublayer(tgt, self.norm1, tb, tg, query_evt, self.SLMHSA.attn, self.SLMHSA._cfg(N, T2, H, W),
                                       Drop(dp, 1, T2 * P, N), N, T2)                                             # ref :210-212
            x, x1 = ops.layernorm_res(x, self.norm2.weight, self.norm2.bias, self.norm2.eps)
            x = self.SpatialFFN.fused(x1, x, dp)                                                                  # ref :214
            x = ops.self_attn_sublayer(x, self.norm3, tb, tg, None, self.temporal_MHSA,
                                       AttnCfg(1, N, P, W, 0, T2, T2, self.num_heads, 0, pd), Drop(pd), N, T2)    # ref :217-221
            x = ops.ffn_sublayer(x, self.norm4, self.linear1, self.linear2, pd)                                   # ref :224-226
            key = fused_memory if fused_memory is not None else pos_fuser(memory, *memory_pos)
            # encoder-decoder attention; its drop_path acts per TIME-STEP (tensor is (T2, N*H*W, C))               ref :229-239
            x = ops.cross_attn_sublayer(x, self.norm5, tb, tg, query_evt, key, memory, self.EncDecAttn,
                                        AttnCfg(1, N, P, W, 0, T2, T1, self.num_heads, 0, pd), Drop(dp, 1, P, T2), N, T2)
            x, x1 = ops.layernorm_res(x, self.norm6.weight, self.norm6.bias, self.norm6.eps)
            return self.SpatialFFN1.fused(x1, x, dp)                                                              # ref :243
        # spatial window attention over fuse(LN1 tgt + query_evt), value LN1 tgt                  ref :210-212
        tgt, t2 = ops.layernorm_res(tgt, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        x = self.SLMHSA.fused(pos_fuser(t2, tb, tg, add=query_evt), t2, tgt, Drop(dp, 1, T2 * P, N))
        x, x1 = ops.layernorm_res(x, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        x = self.SpatialFFN.fused(x1, x, dp)                                                                     # :214
        # temporal self-attention (no mask)                                                       ref :217-221
        x, x1 = ops.layernorm_res(x, self.norm3.weight, self.norm3.bias, self.norm3.eps)
        temp = pos_fuser(x1, tb, tg)
        cfg = AttnCfg(1, N, P, W, 0, T2, T2, self.num_heads, 0, pd)
        x = self.temporal_MHSA.self_attention(temp.reshape(-1, C), x1.reshape(-1, C), cfg, x.reshape(-1, C),
                                              Drop(pd)).view(N, T2, H, W, C)
        x, x1 = ops.layernorm_res(x, self.norm4.weight, self.norm4.bias, self.norm4.eps)                         # :224-226
        x = ops.ffn(x1, x, self.linear1.weight, self.linear1.bias, self.linear2.weight, self.linear2.bias, pd)
        # encoder-decoder attention; its drop_path acts per TIME-STEP (tensor is (T2, N*H*W, C))   ref :229-239
        x, x1 = ops.layernorm_res(x, self.norm5.weight, self.norm5.bias, self.norm5.eps)
        key = fused_memory if fused_memory is not None else pos_fuser(memory, *memory_pos)
        query = pos_fuser(x1, tb, tg, add=query_evt)
        cfg = AttnCfg(1, N, P, W, 0, T2, T1, self.num_heads, 0, pd)
        x = self.EncDecAttn.cross_attention(query.reshape(-1, C), key.reshape(-1, C), memory.reshape(-1, C), cfg,
                                            x.reshape(-1, C), Drop(dp, 1, P, T2)).view(N, T2, H, W, C)
        x, x1 = ops.layernorm_res(x, self.norm6.weight, self.norm6.bias, self.norm6.eps)
        return self.SpatialFFN1.fused(x1, x, dp)                                                                     # :243

    def forward_samples(self, tgt, query_evt, memory, memory_pos, tgt_pos, pos_fuser, fused_memory, samples):
        """The sampler's route (forward only, eval behaviour, stock fuser): tgt (S*N,T2,H,W,C) and query_evt (S*N,H,W,C) hold
        S = `samples` draws per clip, sample-major (clip s*N + n); memory / fused_memory stay at the N clips (N,T1,H,W,C).  `forward`
        in eval mode, sub-layer for sub-layer, on the batch S*N - except the encoder-decoder site, whose K / V side is shared by a
        clip's samples (ops.cross_attn_samples) instead of replicated."""
        B, T2, H, W, C = tgt.shape
        S = int(samples)
        N, T1, P = memory.shape[0], memory.shape[1], H * W
        if self.training:
            raise RuntimeError("VidHRFormerBlockDecNAR.forward_samples: the sampler has eval behaviour only (call .eval() first)")
        if B != S * N or not _stock_fuser(pos_fuser):
            raise ValueError("VidHRFormerBlockDecNAR.forward_samples: tgt must hold samples * N clips, and the stock PosFeatFuser('layer')")
        tb, tg = tgt_pos
        tgt, query_evt = tgt.contiguous(), query_evt.contiguous()
        nd = ops.NO_DROP
        x = ops.self_attn_sublayer(tgt, self.norm1, tb, tg, query_evt, self.SLMHSA.attn, self.SLMHSA._cfg(B, T2, H, W), nd, B, T2)
        x, x1 = ops.layernorm_res(x, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        x = self.SpatialFFN.fused(x1, x, 0.0)
        x = ops.self_attn_sublayer(x, self.norm3, tb, tg, None, self.temporal_MHSA,
                                   AttnCfg(1, B, P, W, 0, T2, T2, self.num_heads, 0, 0.0), nd, B, T2)
        x = ops.ffn_sublayer(x, self.norm4, self.linear1, self.linear2, 0.0)
        x = ops.cross_attn_samples(x, self.norm5, tb, tg, query_evt, fused_memory, memory, self.EncDecAttn,
                                   AttnCfg(1, N, P, W, 0, T2, T1, self.num_heads, 0, 0.0), S, N, T2)              # ref :229-239
        x, x1 = ops.layernorm_res(x, self.norm6.weight, self.norm6.bias, self.norm6.eps)
        return self.SpatialFFN1.fused(x1, x, 0.0)


class VidHRformerDecoderNAR(nn.Module):
    """ref/models/VidHRFormer.py:118-161 (return_intermediate=False)."""

    def __init__(self, num_layers, encH, encW, embed_dim, num_heads, window_size=7, dropout=0., drop_path=0.,
                 Spatial_FFN_hidden_ratio=4, dim_feedforward=1024, norm=None, return_intermediate=False):
        super().__init__()
        if return_intermediate:
            raise NotImplementedError("return_intermediate is never used by the predictor")
        self.layers = _get_clones(VidHRFormerBlockDecNAR(encH, encW, embed_dim, num_heads, window_size, dropout, drop_path,
                                                         Spatial_FFN_hidden_ratio, dim_feedforward), num_layers)
        self.num_layers, self.norm, self.return_intermediate = num_layers, norm, return_intermediate

    def forward_canonical(self, qe, memory, memory_pos, tgt_pos, pos_fuser, T2, nchw=False, samples=1):
        """qe (N,H,W,C), memory (N,T1,H,W,C) canonical -> (N,T2,H,W,C) canonical, after LN + ReLU
        (nchw=True: the reference's (N,T2,C,H,W) layout instead).
        samples = S > 1 (forward only, eval behaviour): qe (S*N,H,W,C) holds S event latents per clip, sample-major (clip s*N + n), memory
        stays at N clips; -> (S*N,T2,...).  Memory, its fused form and every layer's K / V projection are never repeated S times."""
        if samples != 1:
            return self._forward_samples(qe, memory, memory_pos, tgt_pos, pos_fuser, T2, nchw, int(samples))
        N, H, W, C = qe.shape
        out = torch.zeros(N, T2, H, W, C, dtype=torch.float32, device=qe.device)
        # memory and its fused form are the key / value sources of all the layers' encoder-decoder attention: fan_out lets the
        # layers' dgrad GEMMs sum their gradients in place (ops.ActSink)
        fused_memory = ops.fan_out(pos_fuser(memory, *memory_pos))
        memory = ops.fan_out(memory)
        for layer in self.layers:
            out = layer(out, qe, memory, memory_pos, tgt_pos, pos_fuser, fused_memory)
        if nchw and self.norm is not None and ops.layernorm_nchw_supported(out, H, W):
            # K9: the final norm + ReLU writes the reference's (N,T,C,H,W) layout itself (no transpose kernel)
            return ops.layernorm_nchw(out, self.norm.weight, self.norm.bias, self.norm.eps, True, N, T2, H, W)
        if self.norm is not None:
            out = ops.layernorm(out, self.norm.weight, self.norm.bias, self.norm.eps, relu=True)
        else:
            out = torch.relu(out)
        return ops.canonical_to_nchw(out, N, T2, H, W) if nchw else out

    def _final(self, out, B, T2, H, W, nchw):
        if nchw and self.norm is not None and ops.layernorm_nchw_supported(out, H, W):
            return ops.layernorm_nchw(out, self.norm.weight, self.norm.bias, self.norm.eps, True, B, T2, H, W)
        if self.norm is not None:
            out = ops.layernorm(out, self.norm.weight, self.norm.bias, self.norm.eps, relu=True)
        else:
            out = torch.relu(out)
        return ops.canonical_to_nchw(out, B, T2, H, W) if nchw else out

    def _forward_samples(self, qe, memory, memory_pos, tgt_pos, pos_fuser, T2, nchw, S):
        B, H, W, C = qe.shape
        N = memory.shape[0]
        if S < 1 or B != S * N:
            raise ValueError(f"VidHRformerDecoderNAR: samples={S} needs qe of samples * N = {S * N} clips, got {B}")
        if (torch.is_grad_enabled() and (qe.requires_grad or memory.requires_grad)) or self.training:
            raise RuntimeError("VidHRformerDecoderNAR: the sampled route is forward only with eval behaviour (no_grad, .eval())")
        fused_memory = pos_fuser(memory, *memory_pos)
        if not _stock_fuser(pos_fuser):
            # another fuser: per-sample calls of the existing path (memory and its fused form still made once)
            outs = []
            for s in range(S):
                out = torch.zeros(N, T2, H, W, C, dtype=torch.float32, device=qe.device)
                for layer in self.layers:
                    out = layer(out, qe[s * N:(s + 1) * N], memory, memory_pos, tgt_pos, pos_fuser, fused_memory)
                outs.append(out)
            return self._final(torch.cat(outs, 0), B, T2, H, W, nchw)
        out = torch.zeros(B, T2, H, W, C, dtype=torch.float32, device=qe.device)
        for layer in self.layers:
            out = layer.forward_samples(out, qe, memory, memory_pos, tgt_pos, pos_fuser, fused_memory, S)
        return self._final(out, B, T2, H, W, nchw)

    def forward(self, query_evt, memory, memory_pos, tgt_pos, pos_fuser):
        """query_evt (N,T2,C,H,W), memory (N,T1,C,H,W) -> (N,T2,C,H,W)   (reference signature)"""
        N, T2, C, H, W = query_evt.shape
        T1 = memory.shape[1]
        # The kernels add ONE (N,H,W,C) event latent to every time-step (what the predictor passes: z repeated over T2,
        # ref Predictor.py:317).  The reference's signature would also take a query that differs from step to step; silently
        # keeping step 0 of such a tensor would be a wrong answer, so it is refused (one device comparison at this API edge -
        # Predictor.forward goes through forward_canonical and never pays it).
        if T2 > 1 and not query_evt.is_meta and not torch.equal(query_evt[:, 1:], query_evt[:, :1].expand(-1, T2 - 1, -1, -1, -1)):
            raise NotImplementedError("VidHRformerDecoderNAR.forward: query_evt differs between time-steps; this build adds one "
                                      "(N,C,H,W) event latent to all T2 steps (the only form the predictor produces)")
        qe = ops.nchw_to_canonical(query_evt[:, :1]).view(N, H, W, C)
        mem = ops.nchw_to_canonical(memory).view(N, T1, H, W, C)
        return self.forward_canonical(qe, mem, memory_pos, tgt_pos, pos_fuser, T2, nchw=True)
