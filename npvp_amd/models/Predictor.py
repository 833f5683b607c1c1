"""HIP-backed NP predictor: drop-in for ref/models/Predictor.py:265-359 (`Predictor`).  Same
constructor signature, attributes (`stochastic`, `TP`, `observed_coor`, `predict_coor`, `nrmlp`, `fuser`,
`EVT_Former`, `evt_posterior`, `evt_prior`, `transformer`), methods and the 603 state-dict keys,
so reference checkpoints load with load_state_dict and LitPredictor-style callers keep working.
"""
import torch
import torch.nn as nn

from .. import ops
from .submodules import CoorGenerator, NRMLP, PosFeatFuser, EventEncoder
from .VidHRFormer import VidHRformerDecoderNAR, VidHRFormerEncoder


class Predictor(nn.Module):
    def __init__(self, max_H, max_W, max_T, h_list, w_list, to_list, tp_list, embed_dim=512, fuse_method='SPADE',
                 param_free_norm_type='layer', evt_hidden_channels=256, evt_n_layers=1, stochastic=True,
                 transformer_layers=4, num_heads=8, window_size=4, dropout=0.1, drop_path=0.1,
                 Spatial_FFN_hidden_ratio=4, dim_feedforward=1024, norm=None, return_intermediate=False, evt_former=True,
                 learn_evt_token=False, evt_former_num_layers=4, rand_context=False):
        super().__init__()
        if norm is None:
            # the reference's default argument is ONE nn.LayerNorm(512) instance shared by the encoder and
            # the decoder (ref Predictor.py:270,290-291,299): a single tied weight under two state-dict keys
            norm = nn.LayerNorm(512)
        if not evt_former or learn_evt_token:
            raise NotImplementedError("evt_former=False / learn_evt_token=True are outside the hot path")
        self.stochastic, self.evt_former = stochastic, evt_former
        self.h_list, self.w_list = h_list, w_list
        self.max_H, self.max_W = max_H, max_W
        self.coor_generator = CoorGenerator(max_H, max_W, max_T)
        if not rand_context:
            self.register_buffer("observed_coor", self.coor_generator(to_list, h_list, w_list))
            self.register_buffer("predict_coor", self.coor_generator(tp_list, h_list, w_list))
        else:
            # unified model (ref :281-284): the caller picks the context / target time-steps per batch and points
            # observed_coor / predict_coor / TP at rows of `all_coor` (trainer.rand_context_batch_process); the kernels
            # take the sequence lengths at run time (any To, Tp: up to 32 on the MFMA attention kernels, 33 .. 128 on the generic route, above
            # that on the streaming kernels - no upper bound but the 32-bit check on token rows)
            self.observed_coor = None
            self.predict_coor = None
            self.register_buffer("all_coor", self.coor_generator(torch.cat([to_list, tp_list]), h_list, w_list)
                                 .reshape(max_T, max_H, max_W, 3))
        self.nrmlp = NRMLP(out_channels=embed_dim, fuse_method=fuse_method)
        self.fuser = PosFeatFuser(x_channels=embed_dim, param_free_norm_type=param_free_norm_type)
        self.EVT_Former = VidHRFormerEncoder(evt_former_num_layers, max_H, max_W, embed_dim, num_heads, window_size, dropout,
                                             drop_path, Spatial_FFN_hidden_ratio, dim_feedforward, norm, learn_evt_token)
        self.evt_posterior = EventEncoder(embed_dim, evt_hidden_channels, evt_n_layers, stochastic)
        self.evt_prior = None
        if self.stochastic:
            self.evt_prior = EventEncoder(embed_dim, evt_hidden_channels, evt_n_layers, stochastic)
        self.TP = tp_list.shape[0]
        self.transformer = VidHRformerDecoderNAR(transformer_layers, max_H, max_W, embed_dim, num_heads, window_size, dropout,
                                                 drop_path, Spatial_FFN_hidden_ratio, dim_feedforward, norm, return_intermediate)

    def _pos(self, coor):
        """(beta, gamma) tables; for fuse_method 'Add' gamma is identically zero (ref submodules.py:309-312) and
        x*(1+0) is exact, so the fuser kernel is told to skip it."""
        beta, gamma = self.nrmlp(coor)
        # (fan_out: the tables feed every sub-layer - their gradient is summed in place by the consumers, ops.ActSink)
        return (ops.fan_out(beta), ops.fan_out(gamma) if self.nrmlp.fuse_method == 'SPADE' else None)

    # -- helpers on the canonical layout -------------------------------------------------------------
    def _encode(self, feats, pos):
        """(N,T,C,H,W) features -> canonical encoder output (N,T,H,W,C) and event coding [N, H*W, C] (mean over T)."""
        N, T, C, H, W = feats.shape
        x = ops.nchw_to_canonical(feats).view(N, T, H, W, C)
        x = self.EVT_Former.forward_canonical(x, pos, self.fuser)
        evt = ops.mean_mid(x.view(N, T, H * W * C)).view(N, H * W, C)                  # ref :346
        return x, evt

    def _decode(self, z, memory, op, pp):
        """z [N, H*W, C] canonical"""
        N, T1, H, W, C = memory.shape
        zc = ops.fan_out(z.view(N, H, W, C))           # (16 consumers in the decoder: summed in place, ops.ActSink)
        return self.transformer.forward_canonical(zc, memory, op, pp, self.fuser, self.TP, nchw=True)

    def _nchw(self, t):
        N, P, C = t.shape
        return ops._Transpose.apply(t).view(N, C, self.max_H, self.max_W)

    def forward(self, observed_features, predict_features_gt=None):
        """observed_features: (N, To, C, H, W) -> (N, Tp, C, H, W) [, mu_o, logvar_o, mu_p, logvar_p]"""
        H, W = observed_features.shape[-2:]
        op = self._pos(self.observed_coor)
        pp = self._pos(self.predict_coor)
        dual = (self.stochastic and predict_features_gt is not None and ops.AuxStream.enabled
                and observed_features.is_cuda and torch.is_grad_enabled())
        if dual:
            # the target pass (posterior) is independent of the context pass (prior): second HIP stream
            dev = observed_features.device
            main, aux = torch.cuda.current_stream(dev), ops.AuxStream.stream(dev)
            aux.wait_stream(main)
            ops.AuxStream.active = True
            try:
                with torch.cuda.stream(aux):
                    _, pred_evt = self._encode(predict_features_gt, pp)
                    zp, mu_p, logvar_p = self.evt_posterior.forward_canonical(pred_evt, H, W)
                for t in (predict_features_gt, pp[0]) + ((pp[1],) if pp[1] is not None else ()):
                    t.record_stream(aux)
                memory, obs_evt = self._encode(observed_features, op)
                zo, mu_o, logvar_o = self.evt_prior.forward_canonical(obs_evt, H, W)
            finally:
                ops.AuxStream.active = False
            main.wait_stream(aux)
            for t in (zp, mu_p, logvar_p):
                t.record_stream(main)
        else:
            memory, obs_evt = self._encode(observed_features, op)
        if self.stochastic:
            if not dual:
                zo, mu_o, logvar_o = self.evt_prior.forward_canonical(obs_evt, H, W)
                if predict_features_gt is not None:
                    _, pred_evt = self._encode(predict_features_gt, pp)
                    zp, mu_p, logvar_p = self.evt_posterior.forward_canonical(pred_evt, H, W)
            if self.training:
                assert predict_features_gt is not None, \
                    "please input groundtruth predict features for storchastic model training/val"
                out = self._decode(zp, memory, op, pp)
            else:
                out = self._decode(zo, memory, op, pp)
            if predict_features_gt is None:
                return out
            return out, self._nchw(mu_o), self._nchw(logvar_o), self._nchw(mu_p), self._nchw(logvar_p)
        mu_o = self.evt_posterior.forward_canonical(obs_evt, H, W)
        return self._decode(mu_o, memory, op, pp)

    def evt_coding_forward(self, x, pos_beta, pos_gamma):
        """x (N,T,C,H,W) -> (encoder output (N,T,C,H,W), event coding (N,C,H,W))   ref :337-350"""
        N, T, C, H, W = x.shape
        mem, evt = self._encode(x, (pos_beta, pos_gamma))
        return ops.canonical_to_nchw(mem, N, T, H, W), self._nchw(evt)

    def reset_pos_coor(self, to_list, tp_list):
        device = self.observed_coor.device if self.observed_coor is not None else self.all_coor.device
        self.predict_coor = self.coor_generator(tp_list, self.h_list, self.w_list).to(device)
        self.observed_coor = self.coor_generator(to_list, self.h_list, self.w_list).to(device)
        self.TP = tp_list.shape[0]
