"""HIP-backed NP predictor: drop-in for ref/models/Predictor.py:265-359 (`Predictor`).  Same
constructor signature, attributes (`stochastic`, `TP`, `observed_coor`, `predict_coor`, `nrmlp`, `fuser`,
`EVT_Former`, `evt_posterior`, `evt_prior`, `transformer`), methods and the 603 state-dict keys (604 with learn_evt_token=True:
`EVT_Former.EVT`), so reference checkpoints load with load_state_dict and LitPredictor-style callers keep working.
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
        if not evt_former:
            raise NotImplementedError("evt_former=False is not built: the reference's branch (ref/models/Predictor.py:348) feeds the "
                                      "fuser an (N,T,W,C,H) permutation of the features, which only runs because H = W = 8 reshapes "
                                      "without error; it normalises over whole frames and indexes the positional tables scrambled, "
                                      "so it defines nothing worth restating.  Use evt_former=True (with or without learn_evt_token)")
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
    def _encode(self, feats, pos, memory=True):
        """(N,T,C,H,W) features -> canonical encoder output (N,T,H,W,C) and event coding [N, H*W, C]: the mean over T, or with the
        learned event token the encoder's last output frame, the first T being the memory (ref :343-346).  memory=False: the caller
        uses the event coding alone (the target pass); with the token the memory is then not produced (an empty tensor)."""
        N, T, C, H, W = feats.shape
        x = ops.nchw_to_canonical(feats).view(N, T, H, W, C)
        x = self.EVT_Former.forward_canonical(x, pos, self.fuser)
        if self.EVT_Former.evt_token:
            return ops.evt_token_split(x, memory)                                       # ref :344
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
                    _, pred_evt = self._encode(predict_features_gt, pp, memory=False)
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
                    _, pred_evt = self._encode(predict_features_gt, pp, memory=False)
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

    # -- the stochastic model as a sampler: S futures per clip, the context encoded once ---------------
    SAMPLE_SALT = 0x53414D50          # the sampler's stream of the counter hash (dropout sites count 1, 2, ... per step)

    def sample_seed_tensor(self, seed, dev):
        """the device-resident seed of the sampler: the scheduling context's seed tensor (seed None), or a tensor of the sampler's
        own that receives the given int (a device fill: no host read, and the trainer's mask stream is left alone)"""
        if seed is None:
            return ops.current().rng.seed_tensor(dev)
        t = getattr(self, "_sample_seed", None)
        if t is None or t.device != dev:
            t = self._sample_seed = torch.zeros(1, dtype=torch.int64, device=dev)
        t.fill_(int(seed) & 0x7FFFFFFFFFFFFFFF)
        return t

    def sample_context(self, observed_features):
        """Everything of a sampled forward that depends on the context only, run ONCE whatever the number of samples: positional
        tables, the EVT_Former encoder, the prior head (ref Predictor.py:312-321 up to the draw).  Call under no_grad in eval
        mode (`sample` does); -> the state `sample_decode` takes."""
        if not self.stochastic:
            raise ValueError("Predictor.sample needs a stochastic predictor (stochastic=True): a deterministic one has one future")
        H, W = observed_features.shape[-2:]
        op = self._pos(self.observed_coor)
        pp = self._pos(self.predict_coor)
        memory, obs_evt = self._encode(observed_features, op)
        _, mu, logvar = self.evt_prior.forward_canonical(obs_evt, H, W, draw=False)
        return dict(memory=memory, mu=mu, logvar=logvar, op=op, pp=pp, HW=(H, W))

    def sample_decode(self, ctx, n_samples, seed_t, sample_base=0, return_eps=False):
        """S = n_samples futures from one `sample_context`: z [S, N, H*W, C] from the device sampler (samples sample_base ..
        sample_base + S - 1 of the stream of `seed_t`), the decoder on S*N clips, sample-major, against the N-clip memory.
        -> (N, S, Tp, C, H, W), a permuted view of the sample-major result (S*N, Tp, C, H, W); with return_eps also eps and z
        [S, N, H*W, C] (canonical layout)."""
        S = int(n_samples)
        if S < 1:
            raise ValueError("Predictor.sample: n_samples must be at least 1")
        memory, mu = ctx["memory"], ctx["mu"]
        N, T1, H, W, C = memory.shape
        z = ops.reparam_samples(mu, ctx["logvar"], S, seed_t, self.SAMPLE_SALT, sample_base, return_eps)
        z, eps = z if return_eps else (z, None)
        out = self.transformer.forward_canonical(z.view(S * N, H, W, C), memory, ctx["op"], ctx["pp"], self.fuser, self.TP, nchw=True,
                                                 samples=S)
        out = out.view(S, N, self.TP, C, H, W).permute(1, 0, 2, 3, 4, 5)
        return (out, eps, z) if return_eps else out

    def sample(self, observed_features, n_samples, seed=None, sample_base=0, return_eps=False, arithmetic=None):
        """observed_features (N, To, C, H, W) -> n_samples futures per clip, (N, S, Tp, C, H, W) [, eps [S, N, H*W, C]].
        The eval forward (ref Predictor.py:312-322) with S draws of zo instead of one: positional tables, encoder and prior
        head run once, the latent comes from the device sampler (ops.reparam_samples; `evt_prior.eps_fn` is not consulted), the
        decoder runs on S*N clips against the N-clip memory.  seed None: the scheduling context's device seed; an int: that value.
        Sample sample_base + s of a seed is the same latent however S is cut into calls.  Runs under no_grad with eval
        behaviour; the module's train / eval state is restored.  arithmetic (None = the GEMM mode as it is, or a name
        ops.eval_arithmetic takes): "f16x1" runs the context encoding and the decode in the one-term fp16 arithmetic."""
        if not self.stochastic:
            raise ValueError("Predictor.sample needs a stochastic predictor (stochastic=True): a deterministic one has one future")
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad(), ops.arithmetic_scope(arithmetic):
                ctx = self.sample_context(observed_features)
                seed_t = self.sample_seed_tensor(seed, observed_features.device)
                res = self.sample_decode(ctx, n_samples, seed_t, sample_base, return_eps)
        finally:
            self.train(was_training)
        return (res[0], res[1]) if return_eps else res

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
