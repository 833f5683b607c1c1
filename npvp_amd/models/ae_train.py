"""Trainable Stage-1 autoencoder (LitAE, ref/models/ResNetAutoEncoder.py:13-49): the same ResnetEncoder / ResnetDecoder modules, with
the same state-dict keys, run through the HIP ops of csrc/ae_train.hip instead of stock torch:
  [pad] conv [BatchNorm2d [ReLU]] [+ skip]  ->  ops.reflect_pad, the convolution (MIOpen), ops.bn_act_train (statistics + one apply
                                               pass, skip-add fused)
  NonLocalAttenion2D                        ->  one GEMM for [Wq | Wk | Wv] (ops.linear), ops.nonlocal_attn_any_packed (the exact-tile kernels at
                                               the configs' own grids, the any-grid ones at any other; pooling fused, no score
                                               matrix in HBM), out_proj (ops.linear), ops.bn_act_train + ReLU, x + gamma * h
  learn_3d: temporal_conv                   ->  the Conv1d over T as a conv2d with a [C, C, 3, 1] filter on the channels-last frames viewed as
                                               (N, C, T, H*W) (MIOpen, no permute copy), BatchNorm1d through the same ops.bn_act_train
            NonLocalAttenion1D              ->  one GEMM for [Wq | Wk | Wv], ops.temporal_attn_any_packed on the same token rows (csrc/ae_temporal.hip),
                                               out_proj, ops.bn_act_train + ReLU, x + gamma * h
`prepare_trainable_autoencoder` binds these forwards to the two module INSTANCES; the classes, their forward methods and the frozen
Stage-2 path (build_frozen_autoencoder / fuse_frozen_autoencoder) are untouched.
"""
import types

import torch
import torch.nn as nn

from .. import dp, ops
from .ResNetAutoEncoder import (ResnetEncoder, ResnetDecoder, Factorized3DConvAttn, NonLocalAttenion2D, ResnetBlock, _temporal_view,
                                _temporal_view_back)


def build_autoencoder(AE, img_channels):
    """(encoder, decoder) as LitAE.__init__ builds them (ref/models/ResNetAutoEncoder.py:14-19) from the `AE:` section of a reference
    YAML: parameters require grad, train mode."""
    enc = ResnetEncoder(img_channels, ngf=AE['ngf'], n_downsampling=AE['n_downsampling'], num_res_blocks=AE['num_res_blocks'],
                        norm_layer=nn.BatchNorm2d, norm_layer1d=nn.BatchNorm1d, learn_3d=AE['learn_3d'])
    dec = ResnetDecoder(img_channels, ngf=AE['ngf'], n_downsampling=AE['n_downsampling'], out_layer=AE['out_layer'],
                        norm_layer=nn.BatchNorm2d)
    return enc.train(), dec.train()


def _bn(bn, x, act, residual=None):
    """BatchNorm2d (+ ReLU) (+ residual) with nn.BatchNorm2d's own mode logic (ref: torch.nn.modules.batchnorm._BatchNorm.forward).
    A dp.SyncBatchNorm2d in training mode under data parallelism takes its statistics over every rank (Lightning's
    sync_batchnorm=True, ref/train_AutoEncoder_lightning.py:40-42); a plain BatchNorm2d keeps this rank's own, as torch does.
    A BatchNorm1d of a learn_3d block (and its dp.SyncBatchNorm1d twin) takes the same call on the (N*T, C, H, W) frames with its own
    parameters and buffers: over (N*H*W, C, T) it has the per-channel statistics, and the count of the unbiased running variance,
    that BatchNorm2d has over those frames."""
    if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    train = bn.training or bn.running_mean is None
    w = bn.weight if bn.weight is not None else torch.ones(bn.num_features, device=x.device)
    b = bn.bias if bn.bias is not None else torch.zeros(bn.num_features, device=x.device)
    group = dp.syncbn_group() if isinstance(bn, (dp.SyncBatchNorm2d, dp.SyncBatchNorm1d)) and bn.training and dp.active() else None
    return ops.bn_act_train(x, w, b, bn.running_mean, bn.running_var, bn.momentum, bn.eps, act, train, residual, group=group)


def _pad_size(m):
    p = m.padding
    if len(set(p)) != 1:
        raise NotImplementedError("ReflectionPad2d with unequal sides")
    return p[0]


def _run_seq(seq, x, residual=None):
    """Sequential of [ReflectionPad2d] conv [BatchNorm2d] [ReLU] groups (and a final Tanh / Sigmoid); `residual` is added to the
    output of the last module (fused into its BatchNorm pass when it ends in one)"""
    mods, i = list(seq), 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.ReflectionPad2d):
            x = ops.reflect_pad(x, _pad_size(m)); i += 1
        elif isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            x = m(x); i += 1
        elif isinstance(m, nn.BatchNorm2d):
            act = 1 if i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU) else 0
            last = i + 1 + act == len(mods)
            x = _bn(m, x, act, residual if last else None)
            if last:
                residual = None
            i += 1 + act
        elif isinstance(m, nn.ReLU):
            x = torch.relu(x); i += 1
        elif isinstance(m, (nn.Tanh, nn.Sigmoid, nn.Dropout)):
            x = m(x); i += 1
        else:
            raise NotImplementedError(f"trainable autoencoder: {type(m).__name__} is not on the shipped configs' path")
    return x if residual is None else x + residual


def _attn_core(a, x, core):
    """the shared frame of both attentions on the (N', C, H, W) frames x: [Wq | Wk | Wv] GEMM -> core(qkv) -> out_proj -> norm -> ReLU ->
    x + gamma * h"""
    N, C, H, W = x.shape
    A, V = a.attn_dim, a.value_dim
    tok = x.permute(0, 2, 3, 1).reshape(N * H * W, C)               # a view when x is channels_last
    ws = [a.Wq.weight, a.Wk.weight, a.Wv.weight]
    bs = [a.Wq.bias, a.Wk.bias, a.Wv.bias] if a.bias else None
    width = 2 * A + V
    pad = -width % 32                                                # the GEMM's dgrad wants an inner dimension % 32 == 0
    if pad:
        ws = ws + [torch.zeros(pad, C, device=x.device)]
        if bs is not None:
            bs = bs + [torch.zeros(pad, device=x.device)]
    # the GEMM's weight gradient sums over the token rows and wants their count % 32 == 0 (every config grid has it; 4 frames of a
    # 6x10 or 3x5 grid have not): zero rows are appended to the two projections' inputs and cut from their outputs - they add
    # exact zeros to dW, and the cut hands zero gradient rows back, so db is untouched too
    R = N * H * W
    rpad = -R % 32
    if rpad:
        tok = nn.functional.pad(tok, (0, 0, 0, rpad))
    qkv = ops.linear(tok, torch.cat(ws, 0), torch.cat(bs, 0) if bs is not None else None)
    if rpad:
        qkv = qkv[:R]
    o = core(qkv, A, V)
    if rpad:
        o = nn.functional.pad(o, (0, 0, 0, rpad))
    out = ops.linear(o, a.out_proj.weight, a.out_proj.bias)
    if rpad:
        out = out[:R]
    out = out.view(N, H, W, C).permute(0, 3, 1, 2)
    relu = isinstance(a.activ_func, nn.ReLU)
    if isinstance(a.norm_func, (nn.BatchNorm2d, nn.BatchNorm1d)):
        h = _bn(a.norm_func, out, 1 if relu else 0)
        if not relu:
            h = a.activ_func(h)
    else:
        h = a.activ_func(a.norm_func(out))
    return x + a.gamma * h


def _attn(a, x):
    """NonLocalAttenion2D.forward (ref/models/submodules.py:150-176) on the HIP path; ops.nonlocal_attn_any_packed chooses between the
    configs' exact-tile kernels and the any-grid ones"""
    N, C, H, W = x.shape
    return _attn_core(a, x, lambda qkv, A, V: ops.nonlocal_attn_any_packed(qkv, N, H, W, A, V))


def _attn1d(a, x, T):
    """NonLocalAttenion1D.forward (ref/models/submodules.py:221-243) on the HIP path, on the frames x (N*T, C, H, W) themselves: the
    token rows are those of the 2-D attention, a pixel's T frames lie H*W rows apart.  Clips of more than ops.TEMPORAL_ATTN_MAX_T
    frames take the key-tiled kernels (ops.temporal_attn_long_packed), every other clip ops.temporal_attn_packed as before"""
    NT, C, H, W = x.shape
    return _attn_core(a, x, lambda qkv, A, V: ops.temporal_attn_any_packed(qkv, NT // T, T, H * W, A, V))


def _temporal_conv(m, x, T):
    """temporal_conv(y) + y of ref/models/submodules.py:64, :89 on the frames x (N*T, C, H, W): Conv1d(k=3, 'same') over the T frames of a
    pixel is conv2d with the weight viewed as [C, C, 3, 1] and padding (1, 0) on the (N, C, T, H*W) view (zero padding per clip by
    construction; the gradients reach the Conv1d's parameters through the view); BatchNorm1d + ReLU + skip in one pass"""
    conv, bn = m.temporal_conv[0], m.temporal_conv[1]
    if not (isinstance(bn, nn.BatchNorm1d) and isinstance(m.temporal_conv[2], nn.ReLU)):
        raise NotImplementedError("trainable autoencoder: temporal_conv must be Conv1d, BatchNorm1d, ReLU")
    y = nn.functional.conv2d(_temporal_view(x, T), conv.weight.unsqueeze(-1), conv.bias, 1, (1, 0))
    return _bn(bn, _temporal_view_back(y, x.shape), 1, residual=x)


def _fact(m, x, T):
    """Factorized3DConvAttn.forward (ref/models/submodules.py:48-95), both orders, with and without the temporal half"""
    if m.conv_first:
        y = _attn(m.attn2d, _run_seq(m.spatial_conv, x, residual=x))
        if m.learn_3d:
            y = _attn1d(m.attn1d, _temporal_conv(m, y, T), T)
        return y + x
    y = _attn(m.attn2d, x)
    y = _run_seq(m.spatial_conv, y, residual=y)
    if m.learn_3d:
        y = _temporal_conv(m, _attn1d(m.attn1d, y, T), T)
    return y + x


def _encoder_forward(enc, x):
    N, T = x.shape[:2]
    x = x.flatten(0, 1)
    if getattr(enc, "_npvp_channels_last", False):
        x = x.contiguous(memory_format=torch.channels_last)
    x = _run_seq(enc.block1, _run_seq(enc.block0, x))
    for i in range(1, enc.n_downsampling):
        x = _run_seq(getattr(enc, f'block{i + 1}_conv'), _fact(getattr(enc, f'block{i + 1}_3dConvAttn'), x, T))
    for i in range(enc.num_res_blocks):
        rb = getattr(enc, f'res_conv_{i}')
        x = _fact(getattr(enc, f'res_3dConvAttn_{i}'), x, T)
        x = _run_seq(rb.conv_block, x, residual=x)
    x = torch.relu(x)
    return x.reshape(N, T, *x.shape[1:])


def _decoder_forward(dec, x):
    N, T = x.shape[:2]
    x = x.flatten(0, 1)
    if not x.is_contiguous():
        x = x.contiguous()
    y = _run_seq(dec.model, x)
    return y.reshape(N, T, *y.shape[1:])


def prepare_trainable_autoencoder(enc, dec, channels_last=True):
    """Route the pair's forward through the HIP training ops (in place, on these two instances); state-dict keys are unchanged.
    Train mode: batch statistics (running statistics updated; over all ranks for layers converted by dp.convert_sync_batchnorm /
    ae_data_parallel); eval mode: running statistics.  channels_last: the encoder's
    activations run in torch.channels_last memory (BatchNorm layout 0; the attention's token matrix is then a view), the decoder's
    stay NCHW (layout 1), as in the frozen path (to_device_layout).  Returns (enc, dec)."""
    if not isinstance(enc, ResnetEncoder) or not isinstance(dec, ResnetDecoder):
        raise TypeError("prepare_trainable_autoencoder: (ResnetEncoder, ResnetDecoder) expected")
    for m in list(enc.modules()) + list(dec.modules()):
        if isinstance(m, Factorized3DConvAttn) and not isinstance(m.spatial_conv, nn.Sequential):
            raise RuntimeError("prepare_trainable_autoencoder: this pair has been fused for the frozen Stage-2 path")
        if isinstance(m, nn.BatchNorm2d) and m.momentum is None:
            raise NotImplementedError("prepare_trainable_autoencoder: BatchNorm2d(momentum=None) is not supported")
        if isinstance(m, nn.BatchNorm1d) and m.momentum is None:
            raise NotImplementedError("prepare_trainable_autoencoder: BatchNorm1d(momentum=None) is not supported")
        if isinstance(m, Factorized3DConvAttn) and m.learn_3d and not ops.nonlocal_attn_dims(m.attn1d.attn_dim, m.attn1d.value_dim):
            raise NotImplementedError(f"prepare_trainable_autoencoder: attn1d's (attn dim, value dim) = ({m.attn1d.attn_dim}, "
                                      f"{m.attn1d.value_dim}) is not one of {ops.temporal_attn_dims()}")
    enc.forward = types.MethodType(_encoder_forward, enc)
    dec.forward = types.MethodType(_decoder_forward, dec)
    enc._npvp_trainable = dec._npvp_trainable = True
    enc._npvp_channels_last = bool(channels_last)
    return enc, dec
