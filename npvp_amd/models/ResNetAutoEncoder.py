"""Frozen Stage-1 autoencoder around the predictor (ref/models/ResNetAutoEncoder.py:51-261 and the
`Factorized3DConvAttn` / `NonLocalAttenion2D` blocks of ref/models/submodules.py:9-180), needed for the
FULL training step of Stage 2: frozen encoder on past+future frames (no grad), frozen decoder on the
predicted features with the gradient flowing through it to the predictor (ref/models/Predictor.py:172-194).

SURVEY 8f "next" row #1.  Same class names, constructor signatures and state-dict keys as the reference, so Stage-1
checkpoints load.  `learn_3d=True` adds the temporal half of every Factorized3DConvAttn block (Conv1d over the T frames of a pixel
+ NonLocalAttenion1D, ref/models/submodules.py:30-38, 62-66, 86-91, 182-255).
  stage 1: the modules as built run on stock PyTorch-ROCm (MIOpen convolutions, rocBLAS matmuls);
  stage 2: `to_device_layout` -> `fuse_frozen_autoencoder`: the pair is frozen and in eval mode in Stage 2, so every
           conv -> BatchNorm -> ReLU (-> + skip) group becomes a `FoldedConvAct`: the convolution with the BatchNorm folded
           into its weights (MIOpen) + ONE hand-written epilogue pass `npvp_bias_act` (csrc/ae.hip) instead of separate
           bias / BatchNorm / ReLU / skip-add passes; the decoder's input gradient goes through `npvp_act_bwd`.
           `attn2d="hip"` (opt-in, inference only) also sends the encoder's NonLocalAttenion2D through the non-local attention
           kernels and one `npvp_bias_act_scaled` pass (`_fused_attn2d`); the default `"stock"` leaves it on stock PyTorch.
           `conv3x3="hip"` (opt-in, inference only) sends the encoder's 3 x 3 stride-1 convolutions with 64-multiple channels
           (every spatial_conv, both convolutions of every ResnetBlock) through ONE f16x3 implicit-GEMM launch each
           (`ops.conv3x3_packed`, csrc/conv3x3.hip: padding as index math, bias + activation + skip in its epilogue); the default
           `"stock"` leaves them on MIOpen + `npvp_bias_act`.
           `down3x3="hip"` (opt-in, inference only, independent of the other two switches) sends the encoder's 3 x 3 stride-2
           downsampling convolutions (`block1`, every `block{i}_conv`; C_in a multiple of 32, C_out of 64) through the stride-2 form
           of the same kernel (`ops.conv3x3s2_packed`); their output carries its amax slot, so the routed `spatial_conv` behind it
           runs no `npvp_amax` pass.  The default `"stock"` leaves them on MIOpen + `npvp_bias_act`.
           `up3x3="hip"` (opt-in, independent of the other three switches, DIFFERENTIABLE w.r.t. its input: the decoder sits inside
           autograd in Stage 2) sends the decoder's ConvTranspose2d(3, stride 2, padding 1, output_padding 1) groups with 64-multiple
           channels through the transposed form of the same kernel (`ops.convt3x3s2_packed`: one launch per convolution, 9 taps per
           4 outputs; its input gradient is the stride-2 kernel of `down3x3`).  The routed decoder copies its NCHW input frames to
           channels-last once, and copies back to NCHW once in front of its stock remainder (`UP3X3_TAIL`).
           `tail7x7="hip"` (opt-in, independent of the other four switches, differentiable w.r.t. its input) sends the decoder's tail -
           ReflectionPad2d(3), Conv2d(ngf, output_nc, 7), Tanh / Sigmoid - through `ops.tail7x7_packed` (csrc/conv7x7.hip: one launch,
           padding as index math, bias and activation in the epilogue, channels-last frames in, NCHW frames out; the input gradient is
           act_bwd, amax and one launch).  Behind `up3x3="hip"` no copy back to NCHW remains.
           `stem7x7="hip"` (opt-in, inference only, independent of the other five switches) sends the encoder's stem `block0` -
           ReflectionPad2d(3), Conv2d(input_nc, ngf, 7), BatchNorm (folded), ReLU - through `ops.stem7x7_packed` (csrc/conv7x7.hip: one
           launch, planar NCHW frames in, channels-last frames out with their amax slot, so a routed `block1` runs no `npvp_amax` pass).
           With it every convolution of an ngf = 64, `learn_3d=False` pair has a hand-written route.
"""
import functools
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


_ACT_CODE = {nn.ReLU: 1, nn.Tanh: 2, nn.Sigmoid: 3}


def _bn_scale_shift(bn):
    s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    return s, bn.bias - bn.running_mean * s


class FoldedConvAct(nn.Module):
    """[pad ->] conv / transposed conv [-> BatchNorm2d (eval)] [-> ReLU / Tanh / Sigmoid] of a FROZEN network as one convolution
    with folded weights (MIOpen, no bias) and one epilogue pass out = act(conv + bias[c]) (+ residual)  (csrc/ae.hip)."""

    def __init__(self, conv, bn=None, act=None, pad=None):
        super().__init__()
        assert isinstance(conv, (nn.Conv2d, nn.ConvTranspose2d)) and conv.groups == 1
        self.transposed = isinstance(conv, nn.ConvTranspose2d)
        w = conv.weight.detach()
        b = conv.bias.detach() if conv.bias is not None else torch.zeros(conv.out_channels, dtype=w.dtype, device=w.device)
        if bn is not None:
            assert isinstance(bn, nn.BatchNorm2d) and not bn.training and bn.track_running_stats, "fold needs an eval-mode BatchNorm2d"
            s, t = _bn_scale_shift(bn)
            w = w * (s.view(1, -1, 1, 1) if self.transposed else s.view(-1, 1, 1, 1))
            b = b * s + t
        fmt = torch.channels_last if conv.weight.is_contiguous(memory_format=torch.channels_last) and not conv.weight.is_contiguous() \
            else torch.contiguous_format
        self.register_buffer("weight", w.contiguous(memory_format=fmt))
        self.register_buffer("bias", b.detach().float().contiguous())
        self.stride, self.padding, self.dilation = conv.stride, conv.padding, conv.dilation
        self.output_padding = conv.output_padding if self.transposed else None
        self.act = 0 if act is None else _ACT_CODE[type(act)]
        self.pad = pad
        self.conv3x3_pad = None          # "zero" / "reflect" once routed to the 3 x 3 kernel (fuse_frozen_autoencoder(conv3x3="hip"))
        self.down3x3 = False             # True once routed to its stride-2 form (fuse_frozen_autoencoder(down3x3="hip"))
        self.up3x3 = False               # True once routed to its transposed form (fuse_frozen_autoencoder(up3x3="hip"))
        self.tail7x7 = False             # True once routed to the 7 x 7 tail kernels (fuse_frozen_autoencoder(tail7x7="hip"))
        self.stem7x7 = False             # True once routed to the 7 x 7 stem kernel (fuse_frozen_autoencoder(stem7x7="hip"))

    def route_conv3x3(self, pad):
        """send this convolution through ops.conv3x3_packed with the padding rule `pad`; the weight planes and the weight's amax slot
        are non-persistent buffers (the state-dict keys do not change), built here when the weight is on the device and at the first
        routed forward otherwise"""
        self.conv3x3_pad = pad
        planes, w_amax = ops.conv3x3_planes(self.weight) if self.weight.is_cuda else (None, None)
        self.register_buffer("_npvp_planes", planes, persistent=False)
        self.register_buffer("_npvp_w_amax", w_amax, persistent=False)

    def _conv3x3(self, x, residual):
        if torch.is_grad_enabled() and (x.requires_grad or (residual is not None and residual.requires_grad)):
            raise NotImplementedError('conv3x3="hip" (to_device_layout / fuse_frozen_autoencoder) is inference-only: the input of this '
                                      'convolution requires grad; fuse the pair with conv3x3="stock" to differentiate through it')
        if self._npvp_planes is None or self._npvp_planes.device != x.device:
            self._npvp_planes, self._npvp_w_amax = ops.conv3x3_planes(self.weight.to(x.device))
        return ops.conv3x3_packed(x, self._npvp_planes, self._npvp_w_amax, self.bias, self.conv3x3_pad, self.act, residual)

    def route_down3x3(self):
        """send this stride-2 convolution through ops.conv3x3s2_packed; planes and amax slot as route_conv3x3 keeps them"""
        self.down3x3 = True
        planes, w_amax = ops.conv3x3s2_planes(self.weight) if self.weight.is_cuda else (None, None)
        self.register_buffer("_npvp_planes", planes, persistent=False)
        self.register_buffer("_npvp_w_amax", w_amax, persistent=False)

    def _down3x3(self, x, residual):
        if torch.is_grad_enabled() and (x.requires_grad or (residual is not None and residual.requires_grad)):
            raise NotImplementedError('down3x3="hip" (to_device_layout / fuse_frozen_autoencoder) is inference-only: the input of this '
                                      'convolution requires grad; fuse the pair with down3x3="stock" to differentiate through it')
        if self._npvp_planes is None or self._npvp_planes.device != x.device:
            self._npvp_planes, self._npvp_w_amax = ops.conv3x3s2_planes(self.weight.to(x.device))
        return ops.conv3x3s2_packed(x, self._npvp_planes, self._npvp_w_amax, self.bias, self.act, residual)

    _UP3X3_BUFFERS = ("_npvp_planes", "_npvp_w_amax", "_npvp_bwd_planes", "_npvp_bwd_w_amax", "_npvp_zero_bias")

    def route_up3x3(self):
        """send this transposed convolution through ops.convt3x3s2_packed (differentiable w.r.t. its input); the forward planes, the
        input gradient's planes, their amax slots and the gradient launch's zero bias are non-persistent buffers, built as
        route_conv3x3 builds its own"""
        self.up3x3 = True
        planes = ops.convt3x3s2_planes(self.weight) if self.weight.is_cuda else (None,) * len(self._UP3X3_BUFFERS)
        for name, t in zip(self._UP3X3_BUFFERS, planes):
            self.register_buffer(name, t, persistent=False)

    def _up3x3(self, x):
        if self._npvp_planes is None or self._npvp_planes.device != x.device:
            for name, t in zip(self._UP3X3_BUFFERS, ops.convt3x3s2_planes(self.weight.to(x.device))):
                setattr(self, name, t)
        planes = ops.ConvT3x3Planes(*(getattr(self, name) for name in self._UP3X3_BUFFERS))
        return ops.convt3x3s2_packed(x, planes, self.bias, self.act)

    _TAIL7X7_BUFFERS = ("_npvp_planes", "_npvp_w_amax", "_npvp_bwd_planes")

    def route_tail7x7(self):
        """send this ReflectionPad2d(3) -> 7 x 7 convolution -> activation through ops.tail7x7_packed (differentiable w.r.t. its input,
        NCHW out); the forward planes, the weight's amax slot and the input gradient's planes are non-persistent buffers, built as
        route_up3x3 builds its own"""
        self.tail7x7 = True
        planes = ops.tail7x7_planes(self.weight) if self.weight.is_cuda else (None,) * len(self._TAIL7X7_BUFFERS)
        for name, t in zip(self._TAIL7X7_BUFFERS, planes):
            self.register_buffer(name, t, persistent=False)

    def _tail7x7(self, x):
        if self._npvp_planes is None or self._npvp_planes.device != x.device:
            for name, t in zip(self._TAIL7X7_BUFFERS, ops.tail7x7_planes(self.weight.to(x.device))):
                setattr(self, name, t)
        planes = ops.Tail7x7Planes(*(getattr(self, name) for name in self._TAIL7X7_BUFFERS))
        return ops.tail7x7_packed(x, planes, self.bias, self.act)

    def route_stem7x7(self):
        """send this ReflectionPad2d(3) -> 7 x 7 convolution -> activation through ops.stem7x7_packed (inference only; planar frames in,
        channels-last frames out); planes and amax slot as route_conv3x3 keeps them"""
        self.stem7x7 = True
        planes, w_amax = ops.stem7x7_planes(self.weight) if self.weight.is_cuda else (None, None)
        self.register_buffer("_npvp_planes", planes, persistent=False)
        self.register_buffer("_npvp_w_amax", w_amax, persistent=False)

    def _stem7x7(self, x):
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError('stem7x7="hip" (to_device_layout / fuse_frozen_autoencoder) is inference-only: the input of this '
                                      'convolution requires grad; fuse the pair with stem7x7="stock" to differentiate through it')
        if self._npvp_planes is None or self._npvp_planes.device != x.device:
            self._npvp_planes, self._npvp_w_amax = ops.stem7x7_planes(self.weight.to(x.device))
        return ops.stem7x7_packed(x, self._npvp_planes, self._npvp_w_amax, self.bias, self.act)

    def forward(self, x, residual=None):
        # the routed stem: planar (contiguous NCHW) frames of at least 4 x 4 pixels only - what ops.stem7x7_packed accepts
        if self.stem7x7 and residual is None and x.dim() == 4 and x.is_contiguous() and x.shape[2] >= 4 and x.shape[3] >= 4:
            return self._stem7x7(x)
        # routed: channels-last frames only (anything else keeps the stock forward below: no silent copy)
        if self.tail7x7 and residual is None and _channels_last_only(x):
            return self._tail7x7(x)
        if self.up3x3 and residual is None and _channels_last_only(x):
            return self._up3x3(x)
        if self.conv3x3_pad is not None and _channels_last_only(x) and (residual is None or _channels_last_only(residual)):
            return self._conv3x3(x, residual)
        if self.down3x3 and _channels_last_only(x) and (residual is None or _channels_last_only(residual)):
            return self._down3x3(x, residual)
        if self.pad is not None:
            x = self.pad(x)
        if self.transposed:
            y = F.conv_transpose2d(x, self.weight, None, self.stride, self.padding, self.output_padding, 1, self.dilation)
        else:
            y = F.conv2d(x, self.weight, None, self.stride, self.padding, self.dilation, 1)
        return ops.bias_act(y, self.bias, self.act, residual)


def _channels_last_only(x):
    return x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()


def _fold_sequential(seq):
    """Sequential of [pad] conv [BatchNorm2d] [activation] groups -> Sequential of FoldedConvAct"""
    out, mods, i = [], list(seq), 0
    while i < len(mods):
        pad = None
        if isinstance(mods[i], (nn.ReflectionPad2d, nn.ReplicationPad2d)):
            pad = mods[i]; i += 1
        conv = mods[i]; i += 1
        assert isinstance(conv, (nn.Conv2d, nn.ConvTranspose2d)), f"cannot fold {type(conv).__name__}"
        bn = act = None
        if i < len(mods) and isinstance(mods[i], nn.BatchNorm2d):
            bn = mods[i]; i += 1
        if i < len(mods) and type(mods[i]) in _ACT_CODE:
            act = mods[i]; i += 1
        out.append(FoldedConvAct(conv, bn, act, pad))
    return nn.Sequential(*out)


ATTN2D_ROUTES = ("stock", "hip")


def _check_attn2d(attn2d):
    if attn2d not in ATTN2D_ROUTES:
        raise ValueError(f"attn2d={attn2d!r}: the route of the frozen encoder's NonLocalAttenion2D is one of {ATTN2D_ROUTES}")


CONV3X3_ROUTES = ("stock", "hip")


def _check_conv3x3(conv3x3):
    if conv3x3 not in CONV3X3_ROUTES:
        raise ValueError(f"conv3x3={conv3x3!r}: the route of the frozen encoder's 3 x 3 convolutions is one of {CONV3X3_ROUTES}")


def _conv3x3_takes_hip(m):
    """the padding rule ("zero" / "reflect") under which the 3 x 3 kernel runs this FoldedConvAct, or None: a 3 x 3, stride-1,
    undilated, not transposed convolution with 64-multiple channel counts, zero-padded by 1 or behind a ReflectionPad2d(1)"""
    if m.transposed or tuple(m.weight.shape[2:]) != (3, 3) or tuple(m.stride) != (1, 1) or tuple(m.dilation) != (1, 1):
        return None
    # every 64-multiple channel count stays on the kernel: at C = 64, 128, 256 and 512 (the encoders' four (C, grid) pairs, zero and
    # reflection padding) both hip timings beat both MIOpen + npvp_bias_act timings (profiles/frozen_conv3x3_bench.txt); a channel
    # count that loses there would be named and excluded here
    if not ops.conv3x3_takes(m.weight.shape[1], m.weight.shape[0]):
        return None
    if m.pad is None:
        return "zero" if tuple(m.padding) == (1, 1) else None
    if type(m.pad) is nn.ReflectionPad2d and tuple(m.pad.padding) == (1, 1, 1, 1) and tuple(m.padding) == (0, 0):
        return "reflect"
    return None


def _route_conv3x3(folded):
    for m in folded:
        pad = _conv3x3_takes_hip(m)
        if pad is not None:
            m.route_conv3x3(pad)


DOWN3X3_ROUTES = ("stock", "hip")


def _check_down3x3(down3x3):
    if down3x3 not in DOWN3X3_ROUTES:
        raise ValueError(f"down3x3={down3x3!r}: the route of the frozen encoder's stride-2 3 x 3 convolutions is one of {DOWN3X3_ROUTES}")


def _down3x3_takes_hip(m):
    """whether the stride-2 form of the 3 x 3 kernel runs this FoldedConvAct: a 3 x 3, stride-(2, 2), undilated, not transposed
    convolution, zero-padded by 1 with no pad module, C_in a multiple of 32 and C_out of 64"""
    if m.transposed or tuple(m.weight.shape[2:]) != (3, 3) or tuple(m.stride) != (2, 2) or tuple(m.dilation) != (1, 1):
        return False
    if m.pad is not None or tuple(m.padding) != (1, 1):
        return False
    # every (C_in, C_out) of the rule stays on the kernel: at the seven (C_in -> C_out, grid) pairs of the c1- and c4-size encoders
    # (64 -> 128 at 64 x 64 ... 256 -> 512 at 16 x 16; 32 -> 64 at 128 x 128 ... 256 -> 512 at 16 x 16) both hip timings, each with its
    # npvp_amax pass over the input, beat both MIOpen + npvp_bias_act timings (the "conv" lines of profiles/frozen_down3x3_bench.txt);
    # a pair that loses there would be named and excluded here
    return ops.conv3x3s2_takes(m.weight.shape[1], m.weight.shape[0])


def _route_down3x3(folded):
    for m in folded:
        if _down3x3_takes_hip(m):
            m.route_down3x3()


UP3X3_ROUTES = ("stock", "hip")
# where the stock remainder of a routed decoder runs (the 7 x 7 tail, and in front of it the 64 -> 32 transposed convolution of an
# ngf = 32 decoder): on the channels-last tensor the routed convolutions hand over ("nhwc"), or with NCHW weights behind one copy back to
# NCHW ("nchw"); whichever measured faster for decoder forward + input gradient (profiles/frozen_up3x3_bench.txt).  Read at fuse time.
# It decides for a STOCK tail: where tail7x7="hip" routes the tail, which reads channels-last frames, whatever stays stock in front of
# it keeps its channels-last weights and no copy back to NCHW is made.
UP3X3_TAIL = "nchw"


def _check_up3x3(up3x3):
    if up3x3 not in UP3X3_ROUTES:
        raise ValueError(f"up3x3={up3x3!r}: the route of the frozen decoder's transposed 3 x 3 convolutions is one of {UP3X3_ROUTES}")


def _up3x3_takes_hip(m):
    """whether the transposed form of the 3 x 3 kernel runs this FoldedConvAct: a transposed 3 x 3 convolution, stride (2, 2), padding
    (1, 1), output_padding (1, 1), undilated, no pad module, C_in and C_out multiples of 64 (the forward needs C_out, its input
    gradient - the stride-2 kernel with the channels exchanged - C_in)"""
    if not m.transposed or tuple(m.weight.shape[2:]) != (3, 3) or tuple(m.stride) != (2, 2) or tuple(m.dilation) != (1, 1):
        return False
    if m.pad is not None or tuple(m.padding) != (1, 1) or tuple(m.output_padding) != (1, 1):
        return False
    # every (C_in, C_out) of the rule stays on the kernel: at the three (C_in -> C_out, grid) pairs of the decoders - 512 -> 256 at 8 x 8,
    # 256 -> 128 at 16 x 16, 128 -> 64 at 32 x 32, at 320, 1792 and 128 frames - both hip timings beat both MIOpen + npvp_bias_act timings,
    # forward and forward + input gradient, each hip call with an npvp_amax pass over its input (the "conv" lines of
    # profiles/frozen_up3x3_bench.txt); a pair that loses there would be named and excluded here
    return ops.convt3x3s2_takes(m.weight.shape[0], m.weight.shape[1])


def _route_up3x3(folded):
    for m in folded:
        if _up3x3_takes_hip(m):
            m.route_up3x3()


TAIL7X7_ROUTES = ("stock", "hip")


def _check_tail7x7(tail7x7):
    if tail7x7 not in TAIL7X7_ROUTES:
        raise ValueError(f"tail7x7={tail7x7!r}: the route of the frozen decoder's 7 x 7 output convolution is one of {TAIL7X7_ROUTES}")


def _tail7x7_takes_hip(m):
    """whether the 7 x 7 tail kernels run this FoldedConvAct: a 7 x 7, stride-1, undilated, not transposed convolution with conv padding
    0 behind ReflectionPad2d(3), C_in a multiple of 32, 1 <= C_out <= 4, activation none, Tanh or Sigmoid.  (The encoder's 7 x 7 stem
    has C_in = 1 or 3 and wide C_out: another kernel, `_stem7x7_takes_hip`.)"""
    if m.transposed or tuple(m.weight.shape[2:]) != (7, 7) or tuple(m.stride) != (1, 1) or tuple(m.dilation) != (1, 1):
        return False
    if type(m.pad) is not nn.ReflectionPad2d or tuple(m.pad.padding) != (3, 3, 3, 3) or tuple(m.padding) != (0, 0):
        return False
    if m.act not in ops.TAIL7X7_ACTS:
        return False
    # every (C_in, size) pair of the rule stays on the kernels: C_in = 64 at 64 x 64 x 1 and 64 x 64 x 3 frames, C_in = 32 at
    # 128 x 128 x 3 - the "tail" lines of profiles/frozen_tail7x7_bench.txt; a pair that loses there would be named and excluded here
    return ops.tail7x7_takes(m.weight.shape[1], m.weight.shape[0])


def _route_tail7x7(folded):
    for m in folded:
        if _tail7x7_takes_hip(m):
            m.route_tail7x7()


STEM7X7_ROUTES = ("stock", "hip")


def _check_stem7x7(stem7x7):
    if stem7x7 not in STEM7X7_ROUTES:
        raise ValueError(f"stem7x7={stem7x7!r}: the route of the frozen encoder's 7 x 7 input convolution is one of {STEM7X7_ROUTES}")


def _stem7x7_takes_hip(m):
    """whether the 7 x 7 stem kernel runs this FoldedConvAct: a 7 x 7, stride-1, undilated, not transposed convolution with conv padding
    0 behind ReflectionPad2d(3), 1 <= C_in <= 4, C_out a multiple of 32, activation none or ReLU.  (The decoder's 7 x 7 tail has wide
    C_in and C_out <= 4: `_tail7x7_takes_hip`.)"""
    if m.transposed or tuple(m.weight.shape[2:]) != (7, 7) or tuple(m.stride) != (1, 1) or tuple(m.dilation) != (1, 1):
        return False
    if type(m.pad) is not nn.ReflectionPad2d or tuple(m.pad.padding) != (3, 3, 3, 3) or tuple(m.padding) != (0, 0):
        return False
    if m.act not in ops.STEM7X7_ACTS:
        return False
    # every (C_in -> C_out, size) of the rule stays on the kernel: 1 -> 64 at 640 frames of 64 x 64, 3 -> 64 at 1920 frames of 64 x 64 and
    # 3 -> 32 at 160 frames of 128 x 128 - both hip timings, each with its npvp_amax pass over the frames, beat both padded copy + MIOpen +
    # npvp_bias_act timings (the "stem" lines of profiles/frozen_stem7x7_bench.txt); a pair that loses there would be named and excluded here
    return ops.stem7x7_takes(m.weight.shape[1], m.weight.shape[0])


def _route_stem7x7(folded):
    for m in folded:
        if _stem7x7_takes_hip(m):
            m.route_stem7x7()


def _zero_or_bias(lin):
    return lin.bias if lin.bias is not None else torch.zeros(lin.out_features, dtype=lin.weight.dtype, device=lin.weight.device)


def _register_wqkv(a):
    """[Wq | Wk | Wv] of an attention as one projection (non-persistent buffers: the state-dict keys stay the reference's)"""
    a.register_buffer("_npvp_wqkv", torch.cat([a.Wq.weight, a.Wk.weight, a.Wv.weight], 0).detach().clone(), persistent=False)
    a.register_buffer("_npvp_bqkv", torch.cat([_zero_or_bias(a.Wq), _zero_or_bias(a.Wk), _zero_or_bias(a.Wv)], 0).detach().clone(),
                      persistent=False)


def _attn2d_takes_hip(a):
    """a NonLocalAttenion2D of a fused pair (BatchNorm already folded into out_proj) that the HIP route can run: an (A, V) the
    non-local kernels are instantiated for, an activation the epilogue has, gamma a Parameter or the float 1.0"""
    gamma_ok = isinstance(a.gamma, torch.Tensor) or a.gamma == 1.0
    act_ok = isinstance(a.activ_func, nn.Identity) or type(a.activ_func) in _ACT_CODE
    return (ops.nonlocal_attn_dims(a.attn_dim, a.value_dim) and isinstance(a.norm_func, nn.Identity) and act_ok and gamma_ok
            and a.out_proj.bias is not None)


def fuse_frozen_autoencoder(enc, dec, attn2d="stock", conv3x3="stock", down3x3="stock", up3x3="stock", tail7x7="stock",
                            stem7x7="stock"):
    """In-place module surgery on an eval-mode pair that already holds its final weights; freezes its parameters (do it after load_state_dict:
    the folded modules no longer carry the reference's state-dict keys).  Returns (enc, dec).
    attn2d: "stock" (default) leaves every NonLocalAttenion2D of the encoder on its own forward (PyTorch: the (frames, H*W, H*W/4) scores
    in memory); "hip" sends those whose (attn_dim, value_dim) has non-local kernels (ops.nonlocal_attn_dims) through `_fused_attn2d`
    (inference only: no scores in memory, one epilogue pass).  Any other value is refused.
    conv3x3: "stock" (default) leaves every convolution on MIOpen + npvp_bias_act; "hip" sends the ENCODER's FoldedConvActs that
    `_conv3x3_takes_hip` accepts - every spatial_conv and ResnetBlock convolution with 64-multiple channels - through
    ops.conv3x3_packed (inference only).  The 7 x 7 and stride-2 convolutions, ReplicationPad2d blocks and the decoder stay stock.
    Any other value is refused.
    down3x3: "stock" (default) leaves the stride-2 convolutions on MIOpen + npvp_bias_act; "hip" sends the ENCODER's FoldedConvActs
    that `_down3x3_takes_hip` accepts - block1 and every block{i}_conv - through ops.conv3x3s2_packed (inference only).  The decoder's
    transposed convolutions stay stock.  Any other value is refused.
    up3x3: "stock" (default) leaves the DECODER's transposed convolutions on MIOpen + npvp_bias_act; "hip" sends those
    `_up3x3_takes_hip` accepts - ConvTranspose2d(3, stride 2, padding 1, output_padding 1) with 64-multiple channels: all of an
    ngf = 64 decoder, all but the last (64 -> 32) of an ngf = 32 one - through ops.convt3x3s2_packed, which is differentiable w.r.t.
    its input (the decoder sits inside autograd in Stage 2), and makes the decoder convert its input frames to channels-last at its
    entry.  The 7 x 7 tail stays stock, with NCHW weights behind one copy back to NCHW (`UP3X3_TAIL`).  Any other value is refused.
    tail7x7: "stock" (default) leaves the decoder's tail - ReflectionPad2d(3), Conv2d(ngf, output_nc, 7), Tanh / Sigmoid - on a padded
    copy, MIOpen and npvp_bias_act; "hip" sends the FoldedConvAct of the DECODER that `_tail7x7_takes_hip` accepts through
    ops.tail7x7_packed (one launch, padding as index math, bias and activation in the epilogue, NCHW out; differentiable w.r.t. its
    input: act_bwd, amax, one input-gradient launch).  The routed tail reads channels-last frames: behind up3x3="hip" it takes them as
    they come (and whatever stays stock between the routed convolutions keeps its channels-last weights: no copy back to NCHW), behind
    up3x3="stock" the decoder makes one explicit copy to channels-last in front of it.  Any other value is refused.
    stem7x7: "stock" (default) leaves the encoder's stem - block0: ReflectionPad2d(3), Conv2d(input_nc, ngf, 7), BatchNorm, ReLU - on a
    padded copy, MIOpen and npvp_bias_act; "hip" sends the FoldedConvActs of the ENCODER that `_stem7x7_takes_hip` accepts (block0[0])
    through ops.stem7x7_packed (inference only: one launch on the planar frames the data path hands over, padding as index math, bias
    and ReLU in the epilogue, channels-last out with its amax slot).  A frame tensor in another layout keeps the stock forward.  Any
    other value is refused, before anything is changed.  The six switches are independent, and the state dict is the same under
    every combination."""
    _check_attn2d(attn2d)
    _check_conv3x3(conv3x3)
    _check_down3x3(down3x3)
    _check_up3x3(up3x3)
    _check_tail7x7(tail7x7)
    _check_stem7x7(stem7x7)
    for m in (enc, dec):
        assert not m.training, "fuse_frozen_autoencoder: eval mode only (BatchNorm must use its running statistics)"
        for q in m.parameters():
            q.requires_grad_(False)          # Stage 2 never trains the pair (ref/models/Predictor.py:17-25)
    with torch.no_grad():
        for name, mod in list(enc.named_children()):
            if isinstance(mod, nn.Sequential):
                setattr(enc, name, _fold_sequential(mod))
            elif isinstance(mod, Factorized3DConvAttn):
                mod.spatial_conv = _fold_sequential(mod.spatial_conv)[0]
                a = mod.attn2d
                if isinstance(a.norm_func, nn.BatchNorm2d):      # fold the BatchNorm behind out_proj into the Linear
                    s, t = _bn_scale_shift(a.norm_func)
                    a.out_proj.weight.mul_(s.view(-1, 1))
                    a.out_proj.bias.copy_(a.out_proj.bias * s + t)
                    a.norm_func = nn.Identity()
                if attn2d == "hip" and _attn2d_takes_hip(a):
                    _register_wqkv(a)
                    a.forward = types.MethodType(_fused_attn2d, a)
                if mod.learn_3d:
                    mod.temporal_conv = FoldedTemporalConvAct(mod.temporal_conv[0], mod.temporal_conv[1] if isinstance(
                        mod.temporal_conv[1], nn.BatchNorm1d) else None, mod.temporal_conv[2])
                    a = mod.attn1d
                    if isinstance(a.norm_func, nn.BatchNorm1d):      # ... and the BatchNorm1d behind attn1d's out_proj
                        s, t = _bn_scale_shift(a.norm_func)
                        a.out_proj.weight.mul_(s.view(-1, 1))
                        a.out_proj.bias.copy_(a.out_proj.bias * s + t)
                        a.norm_func = nn.Identity()
                    _register_wqkv(a)
            elif isinstance(mod, ResnetBlock):
                mod.conv_block = _fold_sequential(mod.conv_block)
        if conv3x3 == "hip":
            _route_conv3x3([m for m in enc.modules() if isinstance(m, FoldedConvAct)])
        if down3x3 == "hip":
            _route_down3x3([m for m in enc.modules() if isinstance(m, FoldedConvAct)])
        if stem7x7 == "hip":
            _route_stem7x7([m for m in enc.modules() if isinstance(m, FoldedConvAct)])
        dec.model = _fold_sequential(dec.model)
        if tail7x7 == "hip":
            _route_tail7x7(list(dec.model))
            dec.tail7x7 = any(m.tail7x7 for m in dec.model)
        if up3x3 == "hip":
            _route_up3x3(list(dec.model))
            if UP3X3_TAIL == "nchw" and not dec.tail7x7:         # (a routed tail reads channels-last: the stock remainder stays there)
                for m in dec.model:
                    if not m.up3x3:
                        m.weight = m.weight.contiguous()
            dec.up3x3 = True
    return enc, dec


class NonLocalAttenion2D(nn.Module):
    """Self-attention over the H*W positions of one frame with 2x2 max-pooled keys/values
    (ref/models/submodules.py:98-176).  (sic: the reference spells it 'Attenion'.)"""

    def __init__(self, in_channels, atten_channels_downsample_ratio=8, value_channels_downsample_ratio=2, bias=True,
                 learn_gamma=True, norm_func=None, activ_func=None):
        super().__init__()
        self.bias, self.in_channels = bias, in_channels
        self.attn_dim = in_channels // atten_channels_downsample_ratio
        self.value_dim = in_channels // value_channels_downsample_ratio
        self.Wq = nn.Linear(in_channels, self.attn_dim, bias=bias)
        self.Wk = nn.Linear(in_channels, self.attn_dim, bias=bias)
        self.Wv = nn.Linear(in_channels, self.value_dim, bias=bias)
        self.out_proj = nn.Linear(self.value_dim, in_channels, bias=bias)
        self.max_pool = nn.MaxPool2d((2, 2), stride=2)
        self.learn_gamma = learn_gamma
        self.gamma = nn.Parameter(torch.tensor(0., dtype=torch.float32)) if learn_gamma else 1.0
        self.norm_func = norm_func if norm_func is not None else nn.Identity()
        self.activ_func = activ_func if activ_func is not None else nn.Identity()
        for lin in (self.Wq, self.Wk, self.Wv, self.out_proj):
            nn.init.xavier_uniform_(lin.weight)
            if bias:
                nn.init.constant_(lin.bias, 0.)

    def forward(self, x):
        N, C, H, W = x.shape
        tok = x.flatten(2).transpose(1, 2)                                        # (N, HW, C)
        q = self.Wq(tok)                                                          # (N, HW, a)
        k = self.max_pool(self.Wk(tok).transpose(1, 2).reshape(N, self.attn_dim, H, W)).flatten(2)      # (N, a, HW/4)
        v = self.max_pool(self.Wv(tok).transpose(1, 2).reshape(N, self.value_dim, H, W)).flatten(2)     # (N, v, HW/4)
        att = F.softmax(q @ k, dim=-1)                                            # un-scaled scores, as the reference
        out = self.out_proj(att @ v.transpose(1, 2))                              # (N, HW, C)
        out = out.transpose(1, 2).reshape(N, C, H, W)
        return x + self.gamma * self.activ_func(self.norm_func(out))


class NonLocalAttenion1D(nn.Module):
    """Self-attention over the T frames of one pixel, x (N*H*W, C, T) (ref/models/submodules.py:182-255; un-scaled scores, one head,
    no pooling).  (sic: the reference spells it 'Attenion'.)"""

    def __init__(self, in_channels, atten_channels_downsample_ratio=8, value_channels_downsample_ratio=2, bias=True,
                 learn_gamma=True, norm_func=None, activ_func=None):
        super().__init__()
        self.bias, self.in_channels = bias, in_channels
        self.attn_dim = in_channels // atten_channels_downsample_ratio
        self.value_dim = in_channels // value_channels_downsample_ratio
        self.Wq = nn.Linear(in_channels, self.attn_dim, bias=bias)
        self.Wk = nn.Linear(in_channels, self.attn_dim, bias=bias)
        self.Wv = nn.Linear(in_channels, self.value_dim, bias=bias)
        self.out_proj = nn.Linear(self.value_dim, in_channels, bias=bias)
        self.learn_gamma = learn_gamma
        self.gamma = nn.Parameter(torch.tensor(0., dtype=torch.float32)) if learn_gamma else 1.0
        self.norm_func = norm_func if norm_func is not None else nn.Identity()
        self.activ_func = activ_func if activ_func is not None else nn.Identity()
        for lin in (self.Wq, self.Wk, self.Wv, self.out_proj):
            nn.init.xavier_uniform_(lin.weight)
            if bias:
                nn.init.constant_(lin.bias, 0.)

    def forward(self, x):
        tok = x.transpose(1, 2)                                                   # (M, T, C)
        att = F.softmax(self.Wq(tok) @ self.Wk(tok).transpose(1, 2), dim=-1)      # (M, T, T), un-scaled scores, as the reference
        out = self.out_proj(att @ self.Wv(tok)).transpose(1, 2)                   # (M, C, T)
        return x + self.gamma * self.activ_func(self.norm_func(out))


class FoldedTemporalConvAct(nn.Module):
    """Conv1d(C, C, 3, 'same') over T -> BatchNorm1d (eval) -> ReLU (+ skip) of a FROZEN Factorized3DConvAttn on the (N*T, C, H, W)
    frames themselves: that tensor, channels-last, IS a channels-last (N, C, T, H*W) tensor, the Conv1d a conv2d with a [C, C, 3, 1]
    filter and padding (1, 0) (zero padding per clip by construction).  BatchNorm folded into the weights, one npvp_bias_act pass."""

    def __init__(self, conv, bn, act):
        super().__init__()
        assert isinstance(conv, nn.Conv1d) and conv.groups == 1 and conv.kernel_size == (3,) and conv.stride == (1,) and conv.dilation == (1,)
        w = conv.weight.detach()
        b = conv.bias.detach() if conv.bias is not None else torch.zeros(conv.out_channels, dtype=w.dtype, device=w.device)
        if bn is not None:
            assert isinstance(bn, nn.BatchNorm1d) and not bn.training and bn.track_running_stats, "fold needs an eval-mode BatchNorm1d"
            s, t = _bn_scale_shift(bn)
            w = w * s.view(-1, 1, 1)
            b = b * s + t
        self.register_buffer("weight", w.unsqueeze(-1).contiguous(memory_format=torch.channels_last))        # [C, C, 3, 1]
        self.register_buffer("bias", b.detach().float().contiguous())
        self.act = 0 if act is None else _ACT_CODE[type(act)]

    def forward(self, x, T, residual=None):
        y = _temporal_view_back(F.conv2d(_temporal_view(x, T), self.weight, None, 1, (1, 0)), x.shape)
        return ops.bias_act(y, self.bias, self.act, residual)


def _temporal_view(x, T):
    """(N*T, C, H, W) -> (N, C, T, H*W): element (n, c, t, p) is x[n*T + t, c, p / W, p % W].  No copy when x is channels_last (the
    result is then a channels_last 4-D tensor) - what the reference reaches by reshape + permute + flatten (submodules.py:63)."""
    NT, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(NT // T, T, H * W, C).permute(0, 3, 1, 2)       # (an NCHW x is copied to channels_last here)


def _temporal_view_back(y, shape):
    """inverse of _temporal_view: (N, C, T, H*W) -> (N*T, C, H, W), a view of a channels_last y"""
    NT, C, H, W = shape
    return y.permute(0, 2, 3, 1).reshape(NT, H, W, C).permute(0, 3, 1, 2)


class Factorized3DConvAttn(nn.Module):
    """ref/models/submodules.py:9-95: conv3x3+BN+ReLU (+skip) -> NonLocalAttenion2D [-> per pixel over its T frames: Conv1d+BN+ReLU
    (+skip) -> NonLocalAttenion1D, with learn_3d] -> +skip; conv_first=False runs each attention before its convolution."""

    def __init__(self, in_channels, atten_channels_downsample_ratio=8, value_channels_downsample_ratio=2, use_bias=True,
                 learn_gamma=True, norm_layer_2d=nn.BatchNorm2d, norm_layer_1d=nn.BatchNorm1d, activ_func=nn.ReLU(),
                 conv_first=True, learn_3d=True):
        super().__init__()
        self.in_channels, self.learn_3d, self.conv_first = in_channels, learn_3d, conv_first
        self.spatial_conv = nn.Sequential(nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1, bias=use_bias),
                                          norm_layer_2d(in_channels), activ_func)
        self.attn2d = NonLocalAttenion2D(in_channels, atten_channels_downsample_ratio, value_channels_downsample_ratio, True,
                                         learn_gamma, norm_layer_2d(in_channels), activ_func=activ_func)
        self.temporal_conv = None
        self.attn1d = None
        if learn_3d:
            self.temporal_conv = nn.Sequential(nn.Conv1d(in_channels, in_channels, kernel_size=3, stride=1, padding='same', bias=use_bias),
                                               norm_layer_1d(in_channels), activ_func)
            self.attn1d = NonLocalAttenion1D(in_channels, atten_channels_downsample_ratio, value_channels_downsample_ratio, True,
                                             learn_gamma, norm_layer_1d(in_channels), activ_func=activ_func)

    def _spatial(self, x):
        if isinstance(self.spatial_conv, FoldedConvAct):       # fused: relu(conv + b) + x in the epilogue pass
            if self.conv_first:
                return self.attn2d(self.spatial_conv(x, residual=x))
            y = self.attn2d(x)
            return self.spatial_conv(y, residual=y)
        if self.conv_first:
            return self.attn2d(self.spatial_conv(x) + x)
        y = self.attn2d(x)
        return self.spatial_conv(y) + y

    def _temporal(self, x, T):
        """the learn_3d half (ref submodules.py:62-66, 86-91) on x (N*T, C, H, W)"""
        if isinstance(self.temporal_conv, FoldedTemporalConvAct):      # fused, on the frames in place (no permute copy)
            if self.conv_first:
                return _fused_attn1d(self.attn1d, self.temporal_conv(x, T, residual=x), T)
            y = _fused_attn1d(self.attn1d, x, T)
            return self.temporal_conv(y, T, residual=y)
        NT, C, H, W = x.shape
        N = NT // T
        y = x.reshape(N, T, C, H, W).permute(0, 3, 4, 2, 1).flatten(0, 2)          # (N*H*W, C, T)
        if self.conv_first:
            y = self.attn1d(self.temporal_conv(y) + y)
        else:
            y = self.attn1d(y)
            y = self.temporal_conv(y) + y
        return y.reshape(N, H, W, C, T).permute(0, 4, 3, 1, 2).flatten(0, 1)

    def forward(self, x, T):
        y = self._spatial(x)
        if self.learn_3d:
            y = self._temporal(y, T)
        return y + x


def _fused_attn1d(a, x, T):
    """NonLocalAttenion1D of a fused (frozen, eval) pair on the frames x (N*T, C, H, W): on the device the channels-last rows go
    through the temporal attention kernel (ops.temporal_attn_packed, above ops.TEMPORAL_ATTN_MAX_T frames its key-tiled form
    ops.temporal_attn_long_packed); BatchNorm1d is already folded into out_proj"""
    NT, C, H, W = x.shape
    A, V = a.attn_dim, a.value_dim
    tok = x.permute(0, 2, 3, 1).reshape(NT * H * W, C)                  # a view when x is channels_last
    qkv = F.linear(tok, a._npvp_wqkv, a._npvp_bqkv)
    o = ops.temporal_attn_any_packed(qkv, NT // T, T, H * W, A, V)
    out = a.out_proj(o).view(NT, H, W, C).permute(0, 3, 1, 2)
    return x + a.gamma * a.activ_func(a.norm_func(out))


def _fused_attn2d(a, x):
    """NonLocalAttenion2D.forward of a fused (frozen, eval) pair under attn2d="hip", on channels-last frames x (F, C, H, W): one GEMM
    for [Wq | Wk | Wv], the non-local attention kernels (ops.nonlocal_attn_any_packed: online softmax, K / V pooled 2x2 in the tile loads: no (F, HW, HW/4) tensor), one
    GEMM for out_proj and ONE pass  x + gamma * act(y + out_proj.bias[c])  (npvp_bias_act_scaled; gamma is read on the device).
    A grid without a 2x2 window or an input that is not channels-last keeps the stock forward (no silent copy)."""
    Fr, C, H, W = x.shape
    A, V = a.attn_dim, a.value_dim
    if H < 2 or W < 2 or x.is_contiguous() or not x.is_contiguous(memory_format=torch.channels_last):
        return NonLocalAttenion2D.forward(a, x)
    if torch.is_grad_enabled() and x.requires_grad:
        raise NotImplementedError('attn2d="hip" (to_device_layout / fuse_frozen_autoencoder) is inference-only: the input of this '
                                  'NonLocalAttenion2D requires grad; fuse the pair with attn2d="stock" to differentiate through it')
    tok = x.permute(0, 2, 3, 1).reshape(Fr * H * W, C)                  # a view of channels-last frames
    qkv = F.linear(tok, a._npvp_wqkv, a._npvp_bqkv)
    o = ops.nonlocal_attn_any_packed(qkv, Fr, H, W, A, V)
    y = F.linear(o, a.out_proj.weight).view(Fr, H, W, C).permute(0, 3, 1, 2)
    act = 0 if isinstance(a.activ_func, nn.Identity) else _ACT_CODE[type(a.activ_func)]
    return ops.bias_act_scaled(y, a.out_proj.bias, a.gamma if isinstance(a.gamma, torch.Tensor) else None, act, residual=x)


class ResnetBlock(nn.Module):
    """ref/models/ResNetAutoEncoder.py:206-261: x + [pad, conv3, norm, ReLU, (dropout), pad, conv3, norm](x)."""

    def __init__(self, dim, padding_type, norm_layer, use_dropout, use_bias):
        super().__init__()
        pads = {'reflect': nn.ReflectionPad2d, 'replicate': nn.ReplicationPad2d}
        layers = []
        for half in range(2):
            p = 0
            if padding_type in pads:
                layers.append(pads[padding_type](1))
            elif padding_type == 'zero':
                p = 1
            else:
                raise NotImplementedError('padding [%s] is not implemented' % padding_type)
            layers += [nn.Conv2d(dim, dim, kernel_size=3, padding=p, bias=use_bias), norm_layer(dim)]
            if half == 0:
                layers.append(nn.ReLU(True))
                if use_dropout:
                    layers.append(nn.Dropout(0.5))
        self.conv_block = nn.Sequential(*layers)

    def forward(self, x):
        if len(self.conv_block) == 2 and isinstance(self.conv_block[1], FoldedConvAct):      # fused: skip-add in the epilogue
            return self.conv_block[1](self.conv_block[0](x), residual=x)
        return x + self.conv_block(x)


def _use_bias(norm_layer):
    if type(norm_layer) == functools.partial:
        return norm_layer.func == nn.InstanceNorm2d
    return norm_layer == nn.InstanceNorm2d


class ResnetEncoder(nn.Module):
    """ref/models/ResNetAutoEncoder.py:51-146: (N,T,Ci,S,S) frames -> (N,T,ngf*2^n_down,S/2^n_down,S/2^n_down), ReLU'd."""

    def __init__(self, input_nc, ngf=64, n_downsampling=3, num_res_blocks=2, norm_layer=nn.BatchNorm2d,
                 norm_layer1d=nn.BatchNorm1d, use_dropout=False, padding_type='reflect', learn_3d=True):
        super().__init__()
        use_bias = _use_bias(norm_layer)
        self.n_downsampling, self.num_res_blocks = n_downsampling, num_res_blocks
        self.block0 = nn.Sequential(nn.ReflectionPad2d(3), nn.Conv2d(input_nc, ngf, kernel_size=7, padding=0, bias=use_bias),
                                    norm_layer(ngf), nn.ReLU(True))
        self.block1 = nn.Sequential(nn.Conv2d(ngf, ngf * 2, kernel_size=3, stride=2, padding=1, bias=use_bias),
                                    norm_layer(ngf * 2), nn.ReLU(True))
        ch = ngf * 2
        mk_attn = lambda c: Factorized3DConvAttn(in_channels=c, norm_layer_2d=norm_layer, norm_layer_1d=norm_layer1d,
                                                 activ_func=nn.ReLU(True), learn_3d=learn_3d)
        for i in range(1, n_downsampling):
            setattr(self, f'block{i + 1}_3dConvAttn', mk_attn(ch))
            setattr(self, f'block{i + 1}_conv', nn.Sequential(
                nn.Conv2d(ch, ch * 2, kernel_size=3, stride=2, padding=1, bias=use_bias), norm_layer(ch * 2), nn.ReLU(True)))
            ch *= 2
        for i in range(num_res_blocks):
            setattr(self, f'res_3dConvAttn_{i}', mk_attn(ch))
            setattr(self, f'res_conv_{i}', ResnetBlock(ch, padding_type=padding_type, norm_layer=norm_layer,
                                                       use_dropout=use_dropout, use_bias=use_bias))
        self.out_act = nn.ReLU()

    def forward(self, x):
        N, T = x.shape[:2]
        x = self.block1(self.block0(x.flatten(0, 1)))
        for i in range(1, self.n_downsampling):
            x = getattr(self, f'block{i + 1}_conv')(getattr(self, f'block{i + 1}_3dConvAttn')(x, T))
        for i in range(self.num_res_blocks):
            x = getattr(self, f'res_conv_{i}')(getattr(self, f'res_3dConvAttn_{i}')(x, T))
        x = self.out_act(x)
        return x.reshape(N, T, *x.shape[1:])


class ResnetDecoder(nn.Module):
    """ref/models/ResNetAutoEncoder.py:148-204: n_downsampling x [ConvTranspose2d s2 + norm + ReLU], 7x7 conv, Tanh/Sigmoid."""

    def __init__(self, output_nc, ngf=64, n_downsampling=2, norm_layer=nn.BatchNorm2d, use_dropout=False,
                 padding_type='reflect', out_layer='Tanh'):
        super().__init__()
        use_bias = _use_bias(norm_layer)
        model = []
        for i in range(n_downsampling):
            mult = 2 ** (n_downsampling - i)
            model += [nn.ConvTranspose2d(ngf * mult, ngf * mult // 2, kernel_size=3, stride=2, padding=1, output_padding=1,
                                         bias=use_bias), norm_layer(ngf * mult // 2), nn.ReLU(True)]
        model += [nn.ReflectionPad2d(3), nn.Conv2d(ngf, output_nc, kernel_size=7, padding=0)]
        if out_layer == 'Tanh':
            model.append(nn.Tanh())
        elif out_layer == 'Sigmoid':
            model.append(nn.Sigmoid())
        else:
            raise ValueError("Unsupported output layer")
        self.model = nn.Sequential(*model)

    up3x3 = False          # True on a fused decoder whose transposed convolutions are routed (fuse_frozen_autoencoder(up3x3="hip"))
    tail7x7 = False        # True on a fused decoder whose 7 x 7 tail is routed (fuse_frozen_autoencoder(tail7x7="hip"))

    def forward(self, x):
        N, T = x.shape[:2]
        y = x.flatten(0, 1)
        if self.up3x3 or self.tail7x7:
            if self.up3x3:
                # the routed kernels are channels-last and the predictor hands out NCHW: ONE explicit, differentiable copy at the entry
                y = y.contiguous(memory_format=torch.channels_last)
            for m in self.model:
                if m.tail7x7:
                    if not _channels_last_only(y):
                        y = y.contiguous(memory_format=torch.channels_last)      # (up3x3="stock": ONE explicit, differentiable copy)
                elif not m.up3x3 and m.weight.is_contiguous() and not y.is_contiguous():
                    y = y.contiguous()                   # the stock remainder runs in its weights' layout (UP3X3_TAIL): one copy back to NCHW
                y = m(y)
        else:
            y = self.model(y)
        return y.reshape(N, T, *y.shape[1:])


def build_frozen_autoencoder(AE, img_channels):
    """(encoder, decoder) as LitPredictor.__init__ prepares them (ref/models/Predictor.py:17-25): built from the `AE:`
    section of a reference YAML, parameters frozen, eval mode (BatchNorm uses running statistics)."""
    enc = ResnetEncoder(img_channels, ngf=AE['ngf'], n_downsampling=AE['n_downsampling'], num_res_blocks=AE['num_res_blocks'],
                        norm_layer=nn.BatchNorm2d, norm_layer1d=nn.BatchNorm1d, learn_3d=AE['learn_3d'])
    dec = ResnetDecoder(img_channels, ngf=AE['ngf'], n_downsampling=AE['n_downsampling'], out_layer=AE['out_layer'],
                        norm_layer=nn.BatchNorm2d)
    for m in (enc, dec):
        for p in m.parameters():
            p.requires_grad_(False)
        m.eval()
    return enc, dec


def to_device_layout(enc, dec, device, attn2d="stock", conv3x3="stock", down3x3="stock", up3x3="stock", tail7x7="stock",
                     stem7x7="stock"):
    """Move the frozen pair to an MI355X.  The ENCODER runs in torch.channels_last (MIOpen's NHWC kernels: 27.5 -> 24.8 ms
    for 640 frames of 64x64, and its (N*T,H,W,C) output is the predictor's canonical layout, so the layout transpose at
    the predictor's entry disappears); the decoder stays NCHW (NHWC measured slower: 9.0 -> 11.2 ms fwd + input-grad on MIOpen)
    unless up3x3="hip" routes its transposed convolutions to the channels-last kernel: then it is moved to torch.channels_last too,
    and fuse_frozen_autoencoder gives the stock remainder (the 7 x 7 tail) its NCHW weights back (`UP3X3_TAIL`: measured faster).
    tail7x7="hip" routes that tail to the kernels of csrc/conv7x7.hip, which read channels-last frames and write NCHW ones.
    stem7x7="hip" routes the encoder's 7 x 7 stem to the stem kernel of the same file, which reads the planar frames as they come and
    writes channels-last ones."""
    _check_attn2d(attn2d)
    _check_conv3x3(conv3x3)
    _check_down3x3(down3x3)
    _check_up3x3(up3x3)
    _check_tail7x7(tail7x7)
    _check_stem7x7(stem7x7)
    enc, dec = enc.to(device).to(memory_format=torch.channels_last), dec.to(device)
    if up3x3 == "hip":
        dec = dec.to(memory_format=torch.channels_last)
    return fuse_frozen_autoencoder(enc.eval(), dec.eval(), attn2d=attn2d, conv3x3=conv3x3, down3x3=down3x3, up3x3=up3x3,
                                   tail7x7=tail7x7, stem7x7=stem7x7)
