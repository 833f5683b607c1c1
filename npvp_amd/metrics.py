"""Evaluation metrics on device: drop-in for ref/utils/metrics.py:12-140 (`PSNR`, `MSEScore`, `SSIM`,
`pred_ave_metrics`) - same names, arguments and return types - with the reductions and the five Gaussian-filtered
maps of SSIM done by libnpvp_hip.so (csrc/metrics.hip: every image pair is read once).  Inputs must be fp32 tensors
on an MI355X; there is no CPU path (RuntimeError), as everywhere in this package.
"""
from math import exp

import numpy as np
import torch

from . import ops
from ._lib import lib


def _pair(x, y):
    if x.shape != y.shape or x.dim() != 4:
        raise ValueError(f"metrics: two (N, C, H, W) tensors of equal shape are needed, got {tuple(x.shape)} and {tuple(y.shape)}")
    if not (x.is_cuda and y.is_cuda):
        raise RuntimeError("npvp_amd.metrics runs on the GPU only (no CPU fallback): move the frames to the device")
    return x.detach().float().contiguous(), y.detach().float().contiguous()


def _sqdiff(x, y, data_range, scale):
    x, y = _pair(x, y)
    N, per = x.shape[0], x[0].numel()
    L = lib()
    out = torch.empty(N, dtype=torch.float32, device=x.device)
    ws, wsn = ops._ws(L.npvp_sqdiff_workspace_bytes(N, per), x.device)
    ops.check(L.npvp_sqdiff_per_image(ops._ptr(x), ops._ptr(y), N, per, float(data_range), float(scale), ops._ptr(out),
                                       ops._ptr(ws), wsn, ops._stream()), "npvp_sqdiff_per_image")
    return out


def PSNR(x, y, data_range=1.0, mean_flag=True):
    """average (or per-image) PSNR of two batches of (N, C, H, W) images   ref/utils/metrics.py:12-30"""
    mse = _sqdiff(x, y, data_range, 1.0 / x[0].numel())
    score = -10 * torch.log10(mse + 1e-8)
    return torch.mean(score).item() if mean_flag else score


def MSEScore(x, y, mean_flag=True):
    """per-image SUM of squared differences (ref/utils/metrics.py:32-43), averaged over the batch if mean_flag"""
    mse = _sqdiff(x, y, 1.0, 1.0)
    return torch.mean(mse).item() if mean_flag else mse


class SSIM(torch.nn.Module):
    """ref/utils/metrics.py:46-108: Gaussian-window SSIM (sigma 1.5, zero padding), C1 = 0.01^2, C2 = 0.03^2."""

    def __init__(self, window_size=11):
        super().__init__()
        self.window_size = window_size
        self.channel = 1
        self.window = self.create_window(window_size, self.channel)
        self.__name__ = 'SSIM'

    def gaussian(self, window_size, sigma):
        gauss = torch.Tensor([exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)])
        return gauss / gauss.sum()

    def create_window(self, window_size, channel):
        """the reference's (channel, 1, ws, ws) grouped-conv window; the kernel applies its two 1-D factors separably"""
        g = self.gaussian(window_size, 1.5).unsqueeze(1)
        return g.mm(g.t()).float().unsqueeze(0).unsqueeze(0).expand(channel, 1, window_size, window_size).contiguous()

    def forward(self, img1, img2, mean_flag=True):
        img1, img2 = _pair(img1, img2)
        N, C, H, W = img1.shape
        self.channel = C
        taps = np.ascontiguousarray(self.gaussian(self.window_size, 1.5).numpy(), dtype=np.float32)
        L = lib()
        out = torch.empty(N, dtype=torch.float32, device=img1.device)
        ws, wsn = ops._ws(L.npvp_ssim_workspace_bytes(N, C, H, W), img1.device)
        ops.check(L.npvp_ssim_per_image(ops._ptr(img1), ops._ptr(img2), N, C, H, W, taps.ctypes.data, self.window_size,
                                         ops._ptr(out), ops._ptr(ws), wsn, ops._stream()), "npvp_ssim_per_image")
        return out.mean() if mean_flag else out


def pred_ave_metrics(model, data_loader, metric_func, renorm_transform, num_future_frames, ckpt=None, device='cuda:0'):
    """Per-time-step average of `metric_func` over a data loader (ref/utils/metrics.py:110-140).  `model(past, future,
    None)[0]` must give the predicted frames (N, Tp, C, H, W) as in the reference; `ckpt`, if given, is a Lightning
    checkpoint loaded with npvp_amd.load_lightning_checkpoint into `model.predictor` (or `model`)."""
    if ckpt is not None:
        from .trainer import load_lightning_checkpoint
        load_lightning_checkpoint(ckpt, getattr(model, "predictor", model))
    model = model.eval()
    ave_metric = np.zeros(num_future_frames)
    sample_num = 0
    with torch.no_grad():
        for past_frames, future_frames in data_loader:
            past_frames, future_frames = past_frames.to(device), future_frames.to(device)
            pred = model(past_frames, future_frames, None)[0]
            for i in range(num_future_frames):
                pred_t, gt_t = pred[:, i, ...], future_frames[:, i, ...]
                m = metric_func(renorm_transform(pred_t), renorm_transform(gt_t))
                ave_metric[i] += float(m) * pred_t.shape[0]
            sample_num += pred.shape[0]
    return ave_metric / sample_num


def best_of_samples(pred, target, metric_func, higher_is_better=True):
    """Best-of-S evaluation of a stochastic predictor, on the device: pred (N, S, T, C, H, W) - what Predictor.sample and
    predictor_sample_step return - against target (N, T, C, H, W) under the per-image form (`mean_flag=False`) of `SSIM` / `PSNR` /
    `MSEScore`.  -> best_idx [N] (the sample with the best mean over T; ties go to the lowest index), best [N, T] (that sample's
    per-step values) and all [N, S, T].  One metric call per sample on the N * T frames of that sample's slab pred[:, s] (contiguous
    in the sampler's sample-major result; a per-image metric gives every image the same value however the images are batched).
    Nothing is converted to a host number in here."""
    if pred.dim() != 6 or target.dim() != 5 or pred.shape[0] != target.shape[0] or pred.shape[2:] != target.shape[1:]:
        raise ValueError(f"best_of_samples: pred (N, S, T, C, H, W) and target (N, T, C, H, W) are needed, got {tuple(pred.shape)} "
                         f"and {tuple(target.shape)}")
    N, S, T = pred.shape[:3]
    img = tuple(pred.shape[3:])
    tgt = target.reshape((N * T,) + img)
    vals = [metric_func(pred[:, s].reshape((N * T,) + img), tgt, mean_flag=False).reshape(N, T) for s in range(S)]
    every = torch.stack(vals, dim=1)                                  # [N, S, T]
    score = every.mean(dim=2)                                         # [N, S]
    top = score.max(dim=1, keepdim=True).values if higher_is_better else score.min(dim=1, keepdim=True).values
    order = torch.arange(S, device=score.device).expand(N, S)
    best_idx = torch.where(score == top, order, torch.full_like(order, S)).min(dim=1).values      # lowest index among the ties
    best = every.gather(1, best_idx.view(N, 1, 1).expand(N, 1, T)).squeeze(1)
    return best_idx, best, every


def pred_best_metrics(model, data_loader, metric_func, renorm_transform, num_future_frames, n_samples, seed, higher_is_better=True,
                      ckpt=None, device='cuda:0'):
    """The best-of-S counterpart of `pred_ave_metrics`: per-time-step average over a data loader of the best sample's `metric_func`
    (per clip: the sample with the best mean over the future steps).  `model.sample(past_frames, n_samples, seed=seed,
    sample_base=k)` must give the sampled frames (N, S, Tp, C, H, W); batch b draws samples b * n_samples .. of the seed's stream.
    One host transfer per batch (the [Tp] sums), none per time-step."""
    if ckpt is not None:
        from .trainer import load_lightning_checkpoint
        load_lightning_checkpoint(ckpt, getattr(model, "predictor", model))
    model = model.eval()
    ave_metric = np.zeros(num_future_frames)
    sample_num = 0
    with torch.no_grad():
        for b, (past_frames, future_frames) in enumerate(data_loader):
            past_frames, future_frames = past_frames.to(device), future_frames.to(device)
            pred = model.sample(past_frames, n_samples, seed=seed, sample_base=b * n_samples)
            N, S, T = pred.shape[:3]
            img = tuple(pred.shape[3:])
            # renormalise frame by frame, in the sample-major order the sampler produced (no re-layout of its result)
            p = renorm_transform(pred.permute(1, 0, 2, 3, 4, 5).reshape((S * N * T,) + img))
            p = p.view((S, N, T) + tuple(p.shape[1:])).permute(1, 0, 2, 3, 4, 5)
            g = renorm_transform(future_frames.reshape((N * T,) + img))
            g = g.view((N, T) + tuple(g.shape[1:]))
            _, best, _ = best_of_samples(p[:, :, :num_future_frames], g[:, :num_future_frames], metric_func, higher_is_better)
            ave_metric += best.sum(dim=0).double().cpu().numpy()
            sample_num += N
    return ave_metric / sample_num
