"""The training loss on the HIP library: (1 - lambda) L1 + lambda (1 - mean SSIM), one kernel per direction
(csrc/gcp_loss.hip), and the evaluation metrics on the same tiling: per-image squared error, L1 and SSIM in one pass
(`image_metrics`).  The PyTorch formulation both are tested against: oracle/loss_torch.py."""
from typing import NamedTuple

import torch

from . import _lib

_WINDOW_CACHE = {}


def _host_window(window_size, sigma):
    """The normalised window as a ctypes float array (host memory, handed to the loss kernels by value)."""
    import ctypes

    key = (window_size, sigma)
    if key not in _WINDOW_CACHE:
        x = torch.arange(window_size, dtype=torch.float32) - (window_size - 1) / 2
        w = torch.exp(-(x * x) / (2 * sigma * sigma))
        _WINDOW_CACHE[key] = (ctypes.c_float * window_size)(*(w / w.sum()).tolist())
    return _WINDOW_CACHE[key]


class _SplatLoss(torch.autograd.Function):
    """(1 - lambda) L1 + lambda (1 - mean SSIM) in one HIP kernel per direction (csrc/gcp_loss.hip); differentiable in
    the first image only (the second is the target photograph)."""

    @staticmethod
    def forward(ctx, images, targets, lamda, max_val):
        if not images.is_cuda:
            raise RuntimeError("the fused loss is a HIP kernel: tensors must live on the GPU (no CPU path)")
        if images.shape != targets.shape or images.dim() != 4:
            raise RuntimeError("splat_loss expects two (B, C, H, W) tensors of one shape")
        a, b = images.detach().contiguous().float(), targets.detach().contiguous().float()
        bsz, ch, h, w = a.shape
        lib = _lib.load()
        win = _host_window(11, 1.5)
        need_grad = images.requires_grad
        maps = [torch.empty_like(a) for _ in range(3)] if need_grad else [None] * 3
        with torch.cuda.device(a.device):
            stream = torch.cuda.current_stream(a.device).cuda_stream
            partial = torch.empty(lib.gcp_ssim_blocks(bsz * ch, h, w), 2, dtype=torch.float32, device=a.device)
            _lib.check(lib.gcp_ssim_l1_forward(a.data_ptr(), b.data_ptr(), bsz * ch, h, w, win, (0.01 * max_val) ** 2,
                                               (0.03 * max_val) ** 2, *(m.data_ptr() if need_grad else None for m in maps),
                                               partial.data_ptr(), stream), "gcp_ssim_l1_forward")
        sums = partial.double().sum(dim=0) / a.numel()  # [mean SSIM, mean |a - b|]
        ctx.save_for_backward(a, b, *(maps if need_grad else []))
        ctx.lamda, ctx.dtype = lamda, images.dtype
        return ((1 - lamda) * sums[1] + lamda * (1 - sums[0])).to(images.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        a, b, m1, m2, m3 = ctx.saved_tensors
        n = a.numel()
        scales = (grad_out.reshape(1).float() * torch.tensor([-ctx.lamda / n, (1 - ctx.lamda) / n], device=a.device)).contiguous()
        grad = torch.empty_like(a)
        bsz, ch, h, w = a.shape
        with torch.cuda.device(a.device):
            stream = torch.cuda.current_stream(a.device).cuda_stream
            _lib.check(_lib.load().gcp_ssim_l1_backward(a.data_ptr(), b.data_ptr(), m1.data_ptr(), m2.data_ptr(), m3.data_ptr(), bsz * ch,
                                                        h, w, _host_window(11, 1.5), scales.data_ptr(), grad.data_ptr(), stream),
                       "gcp_ssim_l1_backward")
        return grad.to(ctx.dtype), None, None, None


def splat_loss(images, targets, lamda=0.2):
    """(1 - lambda) L1 + lambda (1 - mean SSIM), 11-tap Gaussian window, reflect padding (reference:
    gs_control.py:180-182, kornia.metrics.ssim).  Both terms and their gradient are one HIP kernel per direction
    (csrc/gcp_loss.hip); GPU tensors only.  The PyTorch formulation it is tested against: oracle/loss_torch.py."""
    return _SplatLoss.apply(images, targets, float(lamda), 1.0)


class ImageMetrics(NamedTuple):
    """One entry per image, float64 on the device: mean squared error, mean |a - b|, mean SSIM, and
    psnr = 10 log10(max_val^2 / mse) (inf where mse == 0)."""
    mse: torch.Tensor
    l1: torch.Tensor
    ssim: torch.Tensor
    psnr: torch.Tensor


def psnr_from_mse(mse, max_val=1.0):
    """10 log10(max_val^2 / mse) with torch, on mse's device; inf where mse == 0."""
    return 10.0 * torch.log10((max_val * max_val) / mse)


def image_metrics(images, targets, clamp=True, max_val=1.0):
    """Per-image evaluation metrics of (B, C, H, W) `images` against `targets` -> ImageMetrics of float64 (B,) device tensors.
    One HIP pass over both (gcp_image_metrics, csrc/gcp_loss.hip): SSIM with the 11-tap Gaussian window and reflect padding of
    `splat_loss`, c1, c2 = (0.01 max_val)^2, (0.03 max_val)^2.  clamp=True: `images` (never `targets`) is clamped to [0, 1] as
    it is read — what an 8-bit file of the render would hold, and what other 3DGS trainers evaluate — and all three terms see
    the clamped value.  An image's numbers depend on that image alone, and two calls give the same bits (no atomics).  No
    autograd (the outputs are detached), no device->host read; the inputs need not be contiguous or float32 (converted as
    `splat_loss` converts them).  GPU tensors only.  LPIPS is not computed: it needs pretrained network weights."""
    if not images.is_cuda:
        raise RuntimeError("image_metrics is a HIP kernel: tensors must live on the GPU (no CPU path)")
    if images.shape != targets.shape or images.dim() != 4:
        raise RuntimeError("image_metrics expects two (B, C, H, W) tensors of one shape")
    a, b = images.detach().contiguous().float(), targets.detach().contiguous().float()
    bsz, ch, h, w = a.shape
    lib = _lib.load()
    with torch.cuda.device(a.device):
        stream = torch.cuda.current_stream(a.device).cuda_stream
        partial = torch.empty(lib.gcp_ssim_blocks(bsz * ch, h, w), 3, dtype=torch.float32, device=a.device)
        out = torch.empty(bsz, 3, dtype=torch.float64, device=a.device)
        _lib.check(lib.gcp_image_metrics(a.data_ptr(), b.data_ptr(), bsz, ch, h, w, _host_window(11, 1.5), (0.01 * max_val) ** 2,
                                         (0.03 * max_val) ** 2, _lib.METRICS_CLAMP if clamp else 0, partial.data_ptr(),
                                         out.data_ptr(), stream), "gcp_image_metrics")
    mse, l1, ssim = out.t().contiguous().unbind(dim=0)
    return ImageMetrics(mse, l1, ssim, psnr_from_mse(mse, max_val))
