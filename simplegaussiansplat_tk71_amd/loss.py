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


def _check_exposure(what, images, targets, exposure):
    """The refusals of the exposure paths, before the library is touched -> (a, b, e): contiguous float32, detached."""
    if images.shape != targets.shape or images.dim() != 4:
        raise RuntimeError(f"{what} expects two (B, C, H, W) tensors of one shape")
    if images.shape[1] != 3:
        raise RuntimeError(f"{what}: an exposure is a colour affine of three channels, got C = {images.shape[1]}")
    if not torch.is_tensor(exposure) or tuple(exposure.shape) != (images.shape[0], 3, 4):
        raise RuntimeError(f"{what}: exposure must be a (B, 3, 4) tensor with B = {images.shape[0]}, "
                           f"got {tuple(exposure.shape) if torch.is_tensor(exposure) else type(exposure).__name__}")
    if not images.is_cuda:
        raise RuntimeError(f"{what} is a HIP kernel: tensors must live on the GPU (no CPU path)")
    if exposure.device != images.device or targets.device != images.device:
        raise RuntimeError(f"{what}: images, targets and exposure must live on one device")
    return images.detach().contiguous().float(), targets.detach().contiguous().float(), exposure.detach().contiguous().float()


class _SplatLossExposure(torch.autograd.Function):
    """`_SplatLoss` of the compensated render y = E[:, :, :3] x + E[:, :, 3], differentiable in the render and in the
    exposure; y is formed inside the kernels (csrc/gcp_loss.hip: k_ssim_l1_fwd_exposure, k_ssim_l1_bwd_exposure,
    k_exposure_fold) and never stored."""

    @staticmethod
    def forward(ctx, images, targets, exposure, lamda, max_val):
        a, b, e = _check_exposure("splat_loss with an exposure", images, targets, exposure)
        bsz, _, h, w = a.shape
        lib = _lib.load()
        win = _host_window(11, 1.5)
        need_grad = images.requires_grad or exposure.requires_grad
        maps = [torch.empty_like(a) for _ in range(3)] if need_grad else [None] * 3
        with torch.cuda.device(a.device):
            stream = torch.cuda.current_stream(a.device).cuda_stream
            partial = torch.empty(lib.gcp_ssim_blocks(bsz * 3, h, w), 2, dtype=torch.float32, device=a.device)
            _lib.check(lib.gcp_ssim_l1_forward_exposure(a.data_ptr(), b.data_ptr(), e.data_ptr(), bsz, h, w, win, (0.01 * max_val) ** 2,
                                                        (0.03 * max_val) ** 2, *(m.data_ptr() if need_grad else None for m in maps),
                                                        partial.data_ptr(), stream), "gcp_ssim_l1_forward_exposure")
        sums = partial.double().sum(dim=0) / a.numel()  # [mean SSIM, mean |y - b|]
        ctx.save_for_backward(a, b, e, *(maps if need_grad else []))
        ctx.lamda, ctx.dtype, ctx.e_dtype = lamda, images.dtype, exposure.dtype
        return ((1 - lamda) * sums[1] + lamda * (1 - sums[0])).to(images.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        a, b, e, m1, m2, m3 = ctx.saved_tensors
        n = a.numel()
        want_x, want_e = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        scales = (grad_out.reshape(1).float() * torch.tensor([-ctx.lamda / n, (1 - ctx.lamda) / n], device=a.device)).contiguous()
        bsz, _, h, w = a.shape
        lib = _lib.load()
        grad = torch.empty_like(a) if want_x else None
        grad_e = torch.empty_like(e) if want_e else None  # every entry is written
        with torch.cuda.device(a.device):
            stream = torch.cuda.current_stream(a.device).cuda_stream
            partial_e = torch.empty(lib.gcp_exposure_blocks(bsz, h, w), 12, dtype=torch.float32, device=a.device) if want_e else None
            _lib.check(lib.gcp_ssim_l1_backward_exposure(a.data_ptr(), b.data_ptr(), e.data_ptr(), m1.data_ptr(), m2.data_ptr(), m3.data_ptr(),
                                                         bsz, h, w, _host_window(11, 1.5), scales.data_ptr(),
                                                         grad.data_ptr() if want_x else None, partial_e.data_ptr() if want_e else None,
                                                         grad_e.data_ptr() if want_e else None, stream), "gcp_ssim_l1_backward_exposure")
        return (grad.to(ctx.dtype) if want_x else None), None, (grad_e.to(ctx.e_dtype) if want_e else None), None, None


def splat_loss(images, targets, lamda=0.2, exposure=None):
    """(1 - lambda) L1 + lambda (1 - mean SSIM), 11-tap Gaussian window, reflect padding (reference:
    gs_control.py:180-182, kornia.metrics.ssim).  Both terms and their gradient are one HIP kernel per direction
    (csrc/gcp_loss.hip); GPU tensors only.  The PyTorch formulation it is tested against: oracle/loss_torch.py.
    `exposure` (B, 3, 4), one colour affine per image (`exposure.CameraExposure.rows`): the loss of
    y_c = E[c][0] x_0 + E[c][1] x_1 + E[c][2] x_2 + E[c][3] against the targets, three channels only, differentiable in
    `images` and in `exposure` (either may require a gradient alone; no double backward).  y is formed inside the kernels
    and never stored; E = [I | 0] gives the bits of exposure=None, and None (the default) takes the plain kernels."""
    if exposure is None:
        return _SplatLoss.apply(images, targets, float(lamda), 1.0)
    _check_exposure("splat_loss with an exposure", images, targets, exposure)
    return _SplatLossExposure.apply(images, targets, exposure, float(lamda), 1.0)


def apply_exposure(images, exposure):
    """The compensated images y = E[:, :, :3] x + E[:, :, 3] of (B, 3, H, W) `images` and (B, 3, 4) `exposure`, with plain
    torch operations (differentiable, any device): for writing compensated renders to disk.  Not on the training path:
    `splat_loss(exposure=)` and `image_metrics(exposure=)` form y inside their kernels."""
    if images.dim() != 4 or images.shape[1] != 3 or tuple(exposure.shape) != (images.shape[0], 3, 4):
        raise RuntimeError("apply_exposure expects (B, 3, H, W) images and a (B, 3, 4) exposure")
    return torch.einsum("bck,bkhw->bchw", exposure[..., :3], images) + exposure[..., 3, None, None]


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


def image_metrics(images, targets, clamp=True, max_val=1.0, exposure=None):
    """Per-image evaluation metrics of (B, C, H, W) `images` against `targets` -> ImageMetrics of float64 (B,) device tensors.
    One HIP pass over both (gcp_image_metrics, csrc/gcp_loss.hip): SSIM with the 11-tap Gaussian window and reflect padding of
    `splat_loss`, c1, c2 = (0.01 max_val)^2, (0.03 max_val)^2.  clamp=True: `images` (never `targets`) is clamped to [0, 1] as
    it is read — what an 8-bit file of the render would hold, and what other 3DGS trainers evaluate — and all three terms see
    the clamped value.  An image's numbers depend on that image alone, and two calls give the same bits (no atomics).  No
    autograd (the outputs are detached), no device->host read; the inputs need not be contiguous or float32 (converted as
    `splat_loss` converts them).  GPU tensors only.  LPIPS is not computed: it needs pretrained network weights.
    `exposure` (B, 3, 4): the metrics of the compensated render (`splat_loss`), compensated first and clamped after — the clamp
    applies to y; three channels only.  None (the default) takes the plain kernel."""
    if exposure is not None:
        a, b, e = _check_exposure("image_metrics with an exposure", images, targets, exposure)
        bsz, _, h, w = a.shape
        lib = _lib.load()
        with torch.cuda.device(a.device):
            stream = torch.cuda.current_stream(a.device).cuda_stream
            partial = torch.empty(lib.gcp_ssim_blocks(bsz * 3, h, w), 3, dtype=torch.float32, device=a.device)
            out = torch.empty(bsz, 3, dtype=torch.float64, device=a.device)
            _lib.check(lib.gcp_image_metrics_exposure(a.data_ptr(), b.data_ptr(), e.data_ptr(), bsz, h, w, _host_window(11, 1.5),
                                                      (0.01 * max_val) ** 2, (0.03 * max_val) ** 2, _lib.METRICS_CLAMP if clamp else 0,
                                                      partial.data_ptr(), out.data_ptr(), stream), "gcp_image_metrics_exposure")
        mse, l1, ssim = out.t().contiguous().unbind(dim=0)
        return ImageMetrics(mse, l1, ssim, psnr_from_mse(mse, max_val))
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
