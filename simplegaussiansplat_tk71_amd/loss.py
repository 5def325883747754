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


def _inputs(what, images, targets, exposure=None, kernel=None):
    """The refusals of every path, before the library is touched -> (a, b, e): contiguous float32, detached; e is None
    without an exposure.  `kernel`: what the no-CPU-path refusal calls the operation (default: `what`)."""
    no_cpu = f"{kernel or what} is a HIP kernel: tensors must live on the GPU (no CPU path)"
    if exposure is None and not images.is_cuda:
        raise RuntimeError(no_cpu)
    if images.shape != targets.shape or images.dim() != 4:
        raise RuntimeError(f"{what} expects two (B, C, H, W) tensors of one shape")
    if exposure is not None:
        if images.shape[1] != 3:
            raise RuntimeError(f"{what}: an exposure is a colour affine of three channels, got C = {images.shape[1]}")
        if not torch.is_tensor(exposure) or tuple(exposure.shape) != (images.shape[0], 3, 4):
            raise RuntimeError(f"{what}: exposure must be a (B, 3, 4) tensor with B = {images.shape[0]}, "
                               f"got {tuple(exposure.shape) if torch.is_tensor(exposure) else type(exposure).__name__}")
        if not images.is_cuda:
            raise RuntimeError(no_cpu)
        if exposure.device != images.device or targets.device != images.device:
            raise RuntimeError(f"{what}: images, targets and exposure must live on one device")
    return tuple(None if t is None else t.detach().contiguous().float() for t in (images, targets, exposure))


def _pointers(*tensors):
    return tuple(None if t is None else t.data_ptr() for t in tensors)


def _forward_call(entry, a, b, e, plain_batch, max_val, width, tail):
    """One launch of the forward family (`entry`, with `_exposure` appended when e is given) -> its (blocks, width) partials.
    `plain_batch`: how the plain entry point counts the batch (with an exposure: the matrices, then the images);
    `tail(partial)`: the arguments between c2 and the stream."""
    bsz, ch, h, w = a.shape
    lib = _lib.load()
    name = entry if e is None else entry + "_exposure"
    batch = plain_batch if e is None else (e.data_ptr(), bsz)
    with torch.cuda.device(a.device):
        stream = torch.cuda.current_stream(a.device).cuda_stream
        partial = torch.empty(lib.gcp_ssim_blocks(bsz * ch, h, w), width, dtype=torch.float32, device=a.device)
        _lib.check(getattr(lib, name)(a.data_ptr(), b.data_ptr(), *batch, h, w, _host_window(11, 1.5), (0.01 * max_val) ** 2,
                                      (0.03 * max_val) ** 2, *tail(partial), stream), name)
    return partial


def _loss_forward(ctx, images, a, b, e, need_grad, lamda, max_val):
    """The forward of both Functions: the loss, with (a, b[, e], the three maps if a gradient is needed) saved on ctx."""
    maps = [torch.empty_like(a) if need_grad else None for _ in range(3)]
    partial = _forward_call("gcp_ssim_l1_forward", a, b, e, (a.shape[0] * a.shape[1],), max_val, 2,
                            lambda partial: _pointers(*maps, partial))
    sums = partial.double().sum(dim=0) / a.numel()  # [mean SSIM, mean |a - b|] (of y with an exposure)
    ctx.save_for_backward(a, b, *([] if e is None else [e]), *(maps if need_grad else []))
    ctx.lamda, ctx.dtype = lamda, images.dtype
    return ((1 - lamda) * sums[1] + lamda * (1 - sums[0])).to(images.dtype)


def _loss_backward(ctx, grad_out, want_x=True, want_e=False):
    """The backward of both Functions -> (dL/dimages, dL/dexposure) in float32, None where not wanted."""
    a, b, *e, m1, m2, m3 = ctx.saved_tensors
    n = a.numel()
    scales = (grad_out.reshape(1).float() * torch.tensor([-ctx.lamda / n, (1 - ctx.lamda) / n], device=a.device)).contiguous()
    bsz, ch, h, w = a.shape
    lib = _lib.load()
    grad = torch.empty_like(a) if want_x else None
    grad_e = torch.empty_like(e[0]) if want_e else None  # every entry is written
    with torch.cuda.device(a.device):
        stream = torch.cuda.current_stream(a.device).cuda_stream
        if e:
            partial_e = torch.empty(lib.gcp_exposure_blocks(bsz, h, w), 12, dtype=torch.float32, device=a.device) if want_e else None
            _lib.check(lib.gcp_ssim_l1_backward_exposure(*_pointers(a, b, e[0], m1, m2, m3), bsz, h, w, _host_window(11, 1.5),
                                                         scales.data_ptr(), *_pointers(grad, partial_e, grad_e), stream),
                       "gcp_ssim_l1_backward_exposure")
        else:
            _lib.check(lib.gcp_ssim_l1_backward(*_pointers(a, b, m1, m2, m3), bsz * ch, h, w, _host_window(11, 1.5), scales.data_ptr(),
                                                grad.data_ptr(), stream), "gcp_ssim_l1_backward")
    return grad, grad_e


class _SplatLoss(torch.autograd.Function):
    """(1 - lambda) L1 + lambda (1 - mean SSIM) in one HIP kernel per direction (csrc/gcp_loss.hip); differentiable in
    the first image only (the second is the target photograph)."""

    @staticmethod
    def forward(ctx, images, targets, lamda, max_val):
        a, b, _ = _inputs("splat_loss", images, targets, kernel="the fused loss")
        return _loss_forward(ctx, images, a, b, None, images.requires_grad, lamda, max_val)

    @staticmethod
    def backward(ctx, grad_out):
        return _loss_backward(ctx, grad_out)[0].to(ctx.dtype), None, None, None


class _SplatLossExposure(torch.autograd.Function):
    """`_SplatLoss` of the compensated render y = E[:, :, :3] x + E[:, :, 3], differentiable in the render and in the
    exposure; y is formed inside the kernels (csrc/gcp_loss.hip: k_ssim_l1_fwd_exposure, k_ssim_l1_bwd_exposure,
    k_exposure_fold) and never stored."""

    @staticmethod
    def forward(ctx, images, targets, exposure, lamda, max_val):
        a, b, e = _inputs("splat_loss with an exposure", images, targets, exposure)
        ctx.e_dtype = exposure.dtype
        return _loss_forward(ctx, images, a, b, e, images.requires_grad or exposure.requires_grad, lamda, max_val)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        want_x, want_e = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
        grad, grad_e = _loss_backward(ctx, grad_out, want_x, want_e)
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
    _inputs("splat_loss with an exposure", images, targets, exposure)
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
    a, b, e = _inputs("image_metrics" if exposure is None else "image_metrics with an exposure", images, targets, exposure)
    out = torch.empty(a.shape[0], 3, dtype=torch.float64, device=a.device)
    _forward_call("gcp_image_metrics", a, b, e, tuple(a.shape[:2]), max_val, 3,
                  lambda partial: (_lib.METRICS_CLAMP if clamp else 0, partial.data_ptr(), out.data_ptr()))
    mse, l1, ssim = out.t().contiguous().unbind(dim=0)
    return ImageMetrics(mse, l1, ssim, psnr_from_mse(mse, max_val))
