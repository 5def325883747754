"""Mip-Splatting's 3-D smoothing filter (Yu et al., CVPR 2024) on the kernels of csrc/gcp_filter3d.hip: the highest rate at
which a training camera samples each Gaussian (`sampling_rate`), the filter size it gives (`filter_from_rate`) and the
differentiable stage in front of the projection that widens every Gaussian by it and scales its opacity so that it keeps its
mass (`apply_filter`).  What belongs to the model — when the filter is computed, when it goes stale, what is saved — stays in
`GS_model_with_param` (`filter_3d=True`, `update_filter_3d`).  GPU float32 tensors only: there is no CPU path."""
import torch

from . import _lib


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def sampling_rate(mean, P, K, wh, near=0.2, margin=0.15):
    """rate float32 (N,): per Gaussian the largest max(fx, fy) / depth over the cameras that SEE it — depth t.z > `near` and the
    projected centre inside the image widened by `margin` of its size on every side (Mip-Splatting's 0.2 and 0.15) — and 0
    where no camera does (gcp_filter3d_rate).  mean (N, 3), P (C, 3, 4) world->camera, K (C, 3, 3) (the skew is ignored),
    wh (C, 2) integers: pass ALL training cameras.  One kernel, nothing read back; C == 0 gives zeros."""
    if not (mean.is_cuda and P.is_cuda and K.is_cuda):
        raise RuntimeError("the 3-D filter's sampling rate is a HIP kernel: tensors must live on the GPU (no CPU path)")
    if any(t.dtype != torch.float32 for t in (mean, P, K)):
        raise RuntimeError("sampling_rate expects float32 mean, P and K")
    n, c = mean.shape[0], P.shape[0]
    wh = torch.as_tensor(wh)
    if tuple(mean.shape) != (n, 3) or tuple(P.shape) != (c, 3, 4) or tuple(K.shape) != (c, 3, 3) or tuple(wh.shape) != (c, 2):
        raise RuntimeError("sampling_rate expects mean (N, 3), P (C, 3, 4), K (C, 3, 3) and wh (C, 2)")
    dev = mean.device
    mean, P, K = (t.detach().contiguous() for t in (mean, P, K))
    wh = wh.to(device=dev, dtype=torch.int32).contiguous()
    rate = torch.zeros(n, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gcp_filter3d_rate(mean.data_ptr(), P.data_ptr(), K.data_ptr(), wh.data_ptr(), n, c, float(near), float(margin),
                                                 rate.data_ptr(), _stream(dev)), "gcp_filter3d_rate")
    return rate


def filter_from_rate(rate, variance=0.2):
    """phi (N,): sqrt(variance) / rate where rate > 0; the rows no camera sees get the largest phi among the seen ones (that of
    the lowest seen rate, as the published code does); all zeros when no row is seen.  variance = 0.2 is the published value.
    Device-side torch ops only: nothing is read back, so it can be captured."""
    seen = rate > 0
    lowest = torch.where(seen, rate, torch.full_like(rate, float("inf"))).amin() if rate.numel() else rate.new_zeros(())
    # one float32 division per row (a Python scalar over a tensor would be reciprocal-then-multiply); lowest == inf where
    # nothing is seen: phi = 0
    return torch.full_like(rate, float(variance) ** 0.5) / torch.where(seen, rate, lowest)


class _ApplyFilter(torch.autograd.Function):
    """(variance_scale (N, 3), opacity (N, 1) or (N,), filter (N,)) -> (variance_scale', opacity' (N, 1)) on gcp_filter3d_apply;
    backward = gcp_filter3d_apply_backward from the saved INPUTS (every intermediate is recomputed); the filter gets no gradient."""

    @staticmethod
    def forward(ctx, variance_scale, opacity, filter):
        tensors = (variance_scale, opacity, filter)
        if not all(t.is_cuda for t in tensors):
            raise RuntimeError("the 3-D filter is a HIP kernel: tensors must live on the GPU (no CPU path)")
        n, dev = variance_scale.shape[0], variance_scale.device
        if any(t.dtype != torch.float32 or t.device != dev for t in tensors):
            raise RuntimeError("apply_filter expects float32 tensors on one device")
        if tuple(variance_scale.shape) != (n, 3) or opacity.numel() != n or tuple(filter.shape) != (n,):
            raise RuntimeError(f"apply_filter expects variance_scale (N, 3), opacity (N, 1) and filter (N,), got {tuple(variance_scale.shape)}, "
                               f"{tuple(opacity.shape)} and {tuple(filter.shape)}")
        v, x, phi = (t.detach().contiguous() for t in tensors)
        v_out, x_out = torch.empty_like(v), torch.empty((n, 1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().gcp_filter3d_apply(v.data_ptr(), x.data_ptr(), phi.data_ptr(), n, v_out.data_ptr(), x_out.data_ptr(),
                                                      _stream(dev)), "gcp_filter3d_apply")
        ctx.save_for_backward(v, x, phi)
        ctx.opacity_shape = opacity.shape
        return v_out, x_out

    @staticmethod
    def backward(ctx, g_v_out, g_x_out):
        v, x, phi = ctx.saved_tensors
        n, dev = v.shape[0], v.device
        g_v_out, g_x_out = g_v_out.contiguous().float(), g_x_out.contiguous().float()
        g_v, g_x = torch.empty_like(v), torch.empty_like(x)  # every row is written
        with torch.cuda.device(dev):
            _lib.check(_lib.load().gcp_filter3d_apply_backward(v.data_ptr(), x.data_ptr(), phi.data_ptr(), g_v_out.data_ptr(), g_x_out.data_ptr(),
                                                               n, g_v.data_ptr(), g_x.data_ptr(), _stream(dev)), "gcp_filter3d_apply_backward")
        return g_v, g_x.reshape(ctx.opacity_shape), None


def apply_filter(variance_scale, opacity, filter):
    """The 3-D smoothing filter as a differentiable stage: (variance_scale (N, 3) log, opacity (N, 1) logit, filter (N,) = phi >= 0)
    -> (variance_scale', opacity' (N, 1)) with exp(2 variance_scale') = exp(2 variance_scale) + phi^2 per axis and
    sigmoid(opacity') = sigmoid(opacity) sqrt(prod s^2 / prod s'^2): the Gaussian convolved with an isotropic one of standard
    deviation phi, its mass kept.  A row with phi = 0 comes back bit for bit, values and gradients.  The gradients reach
    `variance_scale` and `opacity`; `filter` gets none.  Two HIP kernels (forward, backward), fixed shapes, nothing read back:
    it can be captured into a graph.  GPU float32 only; CPU tensors raise."""
    return _ApplyFilter.apply(variance_scale, opacity, filter)
