"""Density control on the device: the screen-space statistic and the kernel sequence of the one-pass split / clone / prune
(csrc/gcp_densify.hip), and the MCMC strategy's relocation pass and position noise (csrc/gcp_mcmc.hip), the row gather of a prune by mask (`keep_rows`).
What belongs to the model — parameters, optimiser, statistics — stays in `GS_model_with_param.densify_and_prune_device`,
`relocate_and_grow_device` and `prune_rows`."""
import torch

from . import _lib

DENSIFY_ON = ("position", "screen")
# what densify_on="screen" accumulates per view: the norm of the centre's gradient as the blend backward returns it — a signed
# sum over the splat's pixels — or of the per-pixel absolute values summed per component (AbsGS; csrc/gcp_absgrad.hip)
SCREEN_GRADS = ("signed", "abs")


def accumulate_screen_grads(grad_xy, index, scale, norm_acc, view_count, validate=False):
    """The screen-space densification statistic of one camera (gcp_densify_accumulate, csrc/gcp_densify.hip), in place:
    norm_acc[index[i]] += |grad_xy[i] * scale|, view_count[index[i]] += 1.  grad_xy float32 (m, 2): the loss's gradient with
    respect to the splat centres in list order; index int64 (m,): the list's Gaussian ids, each at most once (what
    `camera_inputs` returns as "index"); scale = (sx, sy); norm_acc float32 (N,), view_count int32 (N,).  GPU tensors only.
    An id outside [0, N) is never written through; validate=True reads the number of such ids back first (one host read)
    and raises, with nothing accumulated."""
    if not (grad_xy.is_cuda and index.is_cuda and norm_acc.is_cuda and view_count.is_cuda):
        raise RuntimeError("the densification statistic is a HIP kernel: tensors must live on the GPU (no CPU path)")
    m, n = index.numel(), norm_acc.numel()
    if index.dtype != torch.int64 or norm_acc.dtype != torch.float32 or view_count.dtype != torch.int32:
        raise RuntimeError("accumulate_screen_grads expects int64 ids, a float32 norm and an int32 view count")
    if tuple(grad_xy.shape) != (m, 2) or view_count.numel() != n or not (norm_acc.is_contiguous() and view_count.is_contiguous()):
        raise RuntimeError("accumulate_screen_grads expects grad_xy (m, 2), index (m,) and contiguous norm_acc, view_count of one length")
    grad_xy, index = grad_xy.detach().float().contiguous(), index.contiguous()
    lib = _lib.load()
    with torch.cuda.device(norm_acc.device):
        stream = torch.cuda.current_stream(norm_acc.device).cuda_stream
        if validate:
            bad = torch.zeros(1, dtype=torch.int32, device=norm_acc.device)
            _lib.check(lib.gcp_densify_accumulate(None, index.data_ptr(), m, 1.0, 1.0, None, None, n, bad.data_ptr(), stream),
                       "gcp_densify_accumulate")
            if int(bad):
                raise RuntimeError(f"accumulate_screen_grads: {int(bad)} of {m} ids lie outside [0, {n})")
        _lib.check(lib.gcp_densify_accumulate(grad_xy.data_ptr(), index.data_ptr(), m, float(scale[0]), float(scale[1]), norm_acc.data_ptr(),
                                              view_count.data_ptr(), n, None, stream), "gcp_densify_accumulate")


def densify_rows(params, moments, norm, views, grad_threshold, split_scale, prune_scale, min_opacity, n_split, seed):
    """The kernel sequence of `GS_model_with_param.densify_and_prune_device`, whose docstring states the rule: plan (an action
    and a row count per Gaussian, their offsets), the one 4-byte device->host read of the new row count m, fill (source row
    and kind of every new row), the row gathers, split (the children's samples over the gathered mean and scale).
    params: {"mean", "variance_q", "variance_scale", "opacity", "color"} -> contiguous float32 (n, ...); moments: name ->
    (exp_avg, exp_avg_sq) of the parameters that have an optimiser state; norm float32 (n,), views int32 (n,): the statistic,
    contiguous; a Gaussian is hot at norm / max(views, 1) >= grad_threshold, splits above split_scale, and a row is dropped
    above prune_scale or below min_opacity; seed: 64 bits.
    -> (new params by name, new (exp_avg, exp_avg_sq) by name — fresh rows 0.0 —, m)"""
    dev, n = params["mean"].device, params["mean"].shape[0]
    lib = _lib.load()
    count, offset = (torch.empty(k, dtype=torch.int32, device=dev) for k in (n, n + 1))
    action = torch.empty(n, dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.gcp_densify_plan_workspace_bytes(n), dtype=torch.uint8, device=dev)
    seed = int(seed) & (2 ** 64 - 1)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.gcp_densify_plan(norm.data_ptr(), views.data_ptr(), params["variance_scale"].data_ptr(), params["opacity"].data_ptr(), n,
                                        float(grad_threshold), float(split_scale), float(prune_scale), float(min_opacity), int(n_split),
                                        count.data_ptr(), action.data_ptr(), offset.data_ptr(), ws.data_ptr(), ws.numel(), stream),
                   "gcp_densify_plan")
        m = int(offset[n])  # the one device->host read
        src_row = torch.empty(m, dtype=torch.int32, device=dev)
        kind = torch.empty(m, dtype=torch.uint8, device=dev)
        _lib.check(lib.gcp_densify_fill(action.data_ptr(), offset.data_ptr(), n, m, src_row.data_ptr(), kind.data_ptr(), stream),
                   "gcp_densify_fill")

        def rows(t, mode):
            out = torch.empty((m, *t.shape[1:]), dtype=torch.float32, device=dev)
            _lib.check(lib.gcp_densify_rows(t.data_ptr(), n, src_row.data_ptr(), kind.data_ptr(), m, t[0].numel() if n else 0, mode,
                                            out.data_ptr(), stream), "gcp_densify_rows")
            return out

        new = {k: rows(t, 0) for k, t in params.items()}
        _lib.check(lib.gcp_densify_split(params["mean"].data_ptr(), params["variance_q"].data_ptr(), params["variance_scale"].data_ptr(),
                                         src_row.data_ptr(), kind.data_ptr(), offset.data_ptr(), n, m, int(n_split), seed & 0xFFFFFFFF,
                                         seed >> 32, new["mean"].data_ptr(), new["variance_scale"].data_ptr(), stream),
                   "gcp_densify_split")
        new_moments = {k: tuple(rows(t.contiguous(), 1) for t in pair) for k, pair in moments.items()}
    return new, new_moments, m


def mcmc_weight_levels(n):
    """W of gcp_mcmc_weights: the largest power of two <= 2^16 with n * W <= 2^31 - 1 (the prefix sum is int32)."""
    w = 1 << 16
    while w > 1 and n * w > 2 ** 31 - 1:
        w >>= 1
    return w


def mcmc_noise(mean, variance_q, variance_scale, opacity, amount, seed, k=100.0, o0=0.005):
    """The MCMC strategy's position noise (gcp_mcmc_noise, csrc/gcp_mcmc.hip), in place on `mean` float32 (N, 3):
    mean += amount * gate * R (s^2 (.) (R^T z)), gate = 1 / (1 + exp(-k (o0 - sigmoid(opacity)))), R from variance_q (x, y, z, w)
    normalised, s = exp(variance_scale), z standard normal from Philox4x32-10 keyed by `seed` (64 bits), counter (i, 0, 0, 1).
    Contiguous float32 GPU tensors only."""
    tensors = (mean, variance_q, variance_scale, opacity)
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError("the position noise is a HIP kernel: tensors must live on the GPU (no CPU path)")
    n = mean.shape[0]
    if any(t.dtype != torch.float32 or not t.is_contiguous() for t in tensors):
        raise RuntimeError("mcmc_noise expects contiguous float32 tensors")
    if tuple(mean.shape) != (n, 3) or tuple(variance_q.shape) != (n, 4) or tuple(variance_scale.shape) != (n, 3) or opacity.numel() != n:
        raise RuntimeError("mcmc_noise expects mean (N, 3), variance_q (N, 4), variance_scale (N, 3) and opacity (N, 1)")
    seed = int(seed) & (2 ** 64 - 1)
    with torch.cuda.device(mean.device):
        _lib.check(_lib.load().gcp_mcmc_noise(mean.data_ptr(), variance_q.data_ptr(), variance_scale.data_ptr(), opacity.data_ptr(), n,
                                              float(amount), float(k), float(o0), seed & 0xFFFFFFFF, seed >> 32,
                                              torch.cuda.current_stream(mean.device).cuda_stream), "gcp_mcmc_noise")


def mcmc_rows(params, moments, n_out, min_opacity, seed):
    """The kernel sequence of `GS_model_with_param.relocate_and_grow_device`, whose docstring states the rule: weights (an
    integer weight per Gaussian, 0 when dead, and their prefix sum), draw (every new row and every dead row draws a live
    source; how often each source was drawn; survivor or fresh), the row gathers of `densify_rows`, values (opacity and
    scale of the sources that were drawn and of their copies).  No device->host read anywhere: n_out is the caller's.
    params, moments: as `densify_rows`; n_out >= n rows come out; a Gaussian is dead at !(sigmoid(opacity) > min_opacity);
    seed: 64 bits.
    -> (new params by name, new (exp_avg, exp_avg_sq) by name — rows that were drawn from, or written by a draw, 0.0 —,
        {"src_row" int32 (n_out,), "kind" uint8 (n_out,), "times" int32 (n,), "cum" int32 (n + 1,), "weight" int32 (n,)})"""
    if not all(t.is_cuda for t in params.values()):
        raise RuntimeError("the relocation pass is a set of HIP kernels: tensors must live on the GPU (no CPU path)")
    dev, n, m = params["mean"].device, params["mean"].shape[0], int(n_out)
    if m < n or (n == 0 and m > 0):
        raise RuntimeError(f"mcmc_rows: {n} rows cannot become {m} (rows are never dropped, and nothing grows out of nothing)")
    lib = _lib.load()
    weight, times, src_row = (torch.empty(k, dtype=torch.int32, device=dev) for k in (n, n, m))
    cum = torch.zeros(n + 1, dtype=torch.int32, device=dev)  # zeros: with n == 0 the entry points touch nothing
    kind = torch.empty(m, dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.gcp_mcmc_workspace_bytes(n), dtype=torch.uint8, device=dev)
    seed = int(seed) & (2 ** 64 - 1)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.gcp_mcmc_weights(params["opacity"].data_ptr(), n, float(min_opacity), mcmc_weight_levels(n), weight.data_ptr(),
                                        cum.data_ptr(), ws.data_ptr(), ws.numel(), stream), "gcp_mcmc_weights")
        _lib.check(lib.gcp_mcmc_draw(cum.data_ptr(), n, m, seed & 0xFFFFFFFF, seed >> 32, src_row.data_ptr(), times.data_ptr(),
                                     kind.data_ptr(), stream), "gcp_mcmc_draw")

        def rows(t, mode):
            out = torch.empty((m, *t.shape[1:]), dtype=torch.float32, device=dev)
            _lib.check(lib.gcp_densify_rows(t.data_ptr(), n, src_row.data_ptr(), kind.data_ptr(), m, t[0].numel() if n else 0, mode,
                                            out.data_ptr(), stream), "gcp_densify_rows")
            return out

        new = {k: rows(t, 0) for k, t in params.items()}
        _lib.check(lib.gcp_mcmc_values(params["opacity"].data_ptr(), params["variance_scale"].data_ptr(), src_row.data_ptr(), times.data_ptr(),
                                       n, m, float(min_opacity), new["opacity"].data_ptr(), new["variance_scale"].data_ptr(), stream),
                   "gcp_mcmc_values")
        new_moments = {k: tuple(rows(t.contiguous(), 1) for t in pair) for k, pair in moments.items()}
    return new, new_moments, {"src_row": src_row, "kind": kind, "times": times, "cum": cum, "weight": weight}


def keep_rows(params, moments, keep):
    """The kernel sequence of `GS_model_with_param.prune_rows`: the kept rows' indices (`keep.nonzero()`, whose size is the one
    device->host read), then the row gathers of `densify_rows` with that list as the source rows and every row a survivor
    (kind 0), so parameters and Adam's moments are both carried bit for bit, in order.
    params, moments: as `densify_rows`; keep: bool (n,) on the parameters' device.  An all-false `keep` raises before anything
    is gathered.  -> (new params by name, new (exp_avg, exp_avg_sq) by name, m)"""
    if not all(t.is_cuda for t in params.values()):
        raise RuntimeError("pruning on the device is a set of HIP kernels: tensors must live on the GPU (no CPU path)")
    dev, n = params["mean"].device, params["mean"].shape[0]
    if not (isinstance(keep, torch.Tensor) and keep.dtype == torch.bool and tuple(keep.shape) == (n,) and keep.device == dev):
        raise RuntimeError(f"keep: expected a bool tensor of shape ({n},) on {dev}")
    src_row = keep.nonzero().flatten().to(torch.int32)  # the one device->host read: its length
    m = src_row.numel()
    if m == 0:
        raise RuntimeError("keep: no row is kept (an empty scene cannot be rendered or trained)")
    kind = torch.zeros(m, dtype=torch.uint8, device=dev)  # survivors all
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream

        def rows(t, mode):
            out = torch.empty((m, *t.shape[1:]), dtype=torch.float32, device=dev)
            _lib.check(lib.gcp_densify_rows(t.data_ptr(), n, src_row.data_ptr(), kind.data_ptr(), m, t[0].numel(), mode, out.data_ptr(),
                                            stream), "gcp_densify_rows")
            return out

        new = {k: rows(t, 0) for k, t in params.items()}
        new_moments = {k: tuple(rows(t.contiguous(), 1) for t in pair) for k, pair in moments.items()}
    return new, new_moments, m
