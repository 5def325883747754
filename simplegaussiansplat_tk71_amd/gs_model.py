"""Caller of the hot path: 3-D Gaussians + cameras -> the inputs of the rasterise-and-blend Function -> images.

Mirrors the reference's model class (reference: gs_model.py:123-460, `GS_model_with_param`): same parameter set
(mean, variance_q, variance_scale, opacity, color), same `forward(P, K, wh, image_sample)` return value
`[images, image_sample, grad_iter]`, same per-parameter Adam learning rates, densify / prune / opacity reset.
Row f4 of SURVEY.md §8: this is caller integration, PyTorch on the GPU around the HIP Function — not a kernel.

This module holds the model and dataset classes and the reference's small helpers.  What the model calls lives next to
it and is re-exported from here under the names it always had: the camera projection (projection.py: `camera_inputs`),
the fused loss (loss.py: `splat_loss`), the optimiser step (optim.py: `HipAdam`) and the kernels of the density control
(density.py: `accumulate_screen_grads`), the 3-D smoothing filter (filter3d.py: `sampling_rate`, `filter_from_rate`,
`apply_filter`), the lens distortion of the photographs (lens.py: `Lens`, `lens_from_colmap`, `fit_pinhole`, `undistort`) and the
normals (normals.py: `gaussian_normals`, `normal_consistency`, `normal_consistency_map`, `depth_normals`, `median_as_depth`) and the mesh extraction
(mesh.py: `TSDFVolume`, `extract_surface`, `face_components`, `clean_mesh`, `vertex_normals`) and the exact nearest neighbours for the initial scales (knn.py: `nearest_neighbours`,
`neighbour_scale`).
Differences from the reference's class, all deliberate (those of the projection: projection.py):
  * images are permuted to (B, 3, H, W); the reference `reshape`s (H, W, 3) memory into (3, H, W), scrambling
    channels (gs_model.py:454) — `reference_layout=True` reproduces that;
  * one Function call per camera, never chunked (nothing of pair-list size exists here; gs_model.py:428);
  * tensors live on the parameters' device instead of a hard-coded "cuda";
  * projection and loss have no CPU path (CPU tensors raise).
"""
import math

import torch

from . import density
from .cuda_kernel import absgrad_buffer as _absgrad_buffer
from .cuda_kernel import contribution as _camera_contribution
from .cuda_kernel import custom_autograd_grouped_cumprod, render
from .cuda_kernel import paint as _paint
from .cuda_kernel import paint_maps as _paint_maps
from .density import DENSIFY_ON, SCREEN_GRADS, accumulate_screen_grads
from .exposure import CameraExposure
from .filter3d import apply_filter, filter_from_rate, sampling_rate
from .knn import nearest_neighbours, neighbour_scale
from .lens import Lens, fit_pinhole, lens_from_colmap, undistort
from .loss import ImageMetrics, apply_exposure, image_metrics, psnr_from_mse, splat_loss
from .mesh import TSDFVolume, clean_mesh, extract_surface, face_components, vertex_normals
from .normals import depth_normals, gaussian_normals, median_as_depth, normal_consistency, normal_consistency_map
from .optim import HipAdam
from .projection import CENTRES, SH_FRAMES, _box_clamp, camera_inputs, splat_options  # noqa: F401  (re-exported)

PARAM_NAMES = ("mean", "variance_q", "variance_scale", "opacity", "color")  # the per-Gaussian parameters, in optimiser order
ADAM_MODES = ("tensor", "fused", "sparse")

__all__ = [
    "CameraExposure",
    "GS_dataset",
    "GS_model_with_param",
    "HipAdam",
    "ImageMetrics",
    "Lens",
    "TSDFVolume",
    "accumulate_screen_grads",
    "allreduce_contribution",
    "apply_exposure",
    "apply_filter",
    "camera_inputs",
    "clean_mesh",
    "depth_normals",
    "extract_surface",
    "face_components",
    "filter_from_rate",
    "fit_pinhole",
    "gather_metrics",
    "gaussian_normals",
    "image_metrics",
    "lens_from_colmap",
    "qvec_to_rotmat_batch",
    "get_expon_lr_func",
    "mean_neighbour_distance",
    "median_as_depth",
    "nearest_neighbours",
    "neighbour_scale",
    "normal_consistency",
    "normal_consistency_map",
    "sampling_rate",
    "splat_loss",
    "split_cameras",
    "undistort",
    "vertex_normals",
]


def qvec_to_rotmat_batch(q):
    """(N, 4) unit quaternions in (x, y, z, w) order -> (N, 3, 3) (reference: uitility.py:231-254)."""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    r0 = torch.stack([1 - 2 * (y**2 + z**2), 2 * (x * y - w * z), 2 * (x * z + w * y)], dim=1)
    r1 = torch.stack([2 * (x * y + w * z), 1 - 2 * (x**2 + z**2), 2 * (y * z - w * x)], dim=1)
    r2 = torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x**2 + y**2)], dim=1)
    return torch.stack([r0, r1, r2], dim=1)


def get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """Log-linear learning-rate decay with an optional eased start (reference: uitility.py:573-607)."""

    def helper(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        delay = 1.0
        if lr_delay_steps > 0:
            delay = lr_delay_mult + (1 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0), 1))
        t = min(max(step / max_steps, 0.0), 1.0)
        return delay * math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)

    return helper


def mean_neighbour_distance(n, cloud, batch_size=2000):
    """Mean distance to the n nearest points (self included), repeated on 3 axes: the initial scale
    (reference: uitility.py:68-78, `kyori2`)."""
    out = torch.zeros((cloud.shape[0], 1), device=cloud.device, dtype=cloud.dtype)
    for i in range(0, cloud.shape[0], batch_size):
        d = torch.cdist(cloud[i:i + batch_size], cloud)
        out[i:i + batch_size] = torch.topk(d, min(n, d.shape[1]), dim=1, largest=False).values.mean(dim=1, keepdim=True)
    return out.repeat(1, 3)


def allreduce_contribution(stats, group=None):
    """The triple of `GS_model_with_param.contribution` over the ranks, in place, when every rank has measured its share of
    the cameras: w_max by MAX, w_sum and views by SUM, so every rank prunes the same rows.  Under backend "gloo" through the
    host, as `GS_model_with_param.allreduce_density_stats`.  Returns `stats`."""
    import torch.distributed as dist

    w_max, w_sum, views = stats
    for t, op in ((w_max, dist.ReduceOp.MAX), (w_sum, dist.ReduceOp.SUM), (views, dist.ReduceOp.SUM)):
        if t.is_cuda and dist.get_backend(group) == "gloo":
            host = t.cpu()
            dist.all_reduce(host, op=op, group=group)
            t.copy_(host)
        else:
            dist.all_reduce(t, op=op, group=group)
    return stats


def split_cameras(names, test_every=8):
    """(train_idx, test_idx): index lists into `names`.  The cameras are sorted by name and position i of that order is held
    out for testing where i % test_every == 0 — the `llffhold` convention of Mip-NeRF 360 and 3DGS, so the numbers compare
    with published ones.  Both lists are in sorted-name order.  test_every=0: everything trains, nothing is held out."""
    test_every = int(test_every)
    if test_every < 0:
        raise ValueError(f"test_every: >= 0, got {test_every}")
    order = sorted(range(len(names)), key=lambda i: names[i])
    if test_every == 0:
        return order, []
    return [j for i, j in enumerate(order) if i % test_every], [j for i, j in enumerate(order) if i % test_every == 0]


def gather_metrics(metrics, index, total, group=None):
    """Every rank has measured its share of `total` images (`metrics`: the ImageMetrics of the images `index`, a list or
    int64 tensor of positions in 0..total-1; both may be empty) -> the ImageMetrics of all of them on every rank: the share is
    scattered into zero vectors of length `total` and these are all-reduced with SUM — under backend "gloo" through the host,
    as `allreduce_contribution`.  Every image is measured by exactly one rank, so a sum adds zeros to its value: the result
    is the single-rank one bit for bit.  `psnr` is recomputed from the summed `mse` (max_val 1)."""
    import torch.distributed as dist

    dev = metrics.mse.device
    index = torch.as_tensor(index, dtype=torch.int64, device=dev)
    full = torch.zeros(3, int(total), dtype=torch.float64, device=dev)
    if index.numel():
        full[:, index] = torch.stack((metrics.mse, metrics.l1, metrics.ssim)).to(torch.float64)
    if full.is_cuda and dist.get_backend(group) == "gloo":
        host = full.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        full.copy_(host)
    else:
        dist.all_reduce(full, op=dist.ReduceOp.SUM, group=group)
    return ImageMetrics(full[0], full[1], full[2], psnr_from_mse(full[0]))


class GS_dataset(torch.utils.data.Dataset):
    """Cameras and their image names (reference: gs_model.py:13-30)."""

    def __init__(self, P, K, wh, image_sample):
        self.P, self.K, self.wh, self.image_sample = P, K, wh, image_sample

    def __len__(self):
        return len(self.P)

    def __getitem__(self, idx):
        return [self.P[idx], self.K[idx], self.wh[idx], self.image_sample[idx]]

    def get_camera_extent(self, reference_translation=False):
        """Largest distance of a camera from the mean camera position.  The reference measures it on the translation
        column of [R|t] (gs_model.py:23-30) — the world origin in camera coordinates, which is the same point for every
        camera that looks at the origin; the camera centres -R^T t are used here (`reference_translation=True`
        restores the reference's quantity)."""
        t = self.P[:, :, 3]
        if not reference_translation:
            t = -(self.P[:, :, 0:3].transpose(1, 2) @ t[:, :, None]).squeeze(-1)
        return torch.max((t.mean(dim=0)[None] - t).norm(dim=1)).item()


class GS_model_with_param(torch.nn.Module):
    """Trainable scene (reference: gs_model.py:123-460).  Hyper-parameters the reference wraps in two nested
    parameter modules (:76-119) are plain floats here: nothing ever trains them."""

    def __init__(self, mean, variance_q, variance_scale, opacity, grad_delta_upper_limit=1e-12, grad_threshold=0.0004,
                 percent_dense=0.01, prunning_min_opacity=0.005, variance_pixel_tile_max_width=0.04,
                 position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
                 position_lr_max_steps=30_000, feature_lr=0.0025, opacity_lr=0.025, scaling_lr=0.005,
                 rotation_lr=0.001, c_00=1.77, L_max=2, lr=0.1, reference_layout=False, sh_frame="camera",
                 active_sh_degree=None, centres="pixel", cov_dilation=None, clamp_colour=False, densify_on="position",
                 antialias=False, adam="tensor", screen_grad="signed", filter_3d=False):
        """L_max (0..3): the SH degree the colour parameter stores, (N, (L_max+1)^2, 3).  active_sh_degree (default L_max):
        the degree that is evaluated and trained; `oneup_sh_degree()` raises it.  sh_frame, centres, cov_dilation,
        clamp_colour, antialias: see `camera_inputs`; `forward`, `render` and `camera_inputs` of the model project with them.
        antialias scales the opacity the blend sees, not the parameter: pruning (`densify_and_prune`,
        `densify_and_prune_device`) and `reset_opacity` keep testing the raw sigmoid(opacity), and `save_ply` stores it.
        densify_on: the statistic `densify_and_prune_device` decides on.  "position" (the default, the reference's): the norm
        of the 3-D positional gradient per step, kept by `param_iter_update`.  "screen" (needs centres="subpixel"): the norm
        of the loss's gradient with respect to the 2-D splat centre, per VIEW, scaled by (W/2, H/2) — the NDC unit other
        3DGS trainers threshold in; `forward` and `render` collect it during `backward` in `screen_grads_norm` /
        `screen_grads_views`.  `grad_threshold` has NOT been tuned for that statistic here: no full-length run on real poses
        exists (the reference's checkout has no images.bin), the default is the reference's value for its own statistic.
        screen_grad: what densify_on="screen" takes the norm of.  "signed" (the default): the centre's gradient as the blend
        backward returns it, a signed sum over the splat's pixels — a large, blurry Gaussian that is too bright on one side and
        too dark on the other cancels there and is never split.  "abs" (needs densify_on="screen"): the per-pixel absolute
        values summed per component (AbsGS; gsplat's absgrad=True; csrc/gcp_absgrad.hip), collected in one [m, 2] buffer per
        drawn camera; the parameters' gradients, and so the optimiser steps, are bit for bit those of "signed".
        `grad_threshold` is not tuned for this statistic here either; it is larger than the signed one by construction, and
        trainers that switch raise their threshold with it (gsplat: 2e-4 -> 8e-4) — a pointer, not a default.
        adam: the optimiser step on the GPU (`HipAdam`).  "tensor" (the default): one kernel per parameter tensor, step counts
        on the host.  "fused": all five tensors in one call, step counts and rates on the device (capturable).  "sparse": the
        fused call with the row mask `train_step(visible)` is given — rows outside it keep parameters and moments, as the
        sparse Adam of other 3DGS trainers; GPU only.
        filter_3d=True: Mip-Splatting's 3-D smoothing filter, the other half of `antialias` (csrc/gcp_filter3d.hip; GPU only).
        `update_filter_3d(P, K, wh)` computes a per-Gaussian filter size from ALL training cameras and keeps it in
        `self.filter_3d` (a plain tensor: no Parameter, not in the optimiser; the option itself is `self.use_filter_3d`); every draw (`forward`, `render`, `evaluate`,
        `contribution`, `camera_inputs`) then projects `apply_filter(variance_scale, opacity, filter_3d)` in place of the raw
        two, and the gradients reach the raw parameters through it.  Like antialias it changes what the blend sees, not the
        parameters: the pruning thresholds, `reset_opacity`, the MCMC weights and noise and the split sizes all keep reading
        the raw values; `save_ply` bakes the filter in by default.  The filter is stale before the first `update_filter_3d` and
        after every pass that changes the row set (`densify_and_prune`, `densify_and_prune_device`, `relocate_and_grow_device`,
        `prune_rows`, `prune_by_contribution`): the next draw raises until `update_filter_3d` has run again — it is never
        carried through a gather, new rows sit at new positions."""
        super().__init__()
        if not isinstance(filter_3d, bool):
            raise ValueError(f"filter_3d: True or False, got {filter_3d!r}")
        self.use_filter_3d, self.filter_3d = filter_3d, None
        if adam not in ADAM_MODES:
            raise ValueError(f"adam: 'tensor', 'fused' or 'sparse', got {adam!r}")
        if adam == "sparse" and not mean.is_cuda:
            raise RuntimeError("adam='sparse' is a HIP kernel: tensors must live on the GPU (CPU models keep torch.optim.Adam)")
        self.adam = adam
        if densify_on not in DENSIFY_ON:
            raise ValueError(f"densify_on: 'position' or 'screen', got {densify_on!r}")
        if screen_grad not in SCREEN_GRADS:
            raise ValueError(f"screen_grad: 'signed' or 'abs', got {screen_grad!r}")
        if screen_grad == "abs" and densify_on != "screen":
            raise ValueError("screen_grad='abs' is a form of the screen-space statistic: it needs densify_on='screen' (and so centres='subpixel')")
        if densify_on == "screen" and centres != "subpixel":
            raise ValueError("densify_on='screen' needs centres='subpixel': with pixel centres the blend has no gradient w.r.t. the centre")
        if not 0 <= L_max <= 3:
            raise ValueError(f"L_max: 0..3, got {L_max}")
        if sh_frame not in SH_FRAMES:
            raise ValueError(f"sh_frame: 'camera' or 'world', got {sh_frame!r}")
        active_sh_degree = L_max if active_sh_degree is None else int(active_sh_degree)
        if not 0 <= active_sh_degree <= L_max:
            raise ValueError(f"active_sh_degree: 0..L_max, got {active_sh_degree}")
        self.grad_delta_upper_limit, self.grad_threshold = grad_delta_upper_limit, grad_threshold
        self.percent_dense, self.prunning_min_opacity = percent_dense, prunning_min_opacity
        self.variance_pixel_tile_max_width = math.log(variance_pixel_tile_max_width / (1 - variance_pixel_tile_max_width))
        self.mean = torch.nn.Parameter(mean)
        self.variance_q = torch.nn.Parameter(variance_q)
        self.variance_scale = torch.nn.Parameter(variance_scale)
        self.opacity = torch.nn.Parameter(opacity)
        color = torch.zeros((mean.size(0), (L_max + 1) ** 2, 3), device=mean.device, dtype=torch.float32)
        color[:, 0, :] = c_00  # mid grey: 0.2821 * 1.77 = 0.5 (:156-158)
        self.color = torch.nn.Parameter(color)
        self.mean_lr_setfunc = get_expon_lr_func(position_lr_init, position_lr_final, lr_delay_steps=0,
                                                 lr_delay_mult=position_lr_delay_mult, max_steps=position_lr_max_steps)
        self.lr = {"mean": self.mean_lr_setfunc(0), "variance_q": rotation_lr, "variance_scale": scaling_lr,
                   "opacity": opacity_lr, "color": feature_lr}
        splat_options(centres, cov_dilation, clamp_colour, antialias)  # validation only: `camera_inputs` forms the record
        self._L_max, self.sh_frame, self.active_sh_degree = L_max, sh_frame, active_sh_degree
        self.centres, self.cov_dilation, self.clamp_colour, self.antialias = centres, cov_dilation, clamp_colour, antialias
        self.reference_layout = reference_layout
        self.densify_on, self.screen_grad = densify_on, screen_grad
        self._zero_density_stats(mean.shape[0])
        self.changing_optimizer()

    # ---- optimiser plumbing (reference: gs_model.py:43-67) -------------------------------------------------
    def changing_optimizer(self):
        groups = [{"params": p, "lr": float(self.lr[name])} for name, p in self.named_parameters(recurse=False)]
        # on the GPU one streaming kernel per tensor (torch's per-op Adam: 0.95 ms per step at 10^6 Gaussians, its fused
        # multi-tensor form 0.38, HipAdam 0.2)
        self._optimizer = HipAdam(groups, fused=self.adam != "tensor") if self.mean.is_cuda else torch.optim.Adam(groups)

    def set_mean_lr(self, iteration):
        """The reference rebuilds Adam (and drops its moments) every step to change one rate (gs_control.py:195-197);
        here the rate of the `mean` group is updated in place."""
        self.lr["mean"] = self.mean_lr_setfunc(iteration)
        for group, (name, _) in zip(self._optimizer.param_groups, self.named_parameters(recurse=False)):
            if name == "mean":
                group["lr"] = float(self.lr["mean"])

    def train_step(self, visible=None):
        """One optimiser step.  `visible` (bool [N] on the device, e.g. `forward`'s grad_iter): the rows adam="sparse" updates,
        required there; the other modes ignore it."""
        if self.adam == "sparse":
            if visible is None:
                raise RuntimeError("adam='sparse' needs train_step(visible=...): the rows to update (forward's grad_iter)")
            self._optimizer.step(visible=visible)
        else:
            self._optimizer.step()
        self._optimizer.zero_grad(set_to_none=True)
        return self

    def oneup_sh_degree(self):
        """Activate the next SH degree, up to L_max; returns the active degree.  Rows above it keep exact zero gradients,
        and Adam leaves a row with zero gradient and zero moments where it is: they start training when they are activated."""
        self.active_sh_degree = min(self.active_sh_degree + 1, self._L_max)
        return self.active_sh_degree

    # ---- camera data parallelism (one process per GPU; the reference is single-GPU) ----------------------------
    def allreduce_grads(self, grad_iter=None, group=None):
        """Cameras of a batch are independent: each rank renders its share (`batch[rank::world]`, loss weighted by its
        share of the batch) and the parameter gradients are summed with ONE all-reduce of the concatenated N x 38
        floats (sharding.allreduce_gaussian_grads; RCCL over xGMI under backend "nccl").  `grad_iter` (seen by any
        camera) is OR-ed across ranks.  Every rank then takes the same optimiser step."""
        import torch.distributed as dist

        from . import sharding

        params = [p for _, p in self.named_parameters(recurse=False)]
        grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in params]
        for p, g in zip(params, sharding.allreduce_gaussian_grads(*grads, group=group)):
            p.grad = g.contiguous()
        if grad_iter is not None:
            seen = grad_iter.to(torch.uint8)
            if seen.is_cuda and dist.get_backend(group) == "gloo":
                host = seen.cpu()
                dist.all_reduce(host, op=dist.ReduceOp.MAX, group=group)
                seen = host.to(grad_iter.device)
            else:
                dist.all_reduce(seen, op=dist.ReduceOp.MAX, group=group)
            grad_iter = seen.bool()
        return grad_iter

    # ---- densification statistics (:190-199) ----------------------------------------------------------------
    def _zero_density_stats(self, n):
        """Both statistics (see `densify_on`) at zero for `n` Gaussians."""
        dev = self.mean.device
        self.mean_grads_norm = torch.zeros(n, device=dev, dtype=torch.float32)
        self.mean_grads_iter = torch.zeros(n, device=dev, dtype=torch.int16)
        self.screen_grads_norm = torch.zeros(n, device=dev, dtype=torch.float32)
        self.screen_grads_views = torch.zeros(n, device=dev, dtype=torch.int32)

    def param_iter_update(self, grad_iter):
        if self.mean.grad is not None:
            self.mean_grads_norm += self.mean.grad.norm(dim=1)
            self.mean_grads_iter += grad_iter.to(torch.int16)

    def param_grads_per_iter_norm(self):
        return self.mean_grads_norm / (self.mean_grads_iter + (self.mean_grads_iter == 0).int())

    def _replace(self, keep, extra=None):
        """Keep rows `keep` of every per-Gaussian tensor and append `extra` (dict name -> rows)."""
        for name in PARAM_NAMES:
            rows = getattr(self, name).data[keep]
            if extra is not None:
                rows = torch.cat((rows, extra[name]), dim=0)
            setattr(self, name, torch.nn.Parameter(rows))
        for name in ("mean_grads_norm", "mean_grads_iter"):
            rows = getattr(self, name)[keep]
            if extra is not None:
                rows = torch.cat((rows, extra[name]), dim=0)
            setattr(self, name, rows)
        self.filter_3d = None  # the row set changed: `update_filter_3d` again

    def _rows(self, mask, repeat=1):
        out = {k: getattr(self, k).data[mask].repeat(repeat, *([1] * (getattr(self, k).dim() - 1)))
               for k in PARAM_NAMES}
        out["mean_grads_norm"] = self.mean_grads_norm[mask].repeat(repeat)
        out["mean_grads_iter"] = self.mean_grads_iter[mask].repeat(repeat)
        return out

    def densify_and_split(self, scene_extent, N=2):
        """Large Gaussians with a big positional gradient are replaced by N samples of themselves (:201-227)."""
        scale = torch.exp(self.variance_scale.data)
        sel = (self.param_grads_per_iter_norm() >= self.grad_threshold) & (scale.max(dim=1).values > self.percent_dense * scene_extent)
        new = self._rows(sel, N)
        stds = scale[sel].repeat(N, 1)
        q = self.variance_q.data[sel] / torch.norm(self.variance_q.data[sel], dim=1, keepdim=True).clamp_min(1e-8)
        rots = qvec_to_rotmat_batch(q).repeat(N, 1, 1)
        new["mean"] = torch.bmm(rots, torch.normal(torch.zeros_like(stds), stds).unsqueeze(-1)).squeeze(-1) + new["mean"]
        new["variance_scale"] = torch.log(stds / (0.8 * N))
        self._replace(~sel, new)

    def densify_and_clone(self, scene_extent):
        """Small Gaussians with a big positional gradient are duplicated (:229-243)."""
        sel = (self.param_grads_per_iter_norm() >= self.grad_threshold) & (
            torch.exp(self.variance_scale.data).max(dim=1).values <= self.percent_dense * scene_extent)
        self._replace(torch.ones_like(sel), self._rows(sel))

    def densify_and_prune(self, extent):
        """(:245-265)"""
        self.densify_and_split(extent)
        self.densify_and_clone(extent)
        prune = (torch.sigmoid(self.opacity.data) < self.prunning_min_opacity).squeeze(1)
        prune |= torch.exp(self.variance_scale.data).max(dim=1).values > 0.1 * extent
        self._replace(~prune)
        self.changing_optimizer()

    def reset_opacity(self, reset_opacity, keep_optimizer=False):
        """(:267-271).  keep_optimizer=True: the opacity is clamped in place and only its own two Adam moments are zeroed; every
        other tensor's moments and every step count stay (the default rebuilds the optimiser, as the reference does)."""
        cap = torch.full_like(self.opacity.data, reset_opacity)
        if keep_optimizer:
            with torch.no_grad():
                self.opacity.copy_(torch.logit(torch.minimum(torch.sigmoid(self.opacity.data), cap)))
            state = self._optimizer.state.get(self.opacity)
            if state:
                state["exp_avg"].zero_()
                state["exp_avg_sq"].zero_()
            return
        self.opacity = torch.nn.Parameter(torch.logit(torch.minimum(torch.sigmoid(self.opacity.data), cap)))
        self.changing_optimizer()

    # ---- density control on the device (csrc/gcp_densify.hip) -------------------------------------------------------
    def _density_stats(self):
        """The active statistic as the plan kernel reads it: (float32 norm, int32 count)."""
        if self.densify_on == "screen":
            return self.screen_grads_norm, self.screen_grads_views
        return self.mean_grads_norm.float(), self.mean_grads_iter.to(torch.int32)

    @torch.no_grad()
    def densify_and_prune_device(self, extent, seed, n_split=2):
        """Split, clone and prune in ONE pass of HIP kernels that keeps Adam's state; returns (n_before, n_after).

        With g = statistic / max(count, 1) (see `densify_on`), s = the largest scale and hot = count > 0 and
        g >= grad_threshold, every Gaussian takes one action, decided on the state before the call: split (hot,
        s > percent_dense * extent: `n_split` children sampled from it, of scale s / (0.8 n_split), replace it), clone (hot
        otherwise: the Gaussian and one copy) or keep; then the rows it would write are dropped if
        sigmoid(opacity) < prunning_min_opacity (the raw opacity, also under antialias=True) or their largest scale > 0.1 * extent.  This is the clone -> split -> prune
        sequence of other 3DGS trainers with zero statistics on new rows; `densify_and_prune` (the reference's order) lets
        split children inherit the parent's statistic, so they may be cloned in the same call.
        Rows come out in Gaussian order, a Gaussian's rows next to each other.  A surviving row keeps its exp_avg /
        exp_avg_sq, fresh rows start at 0.0, every tensor's `step` is kept.  The split samples are Philox4x32-10 draws keyed
        by `seed` (64 bits) and counted by (parent, child): the same on every rank, independent of torch's generators.  All
        statistic arrays come back zeroed at the new length.  One 4-byte device->host read (the new row count).  GPU only."""
        if not self.mean.is_cuda:
            raise RuntimeError("density control on the device is a set of HIP kernels: tensors must live on the GPU (no CPU path)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("densify_and_prune_device reads the new row count back: it cannot be captured into a graph")
        old = {k: getattr(self, k) for k in PARAM_NAMES}
        n = self.mean.shape[0]
        norm, views = (t.contiguous() for t in self._density_stats())
        if norm.numel() != n or views.numel() != n:  # the active pair only: the other one is reallocated below
            raise RuntimeError("the densification statistic does not have one row per Gaussian")
        states = {k: st for k, st in ((k, self._optimizer.state.get(p)) for k, p in old.items()) if st}
        new, moments, m = density.densify_rows(
            {k: p.data.contiguous() for k, p in old.items()}, {k: (st["exp_avg"], st["exp_avg_sq"]) for k, st in states.items()},
            norm, views, self.grad_threshold, self.percent_dense * extent, 0.1 * extent, self.prunning_min_opacity, n_split, seed)
        for k in PARAM_NAMES:
            setattr(self, k, torch.nn.Parameter(new[k]))
        self.changing_optimizer()
        for k, (exp_avg, exp_avg_sq) in moments.items():
            self._optimizer.state[getattr(self, k)] = {"step": states[k]["step"], "exp_avg": exp_avg, "exp_avg_sq": exp_avg_sq}
        self._zero_density_stats(m)
        self.filter_3d = None  # the row set changed: `update_filter_3d` again
        return n, m

    # ---- the MCMC strategy (3DGS-MCMC, Kheradmand et al. 2024; csrc/gcp_mcmc.hip) -----------------------------------------
    @torch.no_grad()
    def add_position_noise(self, seed, noise_lr=5e5):
        """After an optimiser step: mean += lr_mean * noise_lr * gate * Sigma z, in place, one HIP kernel (`density.mcmc_noise`).
        gate = sigmoid(100 (0.005 - sigmoid(opacity))) lets only nearly transparent Gaussians move, Sigma is the Gaussian's own
        covariance, z a Philox4x32-10 normal keyed by `seed` (64 bits) and counted by the Gaussian: the same on every rank.
        lr_mean is `self.lr["mean"]`, the rate `set_mean_lr` keeps.  GPU only."""
        density.mcmc_noise(self.mean.data, self.variance_q.data, self.variance_scale.data, self.opacity.data,
                           float(self.lr["mean"]) * noise_lr, seed)

    @torch.no_grad()
    def relocate_and_grow_device(self, seed, cap_max=None, growth=1.05, min_opacity=None):
        """Relocate dead Gaussians and grow the scene to a fixed row count in ONE pass of HIP kernels that keeps Adam's
        state; returns (n_before, n_after).  n_after = n_before when `cap_max` is None, else
        max(n_before, min(cap_max, int(growth * n_before))): host arithmetic, so the pass reads nothing back from the device
        and needs no gradient statistic, no threshold and no opacity reset.

        A Gaussian is dead at !(sigmoid(opacity) > min_opacity) (default `prunning_min_opacity`; the raw opacity, also under
        antialias=True).  Every dead row and every new row is a slot that draws a live source with probability proportional to its
        opacity (integer weights of 2^16 levels, fewer above 32 767 Gaussians: DESIGN.md §5) from Philox4x32-10 keyed by `seed`
        (64 bits) and counted by the row: the same on every rank.  A slot becomes a copy of its source; a source drawn c times
        and its c copies all get the opacity o' with (1 - o')^(c + 1) = 1 - o and the scale that keeps what the source rendered
        (the paper's relocation rule, c + 1 capped at 51), computed in float64.  Rows that nothing drew are untouched.
        Two deviations from the published code.  One pass on the state before it instead of relocate-then-add: both kinds
        of slot draw from the same distribution, and a source's count is the sum over both.  And Adam's moments are zeroed on
        relocated rows as well as on their sources; the published code zeroes only the sources' and leaves a relocated row
        the moments of the Gaussian it replaced.  Every other row keeps exp_avg / exp_avg_sq, every tensor's `step` is kept.
        All statistic arrays come back zeroed at the new length.  GPU only."""
        if not self.mean.is_cuda:
            raise RuntimeError("density control on the device is a set of HIP kernels: tensors must live on the GPU (no CPU path)")
        old = {k: getattr(self, k) for k in PARAM_NAMES}
        n = self.mean.shape[0]
        m = n if cap_max is None else max(n, min(int(cap_max), int(growth * n)))
        states = {k: st for k, st in ((k, self._optimizer.state.get(p)) for k, p in old.items()) if st}
        new, moments, _ = density.mcmc_rows(
            {k: p.data.contiguous() for k, p in old.items()}, {k: (st["exp_avg"], st["exp_avg_sq"]) for k, st in states.items()},
            m, self.prunning_min_opacity if min_opacity is None else min_opacity, seed)
        for k in PARAM_NAMES:
            setattr(self, k, torch.nn.Parameter(new[k]))
        self.changing_optimizer()
        for k, (exp_avg, exp_avg_sq) in moments.items():
            self._optimizer.state[getattr(self, k)] = {"step": states[k]["step"], "exp_avg": exp_avg, "exp_avg_sq": exp_avg_sq}
        self._zero_density_stats(m)
        self.filter_3d = None  # the row set changed: `update_filter_3d` again
        return n, m

    # ---- prune by what a Gaussian paints (csrc/gcp_contrib.hip) -------------------------------------------------------------
    @torch.no_grad()
    def contribution(self, P, K, wh, stats=None):
        """What every Gaussian contributes to the images of the cameras (P, K, wh) -> (w_max f32[N], w_sum f32[N],
        views i32[N]): per Gaussian the maximum over all pixels of all cameras, and the sum, of the colour weight
        w = T o g the blend paints it with (`cuda_kernel.contribution`), and the number of cameras whose list holds it.
        The cameras are projected with the model's own options (`camera_inputs`), so the opacity measured is the one the
        blend sees — sigmoid(opacity) rho under antialias=True — with float centres under centres="subpixel".  A camera that
        sees nothing is skipped; a Gaussian no camera lists keeps 0, 0, 0.
        `stats`: the triple an earlier call returned; it is accumulated in place and returned, so the training set can be
        fed in batches.  Cameras are folded in in the order given, one after the other: feeding them one at a time in that
        order gives the same w_sum bit for bit (w_max and views do in any order).
        No gradient, no hook, no generator, and the densification statistics are not touched.  GPU only."""
        cams, _, (width, height) = self.camera_inputs(P, K, wh)
        n, dev = self.mean.shape[0], self.mean.device
        if stats is None:
            stats = (torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev),
                     torch.zeros(n, dtype=torch.int32, device=dev))
        w_max, w_sum, views = stats
        if not (w_max.shape == w_sum.shape == views.shape == (n,)):
            raise RuntimeError(f"stats: expected three tensors of shape ({n},), one row per Gaussian")
        for cam in cams:
            if cam is None:
                continue
            cam_max, cam_sum = _camera_contribution(cam["startpoint"], cam["endpoint"], cam["mean"], cam["variance_inverse"], cam["opacity"],
                                                    width, height)
            index = cam["index"]  # unique within a camera: plain indexed statements, no atomics
            w_max[index] = torch.maximum(w_max[index], cam_max)
            w_sum[index] = w_sum[index] + cam_sum
            views[index] = views[index] + 1
        return stats

    @torch.no_grad()
    def prune_rows(self, keep):
        """Keep the rows where `keep` (bool [N] on the device) is true, in order, with Adam's state; returns
        (n_before, n_after).  Parameters and exp_avg / exp_avg_sq are gathered by the row kernel of the device density control
        (`density.keep_rows`), every tensor's `step` is kept, all statistic arrays come back zeroed at the new length — the
        bookkeeping of `densify_and_prune_device` after its gather.  One device->host read (the new row count), so it cannot
        be captured into a graph.  An all-false `keep` raises and leaves the model as it was.  GPU only."""
        if not self.mean.is_cuda:
            raise RuntimeError("pruning on the device is a set of HIP kernels: tensors must live on the GPU (no CPU path)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("prune_rows reads the new row count back: it cannot be captured into a graph")
        old = {k: getattr(self, k) for k in PARAM_NAMES}
        n = self.mean.shape[0]
        states = {k: st for k, st in ((k, self._optimizer.state.get(p)) for k, p in old.items()) if st}
        new, moments, m = density.keep_rows(
            {k: p.data.contiguous() for k, p in old.items()}, {k: (st["exp_avg"], st["exp_avg_sq"]) for k, st in states.items()}, keep)
        for k in PARAM_NAMES:
            setattr(self, k, torch.nn.Parameter(new[k]))
        self.changing_optimizer()
        for k, (exp_avg, exp_avg_sq) in moments.items():
            self._optimizer.state[getattr(self, k)] = {"step": states[k]["step"], "exp_avg": exp_avg, "exp_avg_sq": exp_avg_sq}
        self._zero_density_stats(m)
        self.filter_3d = None  # the row set changed: `update_filter_3d` again
        return n, m

    def prune_by_contribution(self, stats, threshold=0.01, on="max"):
        """`prune_rows` on what `contribution` measured: a Gaussian stays if w_max >= threshold (on="max", RadSplat's
        importance score) or w_sum >= threshold (on="sum", LightGaussian's significance, in pixels); returns
        (n_before, n_after).  A Gaussian buried behind others, seen by no camera, or too thin to paint `threshold` of any
        pixel goes, whatever its opacity parameter says.  The default 0.01 is RadSplat's value for the maximum and has NOT been
        tuned here: no full-length run on real poses exists; for on="sum" choose a threshold of your own."""
        if on not in ("max", "sum"):
            raise ValueError(f"on: 'max' or 'sum', got {on!r}")
        return self.prune_rows(stats[0 if on == "max" else 1] >= threshold)

    def allreduce_density_stats(self, group=None):
        """Sum the screen-space statistic over the ranks, so that every rank takes the same densification decisions; under
        backend "gloo" through the host, as `allreduce_grads`.  Under densify_on="position" there is nothing to sum: every rank
        already holds the same statistic (the gradients were all-reduced before `param_iter_update`), and the call returns."""
        import torch.distributed as dist

        if self.densify_on != "screen":
            return
        for t in (self.screen_grads_norm, self.screen_grads_views):
            if t.is_cuda and dist.get_backend(group) == "gloo":
                host = t.cpu()
                dist.all_reduce(host, group=group)
                t.copy_(host)
            else:
                dist.all_reduce(t, group=group)

    def _watch_centres(self, cams, width, height):
        """densify_on="screen": hooks on the cameras' float centres that add the norm of their gradient, scaled to NDC units
        (W/2, H/2), to `screen_grads_norm` and one view to `screen_grads_views` when `backward` reaches them.
        screen_grad="abs": every such camera also gets its "absgrad" buffer ([m, 2], handed to the Function by `forward` /
        `render`), and the hook accumulates that buffer instead of the signed gradient — the Function's backward has filled it
        by the time the gradient of its input reaches the hook."""
        if self.densify_on != "screen" or not torch.is_grad_enabled():
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("densify_on='screen' collects its statistic in autograd hooks, which a captured graph (cuda_kernel.GraphedStep) "
                               "does not replay: capture with densify_on='position'")
        scale = (0.5 * width, 0.5 * height)
        for cam in cams:
            if cam is not None and cam["mean"].requires_grad:
                if self.screen_grad == "abs":
                    cam["absgrad"] = _absgrad_buffer(cam["startpoint"])
                    cam["mean"].register_hook(lambda grad, index=cam["index"], buf=cam["absgrad"]: self._accumulate_centres(buf, index, scale))
                else:
                    cam["mean"].register_hook(lambda grad, index=cam["index"]: self._accumulate_centres(grad, index, scale))

    def _accumulate_centres(self, grad, index, scale):
        if self.screen_grads_norm.numel() != self.mean.shape[0]:
            raise RuntimeError("screen_grads_norm does not have one row per Gaussian: with densify_on='screen' densify with "
                               "densify_and_prune_device, which resizes it")
        accumulate_screen_grads(grad, index, scale, self.screen_grads_norm, self.screen_grads_views)

    # ---- forward (:277-460) ------------------------------------------------------------------------------------
    @torch.no_grad()
    def update_filter_3d(self, P, K, wh, variance=0.2):
        """Compute and keep `self.filter_3d` float32 (N,), the 3-D filter's size per Gaussian, from the cameras (P, K, wh):
        phi = sqrt(variance) / rate, rate = the largest focal / depth over the cameras that see the Gaussian
        (`sampling_rate`: depth > 0.2, centre within the image widened by 15 %), the rows no camera sees getting the largest phi
        of the seen ones (`filter_from_rate`).  Pass ALL training cameras, not a batch; under camera data parallelism every
        rank passes the full camera arrays (they are small), so there is no collective and every rank gets the same bits.
        Call it before the first draw, every ~100 iterations (the means move) and after every pass that changes the row set.
        variance = 0.2 and that cadence are Mip-Splatting's published values, not tuned here.  One kernel and a few torch ops,
        nothing read back.  Returns the tensor."""
        if not self.use_filter_3d:
            raise RuntimeError("update_filter_3d: this model was built without filter_3d=True")
        if not self.mean.is_cuda:
            raise RuntimeError("the 3-D filter is a HIP kernel: tensors must live on the GPU (no CPU path)")
        self.filter_3d = filter_from_rate(sampling_rate(self.mean.data, P, K, wh), variance)
        return self.filter_3d

    def _filtered(self):
        """(variance_scale, opacity) as the blend sees them: through `apply_filter` under filter_3d=True, the raw parameters
        otherwise."""
        if not self.use_filter_3d:
            return self.variance_scale, self.opacity
        if not self.mean.is_cuda:
            raise RuntimeError("the 3-D filter is a HIP kernel: tensors must live on the GPU (no CPU path)")
        if self.filter_3d is None or self.filter_3d.shape[0] != self.mean.shape[0]:
            raise RuntimeError("filter_3d=True but the filter is stale (never computed, or the row set changed since): call "
                               "update_filter_3d(P, K, wh) with all training cameras before drawing")
        return apply_filter(self.variance_scale, self.opacity, self.filter_3d)

    def camera_inputs(self, P, K, wh, with_depth=False, capture_safe=False):
        if capture_safe and self.densify_on == "screen":
            raise RuntimeError("densify_on='screen' does not support capture-safe lists: its statistic is collected per kept list entry")
        variance_scale, opacity = self._filtered()
        return camera_inputs(self.mean, self.variance_q, variance_scale, opacity, self.color, P, K, wh,
                             self.variance_pixel_tile_max_width, self.active_sh_degree, capture_safe=capture_safe,
                             with_depth=with_depth, sh_frame=self.sh_frame, centres=self.centres, cov_dilation=self.cov_dilation,
                             clamp_colour=self.clamp_colour, antialias=self.antialias)

    # ---- scene files (ply_io) ------------------------------------------------------------------------------------
    def save_ply(self, path, convention="3dgs", bake_filter=True):
        """The scene as a standard 3DGS .ply (ply_io.save_ply).  Other renderers evaluate the SH basis on world-space
        directions: a model in the camera frame with an active degree > 0 is saved with a warning.
        Under filter_3d=True the file holds, by default, the FILTERED scales and opacities (`apply_filter` on the current
        `filter_3d`; a stale filter raises), so a standard viewer shows what was trained and `from_ply` into a model without
        the filter draws the same images; bake_filter=False writes the raw parameters.  Without filter_3d the argument has no
        effect and the file is byte for byte what it always was."""
        from . import ply_io

        if self.sh_frame != "world" and self.active_sh_degree > 0:
            import warnings

            warnings.warn("save_ply: this model evaluates its SH colour on camera-frame directions (sh_frame='camera'); other "
                          "renderers use world-space directions, so the view dependence of the saved scene will be wrong there")
        variance_scale, opacity = self.variance_scale.data, self.opacity.data
        if self.use_filter_3d and bake_filter:
            with torch.no_grad():
                variance_scale, opacity = self._filtered()
        ply_io.save_ply(path, self.mean.data, self.variance_q.data, variance_scale, opacity, self.color.data, convention=convention)

    @classmethod
    def from_ply(cls, path, device="cpu", convention="3dgs", **model_kwargs):
        """A model of the scene in `path` (ply_io.load_ply); L_max comes from the file's number of SH coefficients."""
        from . import ply_io

        mean, variance_q, variance_scale, opacity, color = ply_io.load_ply(path, device=device, convention=convention)
        L_max = math.isqrt(color.shape[1]) - 1
        if model_kwargs.setdefault("L_max", L_max) != L_max:
            raise ValueError(f"{path} holds degree {L_max}, L_max={model_kwargs['L_max']} was asked for")
        model = cls(mean, variance_q, variance_scale, opacity, **model_kwargs)
        with torch.no_grad():
            model.color.copy_(color)
        return model

    @staticmethod
    def _draw_cameras(cams, names, draw):
        """`draw(cam)`, a tuple of maps, for every camera that sees anything (the reference drops the others from the batch,
        :414-417) -> (every map stacked over those cameras, their names)."""
        drawn, kept = [], []
        for cam, name in zip(cams, names):
            if cam is None:
                continue
            drawn.append(draw(cam))
            kept.append(name)
        if not drawn:
            raise RuntimeError("no camera of the batch sees any Gaussian")  # the reference fails in torch.stack (:454)
        return [torch.stack(maps, dim=0) for maps in zip(*drawn)], kept

    def forward(self, P, K, wh, image_sample):
        cams, grad_iter, (width, height) = self.camera_inputs(P, K, wh)
        self._watch_centres(cams, width, height)

        def draw(cam):
            batch = cam["boxsize"].new_tensor([cam["boxsize"].numel()])
            extra = (cam["absgrad"],) if cam.get("absgrad") is not None else ()  # screen_grad="abs" (`_watch_centres`)
            return (custom_autograd_grouped_cumprod.apply(
                cam["boxsize"], batch, cam["startpoint"], cam["endpoint"], cam["mean"], cam["variance_inverse"],
                cam["opacity"], cam["l_d"], width, height, *extra),)

        (out,), names = self._draw_cameras(cams, image_sample, draw)
        out = out[:, 1:, 1:, :]
        h, w = int(height), int(width)
        out = out.reshape(-1, 3, h, w) if self.reference_layout else out.permute(0, 3, 1, 2).contiguous()
        return [out, names, grad_iter]

    def render(self, P, K, wh, background=None, image_sample=None, distortion=False, normals=False, median=False):
        """`forward` with the expected-depth and alpha maps and a background colour (`cuda_kernel.render`, whose
        docstring pins the definitions: depth = sum of the colour weights times the camera-space depth, NOT divided by
        alpha; alpha = 1 - the transmittance behind the pixel; image composited over `background`, a float[3] device tensor
        or None for black).  Returns [images (B, 3, H, W), depth (B, 1, H, W), alpha (B, 1, H, W), names, grad_iter], all
        maps after the same [1:, 1:] crop as `forward`; `names` are `image_sample`'s entries (default: camera indices) of the
        cameras that see anything — the others are dropped, as in `forward`.
        distortion=True: [images, depth, alpha, distortion (B, 1, H, W), names, grad_iter] — the per-pixel depth distortion
        of `cuda_kernel.render(distortion=True)` (sum_{i>j} 2 w_i w_j (z_i - z_j) over the pixel's kept pairs, z the
        camera-space depth the list is sorted by; not divided by alpha), cropped like the others; the first three maps are the
        same bits as without it.
        normals=True: one more map after those, normal (B, 3, H, W) = sum_k w_k n_k in camera coordinates, cropped like the
        others, not divided by alpha — [images, depth, alpha, (distortion,) normal, names, grad_iter].  Per camera the
        normals of its list come from `gaussian_normals` on the RAW parameters (variance_q, variance_scale, mean; the 3-D
        filter does not change which axis is the shortest) and `cam["index"]`, and are blended by
        `cuda_kernel.render(normal=)`; their gradient reaches variance_q, the map's weights' the other parameters.  What
        `normal_consistency(depth, alpha, normal, K)` takes.  The other maps are the same bits as without it.
        median=True: one more map after every other map and before `names`, median (B, 1, H, W): the median depth of
        `cuda_kernel.render(median=True)` (the depth of the layer at which the pixel's transmittance falls through 1/2; a copy
        of one Gaussian's depth, NOT multiplied by alpha; 2DGS's depth_ratio = 1), cropped like the others; its gradient reaches
        the parameters through that Gaussian's camera-space depth alone.  `median_as_depth(median, alpha)` turns it into the
        pair `normal_consistency` and `TSDFVolume.integrate` take.  The other maps are the same bits as without it."""
        cams, grad_iter, (width, height) = self.camera_inputs(P, K, wh, with_depth=True)
        self._watch_centres(cams, width, height)
        if normals:
            for c, cam in enumerate(cams):
                if cam is not None:
                    cam["normal"] = gaussian_normals(self.variance_q, self.variance_scale, self.mean, P[c], cam["index"])
        maps, names = self._draw_cameras(
            cams, range(P.shape[0]) if image_sample is None else image_sample,
            lambda cam: render(cam["startpoint"], cam["endpoint"], cam["mean"], cam["variance_inverse"], cam["opacity"], cam["l_d"],
                               cam["depth"], width, height, background, cam.get("absgrad"), distortion=distortion,
                               normal=cam.get("normal"), median=median))
        images = maps[0][:, 1:, 1:, :].permute(0, 3, 1, 2).contiguous()
        tail = [maps.pop()[:, None, 1:, 1:].contiguous()] if median else []  # the median is always the last map
        n_planes = len(maps) - (2 if normals else 1)
        planes = [m[:, None, 1:, 1:].contiguous() for m in maps[1:1 + n_planes]]  # depth, alpha[, distortion]
        if normals:
            planes.append(maps[-1][:, 1:, 1:, :].permute(0, 3, 1, 2).contiguous())
        return [images, *planes, *tail, names, grad_iter]

    @torch.no_grad()
    def evaluate(self, P, K, wh, targets, background=None, batch_size=4, clamp=True, exposure=None):
        """Image quality on the cameras (P, K, wh) against `targets` (C, 3, H, W) -> `ImageMetrics` (mse, l1, ssim, psnr:
        float64 (C,) on the device), one entry per camera, in order.  The cameras are projected with the model's own options
        and painted as `render` paints them (`background`: float[3] on the device or None for black; the [1:, 1:] crop,
        (B, 3, H, W)) by `cuda_kernel.paint` — the blend without transmittance checkpoints, no autograd node — `batch_size`
        at a time, each batch measured in one pass (`image_metrics`; `clamp`: the render is clamped to [0, 1] first).
        A camera that sees no Gaussian is NOT dropped: its image is the background (or black) and it is measured like the
        others.  Nothing of the training state is touched: no `.grad`, no densification statistic, no optimiser state, no
        generator — a training run with evaluations in it takes the same steps as one without.  The metrics stay on the
        device; the host reads are those of the projection and the binning.  GPU only.  LPIPS is not computed.
        `exposure` (C, 3, 4): one colour affine per camera (`CameraExposure.rows`), handed to `image_metrics` batch by batch —
        the render is compensated first and clamped after.  None (the default): no compensation, the plain kernel."""
        n_cam = P.shape[0]
        if targets.dim() != 4 or targets.shape[0] != n_cam:
            raise RuntimeError(f"targets: expected (C, 3, H, W) with one image per camera ({n_cam})")
        if exposure is not None and tuple(exposure.shape) != (n_cam, 3, 4):
            raise RuntimeError(f"exposure: expected (C, 3, 4) with one matrix per camera ({n_cam}), got {tuple(exposure.shape)}")
        batch_size = max(1, int(batch_size))
        with_depth = background is not None
        parts = []
        for c in range(0, n_cam, batch_size):
            cams, _, (width, height) = self.camera_inputs(P[c:c + batch_size], K[c:c + batch_size], wh[c:c + batch_size],
                                                          with_depth=with_depth)
            frames = []
            for cam in cams:
                if cam is None:  # nothing in view: the background alone
                    frame = torch.zeros(height + 1, width + 1, 3, dtype=torch.float32, device=self.mean.device)
                    if with_depth:
                        frame += background.detach().to(frame).reshape(1, 1, 3)
                else:
                    frame = _paint(cam["startpoint"], cam["endpoint"], cam["mean"], cam["variance_inverse"], cam["opacity"], cam["l_d"],
                                   width, height, cam["depth"] if with_depth else None, background)
                frames.append(frame)
            images = torch.stack(frames, dim=0)[:, 1:, 1:, :].permute(0, 3, 1, 2)
            if exposure is None:
                parts.append(image_metrics(images, targets[c:c + batch_size], clamp=clamp))
            else:
                parts.append(image_metrics(images, targets[c:c + batch_size], clamp=clamp, exposure=exposure[c:c + batch_size]))
        if not parts:
            empty = torch.zeros(0, dtype=torch.float64, device=self.mean.device)
            return ImageMetrics(empty, empty.clone(), empty.clone(), empty.clone())
        return ImageMetrics(*(torch.cat(field) for field in zip(*parts)))

    # ---- mesh extraction (mesh.py, csrc/gcp_tsdf.hip) ---------------------------------------------------------------------------
    @torch.no_grad()
    def extract_mesh(self, P, K, wh, resolution=256, bounds=None, trunc=None, alpha_min=0.5, depth_max=None, batch_size=4, colour=True,
                     depth="expected", keep_largest=None, min_faces=None, normals=False):
        """A triangle mesh of the scene -> (vertices float32 (V, 3), faces int32 (F, 3), colours float32 (V, 3) or None): the
        depth maps of the cameras (P, K, wh) — pass the TRAINING cameras — fused into a truncated signed distance volume
        (`TSDFVolume.integrate`), its zero level set extracted by marching tetrahedra (`TSDFVolume.extract`); what 2DGS, GOF,
        RaDe-GS and PGSR do through Open3D, and what `--normal-reg` / `--distortion-reg` shape the depth for.
        The cameras are projected with the model's own options (the 3-D filter applies if on) and painted over black by
        `cuda_kernel.paint_maps` with the [1:, 1:] crop of `render`, `batch_size` at a time, and integrated in the order
        given; a camera that sees nothing is integrated as an empty map, which changes nothing.
        `bounds`: ((x0, y0, z0), (x1, y1, z1)), the box the volume covers; default: the cube centred at the centroid of the
        camera centres with half-side r = the largest camera distance from that centroid (2DGS's bounded-scene radius).
        `resolution`: lattice points along the longest side: voxel = longest side / resolution (2 r / resolution by default), the
        other sides get as many points as cover them.  `trunc`: the truncation distance, default 5 voxel.  `depth_max`: depths
        beyond it are not fused, default the longest side (2 r); 0 = no limit.  `alpha_min`: pixels fainter than this are not
        fused.  resolution = 256, 5 voxels and alpha_min = 0.5 are pointers from 2DGS and Open3D usage; they are not tuned here.
        colour=False: no colour volume, colours is None.
        `depth`: "expected" (the default) fuses the expected depth sum w z / alpha; "median" the median depth of
        `cuda_kernel.paint_maps(median=True)` through `median_as_depth` — the depth of the layer at which the transmittance falls
        through 1/2, which lies on a surface at an occlusion edge and behind a faint floater, where the mean lies between the
        surfaces (2DGS's depth_ratio = 1 for bounded scenes: a pointer, not a tuned choice).  `alpha_min` gates on the real alpha
        either way.
        `keep_largest`, `min_faces`: both None (the default): the mesh as extracted, floaters included.  If either is given the
        other defaults to 50 and `clean_mesh` drops the small connected components (2DGS's post_process_mesh rule; 50 / 50 are
        its values: pointers, not tuned here).  `normals=True` appends a fourth element, `vertex_normals` of the mesh that is
        returned — computed AFTER the cleaning — pointing out of the surface, towards the cameras.
        A bounded scene only; no decimation, smoothing or hole filling.
        Nothing of the training state is touched: no `.grad`, no densification statistic, no optimiser state, no generator —
        like `evaluate`.  The host reads are those of the projection and the binning, one for the mesh's size and, with cleaning,
        one for the cleaned mesh's size.  GPU only."""
        n_cam, dev = P.shape[0], self.mean.device
        if depth not in ("expected", "median"):
            raise RuntimeError(f'depth: "expected" or "median", got {depth!r}')
        use_median = depth == "median"
        if not self.mean.is_cuda:
            raise RuntimeError("extract_mesh runs HIP kernels: the model must live on the GPU (no CPU path)")
        resolution = int(resolution)
        if resolution < 2:
            raise RuntimeError("resolution: at least 2")
        if bounds is None:
            if n_cam == 0:
                raise RuntimeError("extract_mesh: no camera and no bounds")
            Pd = P.detach().to(device=dev, dtype=torch.float64)
            centres = -(Pd[:, :, :3] * Pd[:, :, 3:]).sum(dim=1)  # -R^T t, camera by camera
            centroid = centres.mean(dim=0)
            r = float((centres - centroid).norm(dim=1).max())
            lo, hi = [float(c) - r for c in centroid], [float(c) + r for c in centroid]
        else:
            lo, hi = [float(v) for v in bounds[0]], [float(v) for v in bounds[1]]
        sides = [h - l for l, h in zip(lo, hi)]
        if len(sides) != 3 or not min(sides) > 0.0:
            raise RuntimeError(f"bounds: a box with three positive sides expected, got {lo} .. {hi}")
        voxel = max(sides) / resolution
        dims = tuple(max(2, int(math.ceil(side / voxel - 1e-9)) + 1) for side in sides)
        trunc = 5.0 * voxel if trunc is None else float(trunc)
        depth_max = max(sides) if depth_max is None else float(depth_max)
        volume = TSDFVolume(lo, voxel, dims, trunc, dev, colour=colour)
        batch_size = max(1, int(batch_size))
        for c in range(0, n_cam, batch_size):
            Pb, Kb = P[c:c + batch_size], K[c:c + batch_size]
            cams, _, (width, height) = self.camera_inputs(Pb, Kb, wh[c:c + batch_size], with_depth=True)
            frames = []
            for cam in cams:
                if cam is None:  # nothing in view: alpha = 0 everywhere, no lattice point is updated
                    frames.append((torch.zeros(height + 1, width + 1, 3, dtype=torch.float32, device=dev),
                                   torch.zeros(height + 1, width + 1, dtype=torch.float32, device=dev),
                                   torch.zeros(height + 1, width + 1, dtype=torch.float32, device=dev))
                                  + ((torch.zeros(height + 1, width + 1, dtype=torch.float32, device=dev),) if use_median else ()))
                elif use_median:
                    frames.append(_paint_maps(cam["startpoint"], cam["endpoint"], cam["mean"], cam["variance_inverse"], cam["opacity"],
                                              cam["l_d"], width, height, cam["depth"], median=True))
                else:
                    frames.append(_paint_maps(cam["startpoint"], cam["endpoint"], cam["mean"], cam["variance_inverse"], cam["opacity"],
                                              cam["l_d"], width, height, cam["depth"]))
            image, depth, alpha, *rest = (torch.stack(maps, dim=0) for maps in zip(*frames))
            if use_median:
                depth, alpha = median_as_depth(rest[0], alpha)
            volume.integrate(depth[:, None, 1:, 1:], alpha[:, None, 1:, 1:], Pb.to(dev), Kb.to(dev),
                             image=image[:, 1:, 1:, :].permute(0, 3, 1, 2) if colour else None, alpha_min=alpha_min, depth_max=depth_max)
        vertices, faces, colours = volume.extract()
        if keep_largest is not None or min_faces is not None:
            vertices, faces, colours, _ = clean_mesh(vertices, faces, colours, keep_largest=50 if keep_largest is None else keep_largest,
                                                     min_faces=50 if min_faces is None else min_faces)
        if normals:
            return vertices, faces, colours, vertex_normals(vertices, faces)
        return vertices, faces, colours
