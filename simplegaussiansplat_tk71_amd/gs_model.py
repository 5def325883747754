"""Caller of the hot path: 3-D Gaussians + cameras -> the inputs of the rasterise-and-blend Function -> images.

Mirrors the reference's model class (reference: gs_model.py:123-460, `GS_model_with_param`): same parameter set
(mean, variance_q, variance_scale, opacity, color), same `forward(P, K, wh, image_sample)` return value
`[images, image_sample, grad_iter]`, same per-parameter Adam learning rates, densify / prune / opacity reset.
Row f4 of SURVEY.md §8: this is caller integration, PyTorch on the GPU around the HIP Function — not a kernel.

The projection (`camera_inputs`, reference: gs_model.py:277-425) is pinned, through its PyTorch restatement in
oracle/gs_forward_torch.py, against the reference's own forward run on CPU (tests/golden/forward_golden.npz: the
arguments the reference hands to `custom_autograd_grouped_cumprod.apply`).  Differences, all deliberate:
  * the 3-sigma box comes from a closed-form 2x2 eigen-decomposition on the device; the reference moves every
    covariance to the CPU for `torch.linalg.eigh` and back (gs_model.py:327-332).  For a positive semi-definite
    matrix `V^2 |lambda|` is just its diagonal, so the box is 3*sqrt(diag) exactly;
  * the depth sort is stable (the reference's `torch.argsort`, :356, leaves ties undefined);
  * images are permuted to (B, 3, H, W); the reference `reshape`s (H, W, 3) memory into (3, H, W), scrambling
    channels (gs_model.py:454) — `reference_layout=True` reproduces that;
  * one Function call per camera, never chunked (nothing of pair-list size exists here; gs_model.py:428);
  * the SH colour stands in for the reference's `sh_utility.eval_sh`, which is not in its checkout
    (gs_model.py:9,335): real spherical harmonics up to degree 3 in the usual 3DGS order and sign — parity unpinned.
    The direction they are evaluated on is, by default, the reference's: -t/|t| in CAMERA coordinates (:335-338), so a
    Gaussian changes colour when the camera rolls; `sh_frame="world"` uses the world-space unit vector from the camera
    centre to the Gaussian, the convention of other 3DGS renderers (what a scene saved with `save_ply` needs);
  * tensors live on the parameters' device instead of a hard-coded "cuda";
  * on the GPU the whole per-Gaussian chain is ONE HIP kernel per camera and direction (`gcp_project_forward`,
    `gcp_project_backward`, csrc/gcp_project.hip) instead of ~150 PyTorch kernels: at 10^6 Gaussians the reference's
    formulation costs 64 ms forward + 110 ms backward around a 1.8 ms Function.  That formulation is kept, as the
    checker the kernels are tested against, in oracle/gs_forward_torch.py — not here: projection and loss have no
    CPU path (CPU tensors raise).
"""
import math
import numbers

import torch

from . import _lib
from . import raster as _raster
from .cuda_kernel import custom_autograd_grouped_cumprod, render

SH_FRAMES = {"camera": 0, "world": 1}
CENTRES = ("pixel", "subpixel")
DENSIFY_ON = ("position", "screen")


def _splat_options(centres, cov_dilation, clamp_colour, antialias=False):
    """Validated (centres, cov_eps, clamp_colour, antialias) of `camera_inputs`; ValueError before anything touches the GPU."""
    if centres not in CENTRES:
        raise ValueError(f"centres: 'pixel' or 'subpixel', got {centres!r}")
    cov_eps = 1e-6 if cov_dilation is None else cov_dilation
    if isinstance(cov_eps, bool) or not isinstance(cov_eps, numbers.Real) or not (math.isfinite(cov_eps) and cov_eps >= 0):
        raise ValueError(f"cov_dilation: None or a finite number >= 0, got {cov_dilation!r}")
    if not isinstance(clamp_colour, bool):
        raise ValueError(f"clamp_colour: True or False, got {clamp_colour!r}")
    if not isinstance(antialias, bool):
        raise ValueError(f"antialias: True or False, got {antialias!r}")
    if antialias and not (cov_dilation is not None and cov_dilation > 0):
        raise ValueError(f"antialias=True compensates the opacity for a covariance dilation: cov_dilation must be > 0, got {cov_dilation!r}")
    return centres, float(cov_eps), clamp_colour, antialias

__all__ = [
    "GS_dataset",
    "GS_model_with_param",
    "HipAdam",
    "accumulate_screen_grads",
    "camera_inputs",
    "qvec_to_rotmat_batch",
    "get_expon_lr_func",
    "mean_neighbour_distance",
    "splat_loss",
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


_CLAMP_CACHE = {}


def _box_clamp(width, height, tile_max_width):
    """Upper bound of the 3-sigma half extents: 10 * sqrt(W*H) * sigmoid(tile_max_width) in float32, as the reference forms
    it (gs_model.py:364-365).  Evaluated once per (W, H, setting) on the host: no device work, no read-back."""
    key = (width, height, float(tile_max_width))
    if key not in _CLAMP_CACHE:
        t = torch.sqrt(torch.tensor(width * height, dtype=torch.int32).to(torch.float32)) * torch.sigmoid(
            torch.tensor(float(tile_max_width), dtype=torch.float32))
        _CLAMP_CACHE[key] = (t * 10).item()
    return _CLAMP_CACHE[key]


class _ProjectCamera(torch.autograd.Function):
    """One camera of `camera_inputs` on the HIP library: the projection's forward kernel, the library's stable radix sort on
    the depth keys, its gather; backward = its backward kernel.  `L_max` is the ACTIVE degree, which may be below what `color`
    stores; `sh_frame` 0 / 1 = camera / world directions; with_depth: the camera-space depths too, right after l_d.
    splat=None: the reference's conventions, on the kernels of csrc/gcp_project.hip (gcp_project_forward_sh,
    gcp_project_gather or gcp_project_gather_depth, gcp_project_backward_sh); the centre is int32 (m, 2) without a gradient.
    splat=(subpixel, cov_eps, clamp_colour): the kernels of csrc/gcp_splat.hip (gcp_splat_forward, gcp_splat_gather,
    gcp_splat_backward): `cov_eps` on the diagonal of the pixel covariance, the SH colour clamped at 0 (`clamp_colour`), and —
    `subpixel` — the pixel centre kept as float32 (m, 2) at px + 0.5, differentiable: its gradient is handed to the backward
    as grad_mean_xy.  Not `subpixel`: the centre is truncated as by default and returned as int32 without a gradient (the box
    still goes around the untruncated centre, by the rule of the float one).
    splat=(subpixel, cov_eps, clamp_colour, antialias): a fourth field, absent = False.  True: gcp_splat_forward_flags and
    gcp_splat_backward_flags with GCP_SPLAT_ANTIALIAS set — alpha is sigmoid(opacity) rho, rho = sqrt(det Sigma / det Sigma').
    Returns (vinv, alpha, l_d, [depth,] mean_xy, start, end, boxsize, index, keep)."""

    @staticmethod
    def forward(ctx, mean, variance_q, variance_scale, opacity, color, cam_P, cam_K, width, height, box_clamp, L_max,
                capture_safe=False, with_depth=False, sh_frame=0, splat=None):
        dev, n = mean.device, mean.shape[0]
        args = [t.detach().contiguous() for t in (mean, variance_q, variance_scale, opacity, color, cam_P, cam_K)]
        for t in args:
            if t.dtype != torch.float32 or t.device != dev:
                raise RuntimeError("projection expects float32 tensors on one device")
        if not mean.is_cuda:
            raise RuntimeError("the fused projection is a HIP kernel: tensors must live on the GPU (no CPU path)")
        lib = _lib.load()
        subpixel = splat is not None and splat[0]
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
        record, sort_key, row_of = f32(n, 16), i32(n), i32(n)
        keep = torch.empty(n, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            world = (*(t.data_ptr() for t in args), n, L_max, color.shape[1], sh_frame, width, height, box_clamp)
            made = (record.data_ptr(), sort_key.data_ptr(), keep.data_ptr(), row_of.data_ptr(), stream)
            if splat is None:
                _lib.check(lib.gcp_project_forward_sh(*world, *made), "gcp_project_forward")
            elif len(splat) > 3 and splat[3]:
                flags = _lib.SPLAT_ANTIALIAS | (_lib.SPLAT_CLAMP_COLOUR if splat[2] else 0)
                _lib.check(lib.gcp_splat_forward_flags(*world, splat[1], 0.5 if subpixel else 0.0, flags, *made), "gcp_splat_forward_flags")
            else:
                _lib.check(lib.gcp_splat_forward(*world, splat[1], 0.5 if subpixel else 0.0, int(splat[2]), *made), "gcp_splat_forward")
            # the one device->host read: sizes of the outputs.  capture_safe: none — the list keeps all n Gaussians, the
            # culled ones behind the kept ones with empty boxes (the gather with the keep mask)
            m = n if capture_safe else (int(keep.sum()) if n else 0)
            # culled Gaussians carry the largest key: the first m entries of the stable permutation are the kept ones in
            # depth order, ties in the Gaussians' own order
            perm = _raster.stable_sort_keys(sort_key, key_bits=31)[1] if n else sort_key
            start, end, boxsize = i32(m, 2), i32(m, 2), torch.empty(m, dtype=torch.int64, device=dev)
            mean_xy = i32(m, 2) if splat is None else f32(m, 2)
            vinv, alpha, l_d, index = f32(m, 2, 2), f32(m, 1), f32(m, 3), torch.empty(m, dtype=torch.int64, device=dev)
            depth = f32(m) if with_depth else None
            lists = (record.data_ptr(), perm.data_ptr(), m, start.data_ptr(), end.data_ptr(), mean_xy.data_ptr(), boxsize.data_ptr(),
                     vinv.data_ptr(), alpha.data_ptr(), l_d.data_ptr())
            rows = (index.data_ptr(), row_of.data_ptr(), keep.data_ptr() if capture_safe else None, stream)
            if splat is not None:
                _lib.check(lib.gcp_splat_gather(*lists, depth.data_ptr() if with_depth else None, *rows), "gcp_splat_gather")
            elif with_depth:
                _lib.check(lib.gcp_project_gather_depth(*lists, depth.data_ptr(), *rows), "gcp_project_gather_depth")
            else:
                _lib.check(lib.gcp_project_gather(*lists, *rows), "gcp_project_gather")
        if splat is not None and not subpixel:
            mean_xy = mean_xy.to(torch.int32)  # towards zero, as the kernels of gcp_project.hip convert
        keep = keep.view(torch.bool)
        ctx.save_for_backward(*args, row_of)
        ctx.L_max, ctx.with_depth, ctx.sh_frame, ctx.splat = L_max, with_depth, sh_frame, splat
        out = (vinv, alpha, l_d, *((depth,) if with_depth else ()), mean_xy, start, end, boxsize, index, keep)
        ctx.mark_non_differentiable(*out[-(5 if subpixel else 6):])
        return out

    @staticmethod
    def backward(ctx, g_vinv, g_alpha, g_ld, *rest):
        *args, row_of = ctx.saved_tensors
        mean, variance_q, variance_scale, opacity, color = args[:5]
        splat = ctx.splat
        subpixel = splat is not None and splat[0]
        grads = [torch.empty_like(t) for t in (mean, variance_q, variance_scale, opacity, color)]  # every row is written
        g = [t.contiguous().float() for t in (g_vinv, g_alpha, g_ld, *rest[:int(ctx.with_depth) + int(subpixel)])]
        g_depth = g[3].data_ptr() if ctx.with_depth else None
        with torch.cuda.device(mean.device):
            upstream = (*(t.data_ptr() for t in args), mean.shape[0], ctx.L_max, color.shape[1], ctx.sh_frame, row_of.data_ptr(),
                        *(t.data_ptr() for t in g[:3]), g_depth)
            made = (*(t.data_ptr() for t in grads), torch.cuda.current_stream(mean.device).cuda_stream)
            lib = _lib.load()
            if splat is None:
                _lib.check(lib.gcp_project_backward_sh(*upstream, *made), "gcp_project_backward")
            elif len(splat) > 3 and splat[3]:
                flags = _lib.SPLAT_ANTIALIAS | (_lib.SPLAT_CLAMP_COLOUR if splat[2] else 0)
                _lib.check(lib.gcp_splat_backward_flags(*upstream, splat[1], flags, g[-1].data_ptr() if subpixel else None, *made),
                           "gcp_splat_backward_flags")
            else:
                _lib.check(lib.gcp_splat_backward(*upstream, splat[1], int(splat[2]), g[-1].data_ptr() if subpixel else None, *made),
                           "gcp_splat_backward")
        return (*grads, *[None] * 10)


def camera_inputs(mean, variance_q, variance_scale, opacity, color, P, K, wh, tile_max_width, L_max=2, capture_safe=False,
                  with_depth=False, sh_frame="camera", centres="pixel", cov_dilation=None, clamp_colour=False, antialias=False):
    """Per camera, the depth-ordered, culled arguments of the Function (reference: gs_model.py:277-425).

    mean (N,3), variance_q (N,4 xyzw), variance_scale (N,3 log), opacity (N,1 logit), color (N,(L+1)^2,3),
    P (C,3,4) world->camera, K (C,3,3), wh (C,2), tile_max_width = logit of the box clamp as a fraction of
    sqrt(W*H)/10.  Returns a list with one dict per camera (None where nothing is visible, :414-417) holding
    boxsize, startpoint, endpoint, mean, variance_inverse, opacity, l_d, index (Gaussian ids, depth order),
    and the (N,) bool `grad_iter` of Gaussians seen by any camera (:401-407).

    One HIP kernel per camera and direction (csrc/gcp_project.hip); GPU tensors only — there is no CPU path.  The
    reference's op-by-op PyTorch formulation lives in oracle/gs_forward_torch.py as the checker.

    capture_safe=True: no device->host read at all (pass `wh` as a CPU tensor or a list): every camera's list keeps all N
    Gaussians in depth order, the culled ones behind the kept ones with EMPTY boxes (binned into no tile, zero
    gradients), and no camera is ever dropped; images and gradients are those of the default mode.  Together with
    `cuda_kernel.tile_capacity` the projection + Function forward and backward queue without waiting for the GPU.

    with_depth=True: every dict also holds "depth", the Gaussians' camera-space depths in list order (the positive depth
    they are sorted by; 0 for the culled entries of a capture-safe list), differentiable w.r.t. `mean` — the `depth`
    argument of `cuda_kernel.render`.

    L_max (0..3) is the ACTIVE SH degree: `color` may store more rows than (L_max+1)^2; those are not read and get exact
    zero gradients.  sh_frame: "camera" (the default, the reference's: the SH basis is evaluated on -t/|t| in camera
    coordinates) or "world" (on the world-space unit vector from the camera centre to the Gaussian, as other 3DGS
    renderers do: the colour does not change when the camera rolls).

    Three more conventions of other 3DGS renderers, opt-in (csrc/gcp_splat.hip; with the defaults nothing below runs):
    centres="subpixel": "mean" is float32 (m, 2) and differentiable — the projected centre px + 0.5 instead of trunc(px), so
    that the blend's gradient w.r.t. the centre reaches `mean` (with "pixel" a Gaussian's position is trained only through
    the Jacobian, the view direction and the depth).  The 0.5: pixel i of the cropped image is frame pixel i + 1 and its
    centre lies at i + 0.5 in the coordinates of K (COLMAP / 3DGS), so dx = (i + 1) - (px + 0.5) = (i + 0.5) - px.  The box
    is ceil(c - h) .. floor(c + h) around the float centre c, h = the clamped 3-sigma half extent.
    cov_dilation=F (finite, >= 0; None = 1e-6, the reference's): F is added to the diagonal of the pixel covariance (0.3: the
    usual screen-space dilation).  clamp_colour=True: l_d = max(SH sum, 0) per channel, no gradient through a clamped channel.
    centres="pixel" with a dilation or the clamp: "mean" stays int32, truncated as by default, without a gradient.
    antialias=True (needs cov_dilation > 0; ValueError otherwise): the opacity compensation of the dilation.  The dilated
    covariance Sigma' = Sigma + F I paints sqrt(det Sigma' / det Sigma) times the energy of the Gaussian it replaces — up to
    8.5 x for one of 0.2 px; "opacity" becomes sigmoid(opacity) rho with rho = sqrt(det Sigma / det Sigma') (det Sigma' with
    the 1e-6 "variance_inverse" is formed with), and rho's exact gradient reaches mean, variance_q and variance_scale.  A
    Gaussian whose det Sigma is <= 0 in float32 has rho = 0 and gets no gradient through it.  Every other entry is bit for
    bit what it is without the option.  Mip-Splatting's 2-D filter; the "antialiased" mode of other renderers."""
    if sh_frame not in SH_FRAMES:
        raise ValueError(f"sh_frame: 'camera' or 'world', got {sh_frame!r}")
    centres, cov_eps, clamp_colour, antialias = _splat_options(centres, cov_dilation, clamp_colour, antialias)
    # None: the defaults, on the kernels of csrc/gcp_project.hip
    splat = (centres == "subpixel", cov_eps, clamp_colour) if centres != "pixel" or cov_dilation is not None or clamp_colour else None
    if antialias:  # validated: there is a dilation, so `splat` is set
        splat = (*splat, True)
    width, height = (int(v) for v in (wh[0].tolist() if isinstance(wh, torch.Tensor) else wh[0]))  # device `wh`: one read (.to(int32) truncates, :279)
    clamp = _box_clamp(width, height, tile_max_width)
    grad_iter = None
    cams = []
    for c in range(P.shape[0]):
        out = _ProjectCamera.apply(mean, variance_q, variance_scale, opacity, color, P[c], K[c], width, height, clamp, L_max,
                                   capture_safe, with_depth, SH_FRAMES[sh_frame], splat)
        mean_xy, start, end, boxsize, index, keep = out[-6:]
        vinv, alpha, l_d = out[:3]
        grad_iter = keep if grad_iter is None else grad_iter | keep
        cam = None if index.numel() == 0 else {
            "boxsize": boxsize, "startpoint": start, "endpoint": end, "mean": mean_xy, "variance_inverse": vinv,
            "opacity": alpha, "l_d": l_d, "index": index}
        if cam is not None and with_depth:
            cam["depth"] = out[3]
        cams.append(cam)
    if grad_iter is None:
        grad_iter = torch.zeros(mean.shape[0], device=mean.device, dtype=torch.bool)
    return cams, grad_iter, (width, height)


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


class HipAdam:
    """torch.optim.Adam's update (default betas / eps, no weight decay, no amsgrad — what the reference constructs at
    gs_model.py:43-47) on the HIP library: one streaming kernel per parameter tensor (csrc/gcp_optim.hip, gcp_adam_step)
    instead of torch's multi-tensor launches (0.38 -> 0.2 ms per step at 10^6 Gaussians).  Same interface as far as the
    model uses it: `param_groups` with one tensor and an `lr` each, `step()`, `zero_grad()`."""

    def __init__(self, param_groups, betas=(0.9, 0.999), eps=1e-8):
        self.param_groups = [dict(g, params=list(g["params"]) if isinstance(g["params"], (list, tuple)) else [g["params"]])
                             for g in param_groups]
        self.betas, self.eps = betas, eps
        self.state = {}

    @torch.no_grad()
    def step(self):
        lib = _lib.load()
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("HipAdam updates contiguous float32 GPU tensors")
                st = self.state.setdefault(p, {"step": 0, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)})
                st["step"] += 1
                grad = p.grad.contiguous()
                with torch.cuda.device(p.device):
                    _lib.check(lib.gcp_adam_step(p.data_ptr(), grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                                 p.numel(), float(group["lr"]), self.betas[0], self.betas[1], self.eps, st["step"],
                                                 torch.cuda.current_stream(p.device).cuda_stream), "gcp_adam_step")

    def zero_grad(self, set_to_none=True):
        for group in self.param_groups:
            for p in group["params"]:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()


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
                 antialias=False):
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
        exists (the reference's checkout has no images.bin), the default is the reference's value for its own statistic."""
        super().__init__()
        if densify_on not in DENSIFY_ON:
            raise ValueError(f"densify_on: 'position' or 'screen', got {densify_on!r}")
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
        _splat_options(centres, cov_dilation, clamp_colour, antialias)
        self._L_max, self.sh_frame, self.active_sh_degree = L_max, sh_frame, active_sh_degree
        self.centres, self.cov_dilation, self.clamp_colour, self.antialias = centres, cov_dilation, clamp_colour, antialias
        self.reference_layout = reference_layout
        self.mean_grads_norm = torch.zeros(mean.shape[0], device=mean.device, dtype=torch.float32)
        self.mean_grads_iter = torch.zeros(mean.shape[0], device=mean.device, dtype=torch.int16)
        self.densify_on = densify_on
        self.screen_grads_norm = torch.zeros(mean.shape[0], device=mean.device, dtype=torch.float32)
        self.screen_grads_views = torch.zeros(mean.shape[0], device=mean.device, dtype=torch.int32)
        self.changing_optimizer()

    # ---- optimiser plumbing (reference: gs_model.py:43-67) -------------------------------------------------
    def changing_optimizer(self):
        groups = [{"params": p, "lr": float(self.lr[name])} for name, p in self.named_parameters(recurse=False)]
        # on the GPU one streaming kernel per tensor (torch's per-op Adam: 0.95 ms per step at 10^6 Gaussians, its fused
        # multi-tensor form 0.38, HipAdam 0.2)
        self._optimizer = HipAdam(groups) if self.mean.is_cuda else torch.optim.Adam(groups)

    def set_mean_lr(self, iteration):
        """The reference rebuilds Adam (and drops its moments) every step to change one rate (gs_control.py:195-197);
        here the rate of the `mean` group is updated in place."""
        self.lr["mean"] = self.mean_lr_setfunc(iteration)
        for group, (name, _) in zip(self._optimizer.param_groups, self.named_parameters(recurse=False)):
            if name == "mean":
                group["lr"] = float(self.lr["mean"])

    def train_step(self):
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
    def param_iter_update(self, grad_iter):
        if self.mean.grad is not None:
            self.mean_grads_norm += self.mean.grad.norm(dim=1)
            self.mean_grads_iter += grad_iter.to(torch.int16)

    def param_grads_per_iter_norm(self):
        return self.mean_grads_norm / (self.mean_grads_iter + (self.mean_grads_iter == 0).int())

    def _replace(self, keep, extra=None):
        """Keep rows `keep` of every per-Gaussian tensor and append `extra` (dict name -> rows)."""
        names = ("mean", "variance_q", "variance_scale", "opacity", "color")
        for name in names:
            rows = getattr(self, name).data[keep]
            if extra is not None:
                rows = torch.cat((rows, extra[name]), dim=0)
            setattr(self, name, torch.nn.Parameter(rows))
        for name in ("mean_grads_norm", "mean_grads_iter"):
            rows = getattr(self, name)[keep]
            if extra is not None:
                rows = torch.cat((rows, extra[name]), dim=0)
            setattr(self, name, rows)

    def _rows(self, mask, repeat=1):
        out = {k: getattr(self, k).data[mask].repeat(repeat, *([1] * (getattr(self, k).dim() - 1)))
               for k in ("mean", "variance_q", "variance_scale", "opacity", "color")}
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
        names = ("mean", "variance_q", "variance_scale", "opacity", "color")
        old = {k: getattr(self, k) for k in names}
        src = {k: old[k].data.contiguous() for k in names}
        dev, n = self.mean.device, self.mean.shape[0]
        norm, views = (t.contiguous() for t in self._density_stats())
        if norm.numel() != n or views.numel() != n:  # the active pair only: the other one is reallocated below
            raise RuntimeError("the densification statistic does not have one row per Gaussian")
        lib = _lib.load()
        count, offset = (torch.empty(k, dtype=torch.int32, device=dev) for k in (n, n + 1))
        action = torch.empty(n, dtype=torch.uint8, device=dev)
        ws = torch.empty(lib.gcp_densify_plan_workspace_bytes(n), dtype=torch.uint8, device=dev)
        seed = int(seed) & (2 ** 64 - 1)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.gcp_densify_plan(norm.data_ptr(), views.data_ptr(), src["variance_scale"].data_ptr(), src["opacity"].data_ptr(), n,
                                            float(self.grad_threshold), float(self.percent_dense * extent), float(0.1 * extent),
                                            float(self.prunning_min_opacity), int(n_split), count.data_ptr(), action.data_ptr(),
                                            offset.data_ptr(), ws.data_ptr(), ws.numel(), stream), "gcp_densify_plan")
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

            new = {k: rows(src[k], 0) for k in names}
            _lib.check(lib.gcp_densify_split(src["mean"].data_ptr(), src["variance_q"].data_ptr(), src["variance_scale"].data_ptr(),
                                             src_row.data_ptr(), kind.data_ptr(), offset.data_ptr(), n, m, int(n_split), seed & 0xFFFFFFFF,
                                             seed >> 32, new["mean"].data_ptr(), new["variance_scale"].data_ptr(), stream),
                       "gcp_densify_split")
            state = {}
            for k in names:
                st = self._optimizer.state.get(old[k])
                if st:
                    state[k] = {"step": st["step"], "exp_avg": rows(st["exp_avg"].contiguous(), 1),
                                "exp_avg_sq": rows(st["exp_avg_sq"].contiguous(), 1)}
        for k in names:
            setattr(self, k, torch.nn.Parameter(new[k]))
        self.changing_optimizer()
        for k, st in state.items():
            self._optimizer.state[getattr(self, k)] = st
        self.mean_grads_norm = torch.zeros(m, device=dev, dtype=torch.float32)
        self.mean_grads_iter = torch.zeros(m, device=dev, dtype=torch.int16)
        self.screen_grads_norm = torch.zeros(m, device=dev, dtype=torch.float32)
        self.screen_grads_views = torch.zeros(m, device=dev, dtype=torch.int32)
        return n, m

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
        (W/2, H/2), to `screen_grads_norm` and one view to `screen_grads_views` when `backward` reaches them."""
        if self.densify_on != "screen" or not torch.is_grad_enabled():
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("densify_on='screen' collects its statistic in autograd hooks, which a captured graph (cuda_kernel.GraphedStep) "
                               "does not replay: capture with densify_on='position'")
        scale = (0.5 * width, 0.5 * height)
        for cam in cams:
            if cam is not None and cam["mean"].requires_grad:
                cam["mean"].register_hook(lambda grad, index=cam["index"]: self._accumulate_centres(grad, index, scale))

    def _accumulate_centres(self, grad, index, scale):
        if self.screen_grads_norm.numel() != self.mean.shape[0]:
            raise RuntimeError("screen_grads_norm does not have one row per Gaussian: with densify_on='screen' densify with "
                               "densify_and_prune_device, which resizes it")
        accumulate_screen_grads(grad, index, scale, self.screen_grads_norm, self.screen_grads_views)

    # ---- forward (:277-460) ------------------------------------------------------------------------------------
    def camera_inputs(self, P, K, wh, with_depth=False, capture_safe=False):
        if capture_safe and self.densify_on == "screen":
            raise RuntimeError("densify_on='screen' does not support capture-safe lists: its statistic is collected per kept list entry")
        return camera_inputs(self.mean, self.variance_q, self.variance_scale, self.opacity, self.color, P, K, wh,
                             self.variance_pixel_tile_max_width, self.active_sh_degree, capture_safe=capture_safe,
                             with_depth=with_depth, sh_frame=self.sh_frame, centres=self.centres, cov_dilation=self.cov_dilation,
                             clamp_colour=self.clamp_colour, antialias=self.antialias)

    # ---- scene files (ply_io) ------------------------------------------------------------------------------------
    def save_ply(self, path, convention="3dgs"):
        """The scene as a standard 3DGS .ply (ply_io.save_ply).  Other renderers evaluate the SH basis on world-space
        directions: a model in the camera frame with an active degree > 0 is saved with a warning."""
        from . import ply_io

        if self.sh_frame != "world" and self.active_sh_degree > 0:
            import warnings

            warnings.warn("save_ply: this model evaluates its SH colour on camera-frame directions (sh_frame='camera'); other "
                          "renderers use world-space directions, so the view dependence of the saved scene will be wrong there")
        ply_io.save_ply(path, self.mean.data, self.variance_q.data, self.variance_scale.data, self.opacity.data, self.color.data,
                        convention=convention)

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

    def forward(self, P, K, wh, image_sample):
        cams, grad_iter, (width, height) = self.camera_inputs(P, K, wh)
        self._watch_centres(cams, width, height)
        images, names = [], []
        for cam, name in zip(cams, image_sample):
            if cam is None:
                continue  # nothing visible: the reference drops the image from the batch (:414-417)
            batch = cam["boxsize"].new_tensor([cam["boxsize"].numel()])
            images.append(custom_autograd_grouped_cumprod.apply(
                cam["boxsize"], batch, cam["startpoint"], cam["endpoint"], cam["mean"], cam["variance_inverse"],
                cam["opacity"], cam["l_d"], width, height))
            names.append(name)
        if not images:
            raise RuntimeError("no camera of the batch sees any Gaussian")  # the reference fails in torch.stack (:454)
        out = torch.stack(images, dim=0)[:, 1:, 1:, :]
        h, w = int(height), int(width)
        out = out.reshape(-1, 3, h, w) if self.reference_layout else out.permute(0, 3, 1, 2).contiguous()
        return [out, names, grad_iter]

    def render(self, P, K, wh, background=None, image_sample=None):
        """`forward` with the expected-depth and alpha maps and a background colour (`cuda_kernel.render`, whose
        docstring pins the definitions: depth = sum of the colour weights times the camera-space depth, NOT divided by
        alpha; alpha = 1 - the transmittance behind the pixel; image composited over `background`, a float[3] device tensor
        or None for black).  Returns [images (B, 3, H, W), depth (B, 1, H, W), alpha (B, 1, H, W), names, grad_iter], all
        maps after the same [1:, 1:] crop as `forward`; `names` are `image_sample`'s entries (default: camera indices) of the
        cameras that see anything — the others are dropped, as in `forward`."""
        cams, grad_iter, (width, height) = self.camera_inputs(P, K, wh, with_depth=True)
        self._watch_centres(cams, width, height)
        names_in = list(range(P.shape[0])) if image_sample is None else image_sample
        images, depths, alphas, names = [], [], [], []
        for cam, name in zip(cams, names_in):
            if cam is None:
                continue
            img, dep, alp = render(cam["startpoint"], cam["endpoint"], cam["mean"], cam["variance_inverse"], cam["opacity"],
                                   cam["l_d"], cam["depth"], width, height, background)
            images.append(img)
            depths.append(dep)
            alphas.append(alp)
            names.append(name)
        if not images:
            raise RuntimeError("no camera of the batch sees any Gaussian")
        images = torch.stack(images)[:, 1:, 1:, :].permute(0, 3, 1, 2).contiguous()
        depth = torch.stack(depths)[:, None, 1:, 1:].contiguous()
        alpha = torch.stack(alphas)[:, None, 1:, 1:].contiguous()
        return [images, depth, alpha, names, grad_iter]


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
