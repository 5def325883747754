"""The camera projection: 3-D Gaussians + cameras -> the depth-ordered, culled inputs of the rasterise-and-blend Function.

`camera_inputs` (reference: gs_model.py:277-425) on the HIP library: per camera one forward kernel, the library's stable
radix sort on the depth keys and one gather; one backward kernel (`_ProjectCamera`).  Two kernel families: the reference's
conventions (csrc/gcp_project.hip) and, when an option of `splat_options` is not at its default, float centres, covariance
dilation, colour clamp and opacity compensation (csrc/gcp_splat.hip).

The projection is pinned, through its PyTorch restatement in oracle/gs_forward_torch.py, against the reference's own
forward run on CPU (tests/golden/forward_golden.npz: the arguments the reference hands to
`custom_autograd_grouped_cumprod.apply`).  Differences, all deliberate:
  * the 3-sigma box comes from a closed-form 2x2 eigen-decomposition on the device; the reference moves every
    covariance to the CPU for `torch.linalg.eigh` and back (gs_model.py:327-332).  For a positive semi-definite
    matrix `V^2 |lambda|` is just its diagonal, so the box is 3*sqrt(diag) exactly;
  * the depth sort is stable (the reference's `torch.argsort`, :356, leaves ties undefined);
  * the SH colour stands in for the reference's `sh_utility.eval_sh`, which is not in its checkout
    (gs_model.py:9,335): real spherical harmonics up to degree 3 in the usual 3DGS order and sign — parity unpinned.
    The direction they are evaluated on is, by default, the reference's: -t/|t| in CAMERA coordinates (:335-338), so a
    Gaussian changes colour when the camera rolls; `sh_frame="world"` uses the world-space unit vector from the camera
    centre to the Gaussian, the convention of other 3DGS renderers (what a scene saved with `save_ply` needs);
  * the whole per-Gaussian chain is ONE HIP kernel per camera and direction (`gcp_project_forward`,
    `gcp_project_backward`, csrc/gcp_project.hip) instead of ~150 PyTorch kernels: at 10^6 Gaussians the reference's
    formulation costs 64 ms forward + 110 ms backward around a 1.8 ms Function.  That formulation is kept, as the
    checker the kernels are tested against, in oracle/gs_forward_torch.py — not here: there is no CPU path (CPU
    tensors raise).
"""
import math
import numbers
from typing import NamedTuple

import torch

from . import _lib
from . import raster as _raster

SH_FRAMES = {"camera": 0, "world": 1}
CENTRES = ("pixel", "subpixel")


class SplatOptions(NamedTuple):
    """What the kernels of csrc/gcp_splat.hip take beyond those of csrc/gcp_project.hip (see `camera_inputs`)."""
    subpixel: bool
    cov_eps: float
    clamp_colour: bool
    antialias: bool

    @property
    def flags(self):
        """The GCP_SPLAT_* word of gcp_splat_forward_flags / gcp_splat_backward_flags."""
        return (_lib.SPLAT_CLAMP_COLOUR if self.clamp_colour else 0) | (_lib.SPLAT_ANTIALIAS if self.antialias else 0)

    @property
    def mean_offset(self):
        """What the forward adds to the projected centre: half a pixel for float centres (see `camera_inputs`)."""
        return 0.5 if self.subpixel else 0.0


def splat_options(centres, cov_dilation, clamp_colour, antialias=False):
    """The validated options of `camera_inputs` as a `SplatOptions`, or None where all are at their defaults (the kernels of
    csrc/gcp_project.hip; an explicit cov_dilation, 1e-6 included, is not the default); ValueError before anything touches
    the GPU."""
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
    if centres == "pixel" and cov_dilation is None and not clamp_colour:
        return None
    return SplatOptions(centres == "subpixel", float(cov_eps), clamp_colour, antialias)


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
    splat=a `SplatOptions`: the kernels of csrc/gcp_splat.hip (gcp_splat_forward_flags, gcp_splat_gather,
    gcp_splat_backward_flags): `cov_eps` on the diagonal of the pixel covariance; `flags` = GCP_SPLAT_CLAMP_COLOUR (the SH
    colour clamped at 0, `clamp_colour`) | GCP_SPLAT_ANTIALIAS (alpha is sigmoid(opacity) rho, rho = sqrt(det Sigma /
    det Sigma'), `antialias`); and — `subpixel` — the pixel centre kept as float32 (m, 2) at px + `mean_offset` = px + 0.5,
    differentiable: its gradient is handed to the backward as grad_mean_xy.  Not `subpixel`: the centre is truncated as by
    default and returned as int32 without a gradient (the box still goes around the untruncated centre, by the rule of the
    float one).
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
        # the family: its entry points, what its forward takes after box_clamp, whether its gather has a depth argument
        if splat is None:
            project, project_name, options = lib.gcp_project_forward_sh, "gcp_project_forward", ()
            gather_name, depth_slot = ("gcp_project_gather_depth", True) if with_depth else ("gcp_project_gather", False)
        else:
            project, project_name = lib.gcp_splat_forward_flags, "gcp_splat_forward_flags"
            options = (splat.cov_eps, splat.mean_offset, splat.flags)
            gather_name, depth_slot = "gcp_splat_gather", True  # NULL without with_depth
        subpixel = splat is not None and splat.subpixel
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
        record, sort_key, row_of = f32(n, 16), i32(n), i32(n)
        keep = torch.empty(n, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            world = (*(t.data_ptr() for t in args), n, L_max, color.shape[1], sh_frame, width, height, box_clamp)
            made = (record.data_ptr(), sort_key.data_ptr(), keep.data_ptr(), row_of.data_ptr(), stream)
            _lib.check(project(*world, *options, *made), project_name)
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
            depth_arg = (depth.data_ptr() if with_depth else None,) if depth_slot else ()
            _lib.check(getattr(lib, gather_name)(*lists, *depth_arg, *rows), gather_name)
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
        subpixel = splat is not None and splat.subpixel
        grads = [torch.empty_like(t) for t in (mean, variance_q, variance_scale, opacity, color)]  # every row is written
        g = [t.contiguous().float() for t in (g_vinv, g_alpha, g_ld, *rest[:int(ctx.with_depth) + int(subpixel)])]
        g_depth = g[3].data_ptr() if ctx.with_depth else None
        lib = _lib.load()
        # the family: its entry point and what it takes between the upstream gradients and the outputs
        if splat is None:
            backward, name, options = lib.gcp_project_backward_sh, "gcp_project_backward", ()
        else:
            backward, name = lib.gcp_splat_backward_flags, "gcp_splat_backward_flags"
            options = (splat.cov_eps, splat.flags, g[-1].data_ptr() if subpixel else None)
        with torch.cuda.device(mean.device):
            upstream = (*(t.data_ptr() for t in args), mean.shape[0], ctx.L_max, color.shape[1], ctx.sh_frame, row_of.data_ptr(),
                        *(t.data_ptr() for t in g[:3]), g_depth)
            made = (*(t.data_ptr() for t in grads), torch.cuda.current_stream(mean.device).cuda_stream)
            _lib.check(backward(*upstream, *options, *made), name)
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
    splat = splat_options(centres, cov_dilation, clamp_colour, antialias)  # None: the defaults, on the kernels of csrc/gcp_project.hip
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
