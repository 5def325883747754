"""Lens distortion: the photographs of a COLMAP model resampled, once, into ideal pinhole cameras (csrc/gcp_undistort.hip) —
what upstream 3DGS gets from `colmap image_undistorter` before training, without a COLMAP binary.

`lens_from_colmap` turns a camera of `colmap_io.read_cameras` into a `Lens`; `fit_pinhole` chooses the output camera — the
source's size and principal point, the focal lengths scaled so that the field of view is the widest that leaves no output
pixel without a source (COLMAP's blank_pixels = 0) —; `undistort` resamples a batch of photographs, each through its own lens,
in one HIP launch.  Nothing downstream changes: the model, the loss and the metrics only ever see K and the targets.

`distort` and `fit_pinhole` are float64 on the host; `undistort` takes GPU tensors only: there is no CPU path.

Not here: distortion inside the projection (training on the raw photographs), an output size other than the
source's, downscaling, and COLMAP's FOV and THIN_PRISM_FISHEYE models."""
import math
from typing import NamedTuple, Tuple

import numpy as np
import torch

from . import _lib

KINDS = _lib.LENS_KINDS  # "pinhole", "polynomial", "fisheye": the record's kind word is the index


class Lens(NamedTuple):
    """One camera's intrinsics and distortion.  `kind` "polynomial": the rational radial model with tangential terms, with
    r^2 = x^2 + y^2 and radial = (1 + k1 r^2 + k2 r^4 + k3 r^6) / (1 + k4 r^2 + k5 r^4 + k6 r^6),
        x_d = x radial + 2 p1 x y + p2 (r^2 + 2 x^2),   y_d = y radial + 2 p2 x y + p1 (r^2 + 2 y^2).
    "fisheye": the equidistant polynomial, theta = atan r, theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),
    (x_d, y_d) = (x, y) theta_d / r and (x, y) at r = 0.  "pinhole": none.  `k` = (k1..k6), `p` = (p1, p2)."""
    kind: str
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int
    k: Tuple[float, float, float, float, float, float] = (0.0,) * 6
    p: Tuple[float, float] = (0.0, 0.0)


# COLMAP model -> (kind, what its parameters after the focal lengths and the principal point are, in the file's order):
# the orders of COLMAP's camera_models.h
_COLMAP = {"SIMPLE_PINHOLE": ("pinhole", ()), "PINHOLE": ("pinhole", ()),
           "SIMPLE_RADIAL": ("polynomial", ("k1",)), "RADIAL": ("polynomial", ("k1", "k2")),
           "OPENCV": ("polynomial", ("k1", "k2", "p1", "p2")),
           "FULL_OPENCV": ("polynomial", ("k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6")),
           "OPENCV_FISHEYE": ("fisheye", ("k1", "k2", "k3", "k4")), "SIMPLE_RADIAL_FISHEYE": ("fisheye", ("k1",)),
           "RADIAL_FISHEYE": ("fisheye", ("k1", "k2"))}


def lens_from_colmap(camera):
    """A camera dict of `colmap_io.read_cameras` (model, width, height, params) -> `Lens`.  FOV and THIN_PRISM_FISHEYE are
    not modelled: ValueError."""
    from .colmap_io import _SINGLE_FOCAL

    model, params = camera["model"], [float(v) for v in camera["params"]]
    if model not in _COLMAP:
        raise ValueError(f"COLMAP camera model {model}: its distortion is not modelled (supported: {', '.join(_COLMAP)})")
    kind, order = _COLMAP[model]
    if model in _SINGLE_FOCAL:
        (f, cx, cy), rest = params[:3], params[3:]
        fx = fy = f
    else:
        (fx, fy, cx, cy), rest = params[:4], params[4:]
    if len(rest) != len(order):
        raise ValueError(f"COLMAP camera model {model}: {len(order)} distortion parameters expected, got {len(rest)}")
    k, p = [0.0] * 6, [0.0] * 2
    for name, value in zip(order, rest):
        (k if name[0] == "k" else p)[int(name[1]) - 1] = value
    return Lens(kind, fx, fy, cx, cy, int(camera["width"]), int(camera["height"]), tuple(k), tuple(p))


def distort(lens, xy):
    """Normalised ideal coordinates (..., 2) -> normalised distorted coordinates, float64 on the host (numpy)."""
    xy = np.asarray(xy, dtype=np.float64)
    x, y = xy[..., 0], xy[..., 1]
    if lens.kind == "pinhole":
        return np.stack([x, y], axis=-1)
    r2 = x * x + y * y
    k1, k2, k3, k4, k5, k6 = lens.k
    if lens.kind == "polynomial":
        p1, p2 = lens.p
        radial = (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)))
        return np.stack([x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x),
                         y * radial + 2.0 * p2 * x * y + p1 * (r2 + 2.0 * y * y)], axis=-1)
    if lens.kind != "fisheye":
        raise ValueError(f"kind: one of {KINDS}, got {lens.kind!r}")
    r = np.sqrt(r2)
    theta = np.arctan(r)
    t2 = theta * theta
    theta_d = theta * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
    scale = np.where(r > 0, theta_d / np.where(r > 0, r, 1.0), 1.0)
    return np.stack([x * scale, y * scale], axis=-1)


def _border_centres(width, height):
    """The centres (i + 0.5, j + 0.5) of the pixels on the border of a width x height image, (m, 2)."""
    i, j = np.arange(width) + 0.5, np.arange(height) + 0.5
    return np.concatenate([np.stack([i, np.full(width, 0.5)], 1), np.stack([i, np.full(width, height - 0.5)], 1),
                           np.stack([np.full(height, 0.5), j], 1), np.stack([np.full(height, width - 0.5), j], 1)])


def fit_pinhole(lens, min_scale=0.2, max_scale=2.0):
    """-> (K_out float64 (3, 3) tensor, scale): the output camera has the source's size and principal point and the focal
    lengths scale fx, scale fy, `scale` being the smallest value in [min_scale, max_scale] (bisection in float64 down to an
    interval of 1e-9; its upper end is returned) at which the centre of every border pixel of the output maps to a source
    coordinate inside [0.5, W - 0.5] x [0.5, H - 0.5]: the widest field of view without a blank pixel, COLMAP's blank_pixels = 0.
    ValueError if `max_scale` itself leaves one."""
    _check_lens(lens)
    border = _border_centres(lens.width, lens.height)
    centre, focal = np.array([lens.cx, lens.cy]), np.array([lens.fx, lens.fy])

    def covered(scale):
        uv = distort(lens, (border - centre) / (scale * focal)) * focal + centre
        return bool(((uv[:, 0] >= 0.5) & (uv[:, 0] <= lens.width - 0.5) & (uv[:, 1] >= 0.5) & (uv[:, 1] <= lens.height - 0.5)).all())

    lo, hi = float(min_scale), float(max_scale)
    if not (0 < lo <= hi and math.isfinite(hi)):
        raise ValueError(f"0 < min_scale <= max_scale expected, got {min_scale}, {max_scale}")
    if not covered(hi):
        raise ValueError(f"max_scale = {max_scale} leaves blank pixels: this lens needs a narrower output camera")
    if covered(lo):
        hi = lo
    while hi - lo >= 1e-9:
        mid = 0.5 * (lo + hi)
        if covered(mid):
            hi = mid
        else:
            lo = mid
    K = torch.tensor([[hi * lens.fx, 0.0, lens.cx], [0.0, hi * lens.fy, lens.cy], [0.0, 0.0, 1.0]], dtype=torch.float64)
    return K, hi


def _check_lens(lens):
    if lens.kind not in KINDS:
        raise ValueError(f"kind: one of {KINDS}, got {lens.kind!r}")
    if len(lens.k) != 6 or len(lens.p) != 2:
        raise ValueError(f"a lens holds six radial and two tangential coefficients, got {len(lens.k)} and {len(lens.p)}")
    if not all(math.isfinite(v) and v > 0 for v in (lens.fx, lens.fy)):
        raise ValueError(f"focal lengths: finite and positive, got {lens.fx}, {lens.fy}")
    if not all(math.isfinite(v) for v in (lens.cx, lens.cy, *lens.k, *lens.p)):
        raise ValueError(f"a lens's principal point and coefficients must be finite, got {lens}")
    if lens.width < 1 or lens.height < 1:
        raise ValueError(f"a lens's size: at least 1 x 1, got {lens.width} x {lens.height}")


def lens_records(lenses, K_out):
    """The device records of the header (GCP_LENS_WORDS floats per image) as a float32 CPU tensor (n, GCP_LENS_WORDS);
    K_out float64 (n, 3, 3) on the CPU."""
    rows = [[lens.fx, lens.fy, lens.cx, lens.cy, 0.0, 0.0, 0.0, 0.0, *lens.k, *lens.p, float(KINDS.index(lens.kind)), 0.0, 0.0, 0.0]
            for lens in lenses]
    rec = torch.tensor(rows, dtype=torch.float64).reshape(len(rows), _lib.LENS_WORDS)
    rec[:, 4:8] = torch.stack([K_out[:, 0, 0], K_out[:, 1, 1], K_out[:, 0, 2], K_out[:, 1, 2]], dim=1)
    return rec.float()


def undistort(photos, lenses, K_out):
    """Photographs through `lenses` -> the photographs an ideal pinhole camera `K_out` would have taken, float32 (n, 3, H, W).
    photos: uint8 (n, H, W, 3) — what a JPEG decodes to; the result is divided by 255 — or float32 (n, 3, H, W), on the GPU.
    lenses: one `Lens` per image, of the photographs' size.  K_out: (n, 3, 3) or one (3, 3) for all, any float type on any
    device (`fit_pinhole`); its focal lengths and principal point are read, the skew is ignored.
    Output pixel (i, j) is the bilinear sample of the source at the point its centre's ray meets after the distortion; rays
    that leave the source repeat its edge.  One HIP launch for the batch (gcp_undistort_u8 / gcp_undistort_f32), every image
    independent of the others bit for bit.  Refused before the library is touched: CPU tensors, other shapes or types, a lens
    whose size is not the photographs', and focal lengths that are not finite and positive."""
    if not torch.is_tensor(photos) or photos.dim() != 4:
        raise RuntimeError("undistort expects photos as one tensor, uint8 (n, H, W, 3) or float32 (n, 3, H, W)")
    if photos.dtype == torch.uint8 and photos.shape[3] == 3:
        n, height, width = photos.shape[:3]
    elif photos.dtype == torch.float32 and photos.shape[1] == 3:
        n, height, width = photos.shape[0], photos.shape[2], photos.shape[3]
    else:
        raise RuntimeError(f"undistort expects uint8 (n, H, W, 3) or float32 (n, 3, H, W), got {photos.dtype} {tuple(photos.shape)}")
    if height < 1 or width < 1:
        raise RuntimeError(f"undistort expects photographs of at least 1 x 1, got {width} x {height}")
    lenses = list(lenses)
    if len(lenses) != n:
        raise RuntimeError(f"one lens per photograph expected: {len(lenses)} lenses for {n} photographs")
    K_out = torch.as_tensor(K_out).detach().to(device="cpu", dtype=torch.float64)
    if tuple(K_out.shape) == (3, 3):
        K_out = K_out.expand(n, 3, 3)
    if tuple(K_out.shape) != (n, 3, 3):
        raise RuntimeError(f"K_out: (n, 3, 3) or (3, 3) expected, got {tuple(K_out.shape)}")
    for i, lens in enumerate(lenses):
        try:
            _check_lens(lens)
        except ValueError as e:
            raise RuntimeError(f"lens {i}: {e}") from e
        if (lens.width, lens.height) != (width, height):
            raise RuntimeError(f"lens {i} is of a {lens.width} x {lens.height} camera, the photographs are {width} x {height}")
    focal = torch.stack([K_out[:, 0, 0], K_out[:, 1, 1]], dim=1)
    if n and not bool((torch.isfinite(focal) & (focal > 0)).all()):
        raise RuntimeError("K_out: focal lengths must be finite and positive")
    if n and not bool(torch.isfinite(K_out[:, :2, 2]).all()):
        raise RuntimeError("K_out: the principal point must be finite")
    if not photos.is_cuda:
        raise RuntimeError("undistort is a HIP kernel: the photographs must live on the GPU (no CPU path)")
    dev = photos.device
    src = photos.detach().contiguous()
    out = torch.empty((n, 3, height, width), dtype=torch.float32, device=dev)
    records = lens_records(lenses, K_out).to(dev)
    fn, name = (_lib.load().gcp_undistort_u8, "gcp_undistort_u8") if src.dtype == torch.uint8 else (_lib.load().gcp_undistort_f32, "gcp_undistort_f32")
    with torch.cuda.device(dev):
        _lib.check(fn(src.data_ptr(), records.data_ptr(), n, height, width, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), name)
    return out
