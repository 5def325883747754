"""Resampling a photograph through a lens's distortion into a pinhole camera (csrc/gcp_undistort.hip,
simplegaussiansplat_tk71_amd/lens.py) restated in float64 torch, and the cases its tests run on.  A helper, not a test.

Written from the published formulas — COLMAP's camera_models.h, OpenCV's calibration documentation — and independent of the
product: it imports neither `lens.distort` nor the kernel's record; a lens here is a plain dict.

    polynomial  r^2 = x^2 + y^2, radial = (1 + k1 r^2 + k2 r^4 + k3 r^6) / (1 + k4 r^2 + k5 r^4 + k6 r^6)
                x_d = x radial + 2 p1 x y + p2 (r^2 + 2 x^2),  y_d = y radial + p1 (r^2 + 2 y^2) + 2 p2 x y
    fisheye     theta = atan r, theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8), scale theta_d / r (1 at r = 0)
    output pixel (i, j): (x, y) = ((i + 0.5 - cx') / fx', (j + 0.5 - cy') / fy'); source coordinate (fx x_d + cx, fy y_d + cy),
    clamped to [0.5, W - 0.5] x [0.5, H - 0.5]; the value is the bilinear interpolation at (u - 0.5, v - 0.5) in pixel indexes.
"""
import torch

COORD_BOUND = 1e-3  # px: coordinates below 256 have a float32 spacing of 1.5e-5 px, the formula fewer than 40 roundings, each scaled
#                     by at most the coordinate: 1e-3 allows about 60
VALUE_BOUND = 4e-3  # neighbouring pixels differ by at most 1.0 and each axis is off by at most 1e-3: 2e-3, doubled — one grey level

SIZES = ((70, 37, 48.0), (97, 61, 66.0), (64, 64, 40.0))  # (W, H, f): odd width, no multiple of 64; two waves per row; one tile

# name -> (kind, k1..k6, p1, p2)
COEFFICIENTS = {
    "simple radial": ("polynomial", (-0.12, 0, 0, 0, 0, 0), (0, 0)),
    "radial": ("polynomial", (-0.2, 0.05, 0, 0, 0, 0), (0, 0)),
    "OpenCV": ("polynomial", (-0.115, 0.068, 0, 0, 0, 0), (-2.8e-4, 5.4e-3)),  # camera 1 of tests/golden/colmap_scene
    "pincushion": ("polynomial", (0.1, 0.02, 0, 0, 0, 0), (1e-3, -2e-3)),
    "full OpenCV": ("polynomial", (0.1, -0.05, 0.01, 0.12, -0.03, 0.005), (1e-3, 2e-3)),
    "fisheye": ("fisheye", (-0.03, 0.01, -0.002, 0.0005, 0, 0), (0, 0)),
}
FITTED = tuple(COEFFICIENTS)  # the six lenses that are used at their fitted scale; "identity" is used at scale 1


def make_lens(name, width, height, f, cx=None, cy=None):
    """A lens as a dict: fx = f, fy = 1.02 f, cx = W / 2 + 0.3, cy = H / 2 - 0.2 unless given."""
    kind, k, p = ("pinhole", (0.0,) * 6, (0.0, 0.0)) if name == "identity" else COEFFICIENTS[name]
    return {"kind": kind, "fx": float(f), "fy": 1.02 * f, "cx": width / 2 + 0.3 if cx is None else cx, "cy": height / 2 - 0.2 if cy is None else cy,
            "width": width, "height": height, "k": tuple(float(v) for v in k), "p": tuple(float(v) for v in p)}


def distort(lens, x, y):
    """Normalised ideal (x, y) float64 tensors -> normalised distorted (x_d, y_d)."""
    if lens["kind"] == "pinhole":
        return x, y
    r2 = x ** 2 + y ** 2
    k1, k2, k3, k4, k5, k6 = lens["k"]
    if lens["kind"] == "polynomial":
        p1, p2 = lens["p"]
        radial = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
        return x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x ** 2), y * radial + p1 * (r2 + 2 * y ** 2) + 2 * p2 * x * y
    assert lens["kind"] == "fisheye"
    r = torch.sqrt(r2)
    theta = torch.atan(r)
    theta_d = theta * (1 + k1 * theta ** 2 + k2 * theta ** 4 + k3 * theta ** 6 + k4 * theta ** 8)
    scale = torch.where(r > 0, theta_d / torch.where(r > 0, r, torch.ones_like(r)), torch.ones_like(r))
    return x * scale, y * scale


def source_coords(lens, scale, pixels=None):
    """The UNCLAMPED source coordinate (u, v), float64 (H, W) each, of the centre of every output pixel of the camera with the
    lens's size and principal point and the focal lengths scale fx, scale fy; `pixels` = (i, j) integer tensors: those only."""
    w, h = lens["width"], lens["height"]
    if pixels is None:
        j, i = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    else:
        i, j = (t.double() for t in pixels)
    x, y = (i + 0.5 - lens["cx"]) / (scale * lens["fx"]), (j + 0.5 - lens["cy"]) / (scale * lens["fy"])
    xd, yd = distort(lens, x, y)
    return lens["fx"] * xd + lens["cx"], lens["fy"] * yd + lens["cy"]


def inside(lens, u, v):
    return (u >= 0.5) & (u <= lens["width"] - 0.5) & (v >= 0.5) & (v <= lens["height"] - 0.5)


def border_pixels(width, height):
    """(i, j) of the pixels on the border."""
    j, i = torch.meshgrid(torch.arange(height), torch.arange(width), indexing="ij")
    edge = (i == 0) | (i == width - 1) | (j == 0) | (j == height - 1)
    return i[edge], j[edge]


def clamped_coords(lens, scale):
    """(u, v) clamped to the source's border pixel centres, and the bool map of the pixels the clamp moved."""
    u, v = source_coords(lens, scale)
    return u.clamp(0.5, lens["width"] - 0.5), v.clamp(0.5, lens["height"] - 0.5), ~inside(lens, u, v)


def undistort(photo, lens, scale):
    """photo float64 (3, H, W) -> the resampled (3, H, W): the four taps around the clamped coordinate."""
    w, h = lens["width"], lens["height"]
    u, v, _ = clamped_coords(lens, scale)
    u, v = u - 0.5, v - 0.5
    x0, y0 = u.floor().long().clamp(0, w - 1), v.floor().long().clamp(0, h - 1)
    x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
    wx, wy = u - x0, v - y0
    tap = lambda yy, xx: photo[:, yy, xx]  # noqa: E731
    return (1 - wy) * ((1 - wx) * tap(y0, x0) + wx * tap(y0, x1)) + wy * ((1 - wx) * tap(y1, x0) + wx * tap(y1, x1))


def ramp(width, height):
    """float32 (3, H, W): x + 0.5, y + 0.5 and x + y + 1 — linear, so bilinear interpolation returns the coordinate sampled."""
    j, i = torch.meshgrid(torch.arange(height, dtype=torch.float32), torch.arange(width, dtype=torch.float32), indexing="ij")
    return torch.stack([i + 0.5, j + 0.5, i + j + 1.0])


def random_bytes(n, width, height, seed):
    """uint8 (n, H, W, 3), uniform."""
    return torch.randint(0, 256, (n, height, width, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
