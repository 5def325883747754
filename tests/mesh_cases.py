"""The inputs of tests/test_tsdf_gpu.py, built on the CPU so that tests/test_mesh_cabi.py can check their conditions without a GPU:
three `synthetic.ring_cameras` at 24 x 16 looking at a sphere of radius 0.8 whose depth maps are analytic, and small volumes
around it.  alpha is 0 (a miss) or in [0.6, 1]: nothing is marginal at alpha_min = 0.5.  Origins and voxels are irrational-
looking so that few lattice points project onto a pixel boundary."""
import functools

import numpy as np
import torch

from simplegaussiansplat_tk71_amd.synthetic import ring_cameras
from tests import mesh_ref as mr

WIDTH, HEIGHT, RADIUS, CAMERA_RADIUS = 24, 16, 0.8, 3.2
ALPHA_MIN = 0.5

TSDF_CASES = [
    dict(id="13x7x5", dims=(13, 7, 5), origin=(-1.0371, -0.6113, -0.4337), voxel=0.17139, trunc=0.41, depth_max=0.0, colour=True),
    dict(id="70x3x2", dims=(70, 3, 2), origin=(-1.0457, -0.0319, -0.0173), voxel=0.030173, trunc=0.13, depth_max=0.0, colour=True),
    dict(id="holes", dims=(13, 7, 5), origin=(-1.0371, -0.6113, -0.4337), voxel=0.17139, trunc=0.41, depth_max=0.0, colour=True, holes=True),
    dict(id="depth_max", dims=(13, 7, 5), origin=(-1.0371, -0.6113, -0.4337), voxel=0.17139, trunc=0.41, depth_max=2.8, colour=False),
    dict(id="behind", dims=(13, 7, 5), origin=(-1.0371, -0.6113, -0.4337), voxel=0.17139, trunc=0.41, depth_max=0.0, colour=False,
         expect_behind=True),
]


def sphere_maps(P, K, width=WIDTH, height=HEIGHT, radius=RADIUS):
    """Analytic maps of the sphere |x| = radius -> (depth (B, 1, H, W) = z alpha, alpha (B, 1, H, W), image (B, 3, H, W)),
    float32: z the camera-space depth of the first intersection of the ray through the pixel centre."""
    P, K = P.double(), K.double()
    y, x = torch.meshgrid(torch.arange(height, dtype=torch.float64), torch.arange(width, dtype=torch.float64), indexing="ij")
    depth, alpha, image = [], [], []
    for c in range(P.shape[0]):
        R, t = P[c, :, :3], P[c, :, 3]
        eye = -R.T @ t
        ray = torch.stack([(x + 0.5 - K[c, 0, 2]) / K[c, 0, 0], (y + 0.5 - K[c, 1, 2]) / K[c, 1, 1], torch.ones_like(x)], dim=-1) @ R  # R^T r
        a2, b, c0 = (ray * ray).sum(-1), (ray @ eye), float(eye @ eye) - radius * radius
        disc = b * b - a2 * c0
        hit = (disc > 0) & (-b > 0)
        z = torch.where(hit, (-b - disc.clamp_min(0).sqrt()) / a2, torch.zeros_like(b))
        a = torch.where(hit, 0.6 + 0.4 * (0.5 + 0.5 * torch.sin(1.7 * x + 0.9 * y + c)), torch.zeros_like(b))
        depth.append((z * a)[None])
        alpha.append(a[None])
        image.append(torch.stack([0.5 + 0.5 * torch.sin(0.3 * x + c), 0.5 + 0.5 * torch.cos(0.4 * y - c), (x + y) / (width + height)]))
    return torch.stack(depth).float(), torch.stack(alpha).float(), torch.stack(image).float()


@functools.lru_cache(maxsize=None)
def _inputs(case_id):
    case = next(c for c in TSDF_CASES if c["id"] == case_id)
    P, K, _ = ring_cameras(3, WIDTH, HEIGHT, radius=CAMERA_RADIUS)
    out = {"behind": 0, "grazing": 0}
    if case.get("expect_behind"):
        # camera 0 looks along +z from inside the volume: its z = 0 plane lies 5e-5 in front of the lattice plane k = 2
        ox, oy, oz = (float(np.float32(v)) for v in case["origin"])
        plane = float(np.float32(oz) + np.float32(case["voxel"]) * np.float32(2))
        P = P.clone()
        P[0] = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, -plane + 5e-5]])
        z = mr.lattice(case["dims"], (ox, oy, oz), float(np.float32(case["voxel"])))[..., 2] + float(P[0, 2, 3])
        out["behind"], out["grazing"] = int((z < 0).sum()), int(((z > 0) & (z < 1e-4)).sum())
    depth, alpha, image = sphere_maps(P, K)
    if case.get("holes"):
        depth, alpha = depth.clone(), alpha.clone()
        depth[0, 0, 6:10, 9:12] = float("nan")
        depth[1, 0, 7:9, 10:14] = 0.0
        depth[1, 0, 5:7, 10:14] = -1.0
        alpha[2, 0, 6:9, 11:13] = float("nan")
        depth[2, 0, 9:11, 11:13] = float("inf")
        alpha[2, 0, 9:11, 11:13] = 0.0
    out.update(P=P, K=K, depth=depth, alpha=alpha, image=image)
    return out


def tsdf_inputs(case):
    return _inputs(case["id"])


@functools.lru_cache(maxsize=None)
def _reference(case_id):
    case = next(c for c in TSDF_CASES if c["id"] == case_id)
    inp = _inputs(case_id)
    nx, ny, nz = case["dims"]
    state = (torch.ones(nz, ny, nx, dtype=torch.float64), torch.zeros(nz, ny, nx, dtype=torch.float64),
             torch.zeros(3, nz, ny, nx, dtype=torch.float64) if case["colour"] else None)
    return mr.integrate(state, case["dims"], case["origin"], case["voxel"], case["trunc"], inp["depth"], inp["alpha"], inp["P"], inp["K"],
                        image=inp["image"] if case["colour"] else None, alpha_min=ALPHA_MIN, depth_max=case["depth_max"])


def tsdf_reference(case, inputs=None):
    """-> ((tsdf, weight, rgb or None) float64, marginal bool, scale float64); computed once per case and shared: do not write
    into it."""
    return _reference(case["id"])


def slab_weight(shape):
    """Weights (nz, ny, nx) with an unobserved slab of two lattice planes across x."""
    w = np.ones(shape, dtype=np.float32)
    w[:, :, 8:10] = 0.0
    return w

