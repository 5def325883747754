"""The inputs of tests/test_normals_gpu.py, built here so that tests/test_normals.py (no GPU) builds them the same way and asserts
the margins that keep every row and pixel in every comparison: no tie between the two smallest log scales, no normal at right
angles to its view ray, no alpha near alpha_min."""
import math

import torch

ALPHA_MIN = 1e-3
TILE_W, TILE_H = 32, 16  # the consistency kernels' tile (csrc/gcp_normal.hip)
NORMAL_SIZES = (1, 64, 65, 1000)
FRAMES = ((3, 3), (2, 9), (5, 7), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (33, 65))  # (H, W)
BATCHES = (1, 3)


def random_rotation(g):
    q = torch.randn(4, generator=g, dtype=torch.float64)
    x, y, z, w = (q / q.norm()).tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


def normals_case(n, full, seed=0):
    """float32 CPU tensors (variance_q (n, 4), variance_scale (n, 3), mean (n, 3), P_c (3, 4), index int64 (m,), G (m, 3)): a
    list that is a permuted strict subset (m = 2n // 3; empty for n = 1) or, `full`, a permutation of all rows.  The quaternions
    are not normalised.  The two smallest log scales of a row differ by >= 0.1, and every centre is moved along its normal until
    |n_c . t_c| >= 0.15 |t_c|."""
    from tests.normal_torch import rotation, shortest_axis

    g = torch.Generator().manual_seed(1000 * seed + n)
    q = torch.randn(n, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True) * (1.5 + torch.rand(n, 1, generator=g))  # lengths in [1.5, 2.5]
    gaps =torch.stack([torch.zeros(n), 0.1 + torch.rand(n, generator=g), 1.2 + torch.rand(n, generator=g)], dim=1)
    order = torch.argsort(torch.rand(n, 3, generator=g), dim=1)
    scale = -3.0 + torch.rand(n, 1, generator=g) + torch.gather(gaps, 1, order)
    Rc = random_rotation(g)
    tvec = torch.tensor([0.2, -0.1, 5.0], dtype=torch.float64)
    qd = q.double() / q.double().norm(dim=1, keepdim=True)
    n_c = rotation(qd)[torch.arange(n), :, shortest_axis(scale.double())] @ Rc.T
    t_c = torch.randn(n, 3, generator=g).double() + tvec
    d = (n_c * t_c).sum(1) / t_c.norm(dim=1)
    push = torch.where(d.abs() < 0.1, torch.where(d < 0, -1.0, 1.0) * 0.3 * t_c.norm(dim=1), torch.zeros_like(d))
    t_c = t_c + push[:, None] * n_c
    mean = ((t_c - tvec) @ Rc).float()
    P_c = torch.cat([Rc, tvec[:, None]], dim=1).float()
    m = n if full else (2 * n) // 3
    index = torch.randperm(n, generator=g)[:m]
    return q, scale, mean, P_c, index, torch.randn(m, 3, generator=g)


def consistency_case(batch, height, width, seed=0):
    """float32 CPU maps (depth (B, 1, H, W), alpha, normal (B, 3, H, W), K (B, 3, 3)): alpha uniform in [0.3, 1] with ~8 % of the
    pixels at exactly 0 — among them, where the frame holds them, the corner pixels of the first tile, the first pixel of the
    tile diagonally behind it and a pixel next to the frame's edge —, depth = alpha * U(2, 5), normal = a random direction *
    alpha * U(0, 1), and a K of its own per image.  The 3 x 3 frame keeps its cross of five pixels: one defined pixel."""
    g = torch.Generator().manual_seed(7919 * seed + 131 * height + width + 17 * batch)
    alpha = 0.3 + 0.7 * torch.rand(batch, 1, height, width, generator=g)
    holes = torch.rand(batch, 1, height, width, generator=g) < 0.08
    if (height, width) == (3, 3):
        holes[:] = False
        holes[:, :, 0, 0] = True
        holes[:, :, 2, 2] = True
    else:
        for y, x in ((TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W), (height // 2, 1), (height // 2, width - 2)):
            if 0 <= y < height and 0 <= x < width:
                holes[:, :, y, x] = True
    alpha = torch.where(holes, torch.zeros_like(alpha), alpha)
    depth = alpha * (2.0 + 3.0 * torch.rand(batch, 1, height, width, generator=g))
    direction = torch.randn(batch, 3, height, width, generator=g)
    normal = direction / direction.norm(dim=1, keepdim=True) * alpha * torch.rand(batch, 1, height, width, generator=g)
    K = torch.zeros(batch, 3, 3)
    for b in range(batch):
        f = max(height, width) * (0.8 + 0.35 * b)
        K[b] = torch.tensor([[f, 0, width / 2 + 0.3 + b], [0, 1.1 * f, height / 2 - 0.2 - 0.5 * b], [0, 0, 1.0]])
    return depth, alpha, normal, K


def model_scene(seed=3, n_gauss=80, n_cam=2, width=33, height=25):
    """A small ring-camera scene for GS_model_with_param.render(normals=True): float32 CPU tensors
    {mean, variance_q, variance_scale, opacity, color, P, K, wh} and a target (n_cam, 3, H, W).  Flat Gaussians (one axis four
    to eight times shorter than the others, so the two smallest log scales are far apart), large enough to cover the frame."""
    from simplegaussiansplat_tk71_amd import synthetic
    from tests.normal_torch import gaussian_normals

    g = torch.Generator().manual_seed(seed)
    P, K, wh = synthetic.ring_cameras(n_cam, width, height)
    # a jittered 9 x 7 grid over the plane through the origin that faces the first camera (the second one, opposite, sees its
    # back), wide enough to fill the frame, so that every pixel lies in the core of some Gaussian and alpha stays far above
    # alpha_min; the other rows are scattered around the origin, in front of and behind the sheet
    right, down, fwd = P[0, 0, :3], P[0, 1, :3], P[0, 2, :3]
    a, b = torch.meshgrid(torch.linspace(-1.9, 1.9, 9), torch.linspace(-1.45, 1.45, 7), indexing="ij")
    sheet = a.reshape(-1, 1) * right + b.reshape(-1, 1) * down + 0.2 * torch.randn(63, 1, generator=g) * fwd
    mean = torch.cat([sheet + 0.08 * torch.randn(63, 3, generator=g), 0.4 * torch.randn(n_gauss - 63, 3, generator=g)])
    q = torch.randn(n_gauss, 4, generator=g)
    big = 0.3 + 0.15 * torch.rand(n_gauss, 3, generator=g)
    flat = torch.randint(0, 3, (n_gauss,), generator=g)
    big[torch.arange(n_gauss), flat] = big[torch.arange(n_gauss), flat] / (4.0 + 4.0 * torch.rand(n_gauss, generator=g))
    opacity = torch.logit(0.35 + 0.5 * torch.rand(n_gauss, 1, generator=g))
    color = torch.zeros(n_gauss, 9, 3)
    color[:, 0, :] = torch.rand(n_gauss, 3, generator=g) / 0.28209479177387814
    color[:, 1:4, :] = 0.2 * torch.randn(n_gauss, 3, 3, generator=g)
    for _ in range(100):  # by rejection: no normal within 0.08 of a right angle to its view ray, from any camera
        low = torch.zeros(n_gauss, dtype=torch.bool)
        for c in range(n_cam):
            dot = gaussian_normals(q.double(), torch.log(big).double(), mean.double(), P[c].double(), torch.arange(n_gauss))[3]
            low |= dot.abs() < 0.08
        if not bool(low.any()):
            break
        q = torch.where(low[:, None], torch.randn(n_gauss, 4, generator=g), q)
    target =torch.rand(n_cam, 3, height, width, generator=g)
    return {"mean": mean, "variance_q": q, "variance_scale": torch.log(big), "opacity": opacity, "color": color, "P": P, "K": K, "wh": wh,
            "target": target}


TILE_MAX_WIDTH = math.log(0.04 / 0.96)  # GS_model_with_param's default box clamp, as the oracle takes it
PARAMS = ("mean", "variance_q", "variance_scale", "opacity", "color")
NORMAL_WEIGHT, DISTORTION_WEIGHT = 0.05, 0.1


def model_phi(sc):
    """The 3-D filter's size per Gaussian for the scene's cameras, float32: tests/filter3d_torch.py's rate in float64 through
    filter3d.filter_from_rate (plain torch)."""
    from simplegaussiansplat_tk71_amd.filter3d import filter_from_rate
    from tests import filter3d_torch as ft

    return filter_from_rate(ft.rate(sc["mean"], sc["P"], sc["K"], sc["wh"])["rate"].float())


def model_reference(sc, phi=None, distortion=False):
    """splat_loss + NORMAL_WEIGHT * normal_consistency (+ DISTORTION_WEIGHT * mean distortion) of the scene through
    oracle/gs_forward_torch.camera_inputs (float32, as the model's projection decides its boxes), the dense float64 renderers and
    tests/normal_torch.py -> {"loss", "grads": {name: float64}, "alpha", "depth" (C, 1, H, W), "normal" (C, 3, H, W),
    "dots": per camera n_c . t_c / |t_c| of its list}.  `phi`: the 3-D filter's sizes (float32), applied to what the projection
    sees; the normals take the raw parameters."""
    from oracle import gs_forward_torch as gft
    from oracle import loss_torch
    from tests import filter3d_torch as ft
    from tests import normal_torch as nt
    from tests.distortion_torch import dense_render_distortion
    from tests.test_render_depth_gpu import dense_render_depth

    P, K, wh = sc["P"], sc["K"], sc["wh"]
    wd, h = int(wh[0, 0]), int(wh[0, 1])
    leaves = {k: sc[k].clone().requires_grad_(True) for k in PARAMS}
    vs, op = leaves["variance_scale"], leaves["opacity"]
    if phi is not None:
        v2, x2 = ft.apply_stable(vs.double(), op.double()[:, 0], phi.double())
        vs, op = v2.float(), x2[:, None].float()
    cams, _, _ = gft.camera_inputs(leaves["mean"], leaves["variance_q"], vs, op, leaves["color"], P, K, wh, TILE_MAX_WIDTH)
    assert all(cam is not None for cam in cams)
    images, depths, alphas, dists, nmaps, dots = [], [], [], [], [], []
    for c, cam in enumerate(cams):
        zc = (leaves["mean"] @ P[c, 2, :3] + P[c, 2, 3])[cam["index"]].double()
        n, _, _, dot = nt.gaussian_normals(leaves["variance_q"].double(), leaves["variance_scale"].double(), leaves["mean"].double(),
                                           P[c].double(), cam["index"])
        args = (cam["startpoint"], cam["endpoint"], cam["mean"], cam["variance_inverse"].double(), cam["opacity"].double())
        if distortion:
            img, dep, alp, dist, _ = dense_render_distortion(*args, cam["l_d"].double(), zc, wd, h)
            dists.append(dist)
        else:
            img, dep, alp = dense_render_depth(*args, cam["l_d"].double(), zc, wd, h)
        nmaps.append(dense_render_depth(*args, n, zc, wd, h)[0])
        images.append(img), depths.append(dep), alphas.append(alp), dots.append(dot)
    chw = lambda maps: torch.stack(maps)[:, 1:, 1:, :].permute(0, 3, 1, 2)  # noqa: E731
    plane = lambda maps: torch.stack(maps)[:, None, 1:, 1:]  # noqa: E731
    image, normal, depth, alpha = chw(images), chw(nmaps), plane(depths), plane(alphas)
    loss = loss_torch.splat_loss(image, sc["target"].double(), 0.2) + NORMAL_WEIGHT * nt.normal_consistency(depth, alpha, normal, K.double())[0]
    if distortion:
        loss = loss + DISTORTION_WEIGHT * plane(dists).mean()
    loss.backward()
    return {"loss": loss.detach(), "grads": {k: leaves[k].grad.double() for k in PARAMS}, "alpha": alpha.detach(), "depth": depth.detach(),
            "normal": normal.detach(), "dots": dots, "image": image.detach()}
