"""Every Gaussian's row of every gradient of the blend's four maps, and every pixel of the depth and distortion maps, against the
float64 closed form of tests/blend_rows_torch.py, each within its own condition scale:

    |got_i - want_i|_inf <= 2e-5 * scale_i + 4 * |f32_i - want_i|_inf

(2e-5: test_raster_gpu.py::test_deep_pixel_columns_relative_gradient_accuracy's number for the colour path; f32: the same
closed form run in float32 on the CPU — the distortion in its pair form — i.e. what float32 can deliver; a row whose float64
value and scale are exactly zero must be exactly zero).  tests/test_render_depth_gpu.py and tests/test_distortion_gpu.py hold
the same kernels to 2e-4 of the LARGEST gradient of the scene, which the front layers set: a semi-occluded Gaussian could be
wholly wrong there.  tests/test_blend_rows.py checks on the CPU that the closed form is the autograd oracles' and that the
measured term stays a round-off term on every scene of this file.

Scenes: one to four 16x16 tiles, the smallest at which the walk changes branch — stacks of n layers over one tile with n around
kStageBwd = 32 and kStage = 256, the golden deep stacks, T_N == 0 by underflow, T_N at the edge of float32, an exactly opaque
layer, a 17 x 17 frame (four tiles, three partly outside the frame, one a single pixel wide) and sub-pixel means with opacity-1
Gaussians.  Depths, ascending in list order: spread over [0.5, 20.5] as the older tests draw them, and CLUSTERED — a surface
dz thick at depth z0 — which is where the distortion regulariser works and where z_k A - B cancels.  Each test prints a ROWS
line per leaf."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.blend_rows_torch import blend_rows
from tests.test_render_depth_gpu import golden_stack, opaque_layer_scene, random_grads, stack_scene
from tests.util import TOL, make_scene

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
RTOL, MARGIN = 2e-5, 4.0
BG = torch.tensor([0.9, 0.35, 0.6])
CLUSTERS = {"z20_1": (20.0, 1.0), "z20_1e-2": (20.0, 1e-2), "z100_1e-2": (100.0, 1e-2), "z5_1e-3": (5.0, 1e-3)}
DEPTH_SETS = ("spread", *CLUSTERS, "two_clusters")
STACK_SIZES = (31, 32, 33, 64, 65, 255, 256, 257, 700)
DIST_LEAVES = ("vinv", "opacity", "z")


def depths(kind, n, seed=1):
    """float32 depths of `n` layers, ascending.  spread: 0.5 + 20 rand; a cluster (z0, dz): z0 + dz rand; two_clusters: the front
    half at 5 +- 1e-3, the rest at 50 +- 1e-3; dyadic: the (20, 1e-2) cluster on multiples of 2^-12 (z + 64 is exact too)."""
    r = torch.rand(n, generator=torch.Generator().manual_seed(seed))
    if kind == "spread":
        z = 0.5 + 20.0 * r
    elif kind in CLUSTERS:
        z = CLUSTERS[kind][0] + CLUSTERS[kind][1] * r
    elif kind == "two_clusters":
        z = torch.where(torch.arange(n) < n // 2, 5.0, 50.0) + 1e-3 * (2.0 * r - 1.0)
    elif kind == "dyadic":
        z = 20.0 + torch.round(r * 1e-2 * 4096.0) / 4096.0
    else:
        raise ValueError(kind)
    return torch.sort(z.float()).values


def stack_opacity(n):
    """opacities under which a stack of n layers ends semi-occluded (the median T_N between 1e-6 and 0.3), not dead"""
    return (0.02, 0.3) if n <= 65 else (0.01, 0.1) if n <= 257 else (0.005, 0.05)


def underflow_scene():
    """opacity 0.4 - 0.8: T falls below FLT_MIN, walk_back's slow branch, T_N == 0 in float32 at about half the pixels.  200 layers:
    at 300 (the `underflow_300` of tests/test_render_depth_gpu.py) the float32 formulation itself misses 2e-5 of some rows' scale"""
    return stack_scene(200, 0.4, 0.8, 43)


def tiny_tn_scene():
    """T_N non-zero but between 1e-36 and 1e-30 at some pixels: R_N is in force at the edge of float32"""
    return stack_scene(230, 0.25, 0.45, 47)


def frame17_scene():
    """a 17 x 17 frame of full-cover boxes: four tiles, three of them partly outside the frame, one a single pixel wide"""
    return stack_scene(40, 0.02, 0.3, 51, w=16, h=16)


def subpixel_scene():
    """45 x 38 with float means off the pixel grid and every seventh opacity 1; every Gaussian is widened until it keeps 1e-6 of
    its peak at the corners of its box, as a box cut at a few sigma does: where only tails of 1e-30 meet, `dist` is 1e-62 and
    no float32 arithmetic holds such a pixel to a relative bound"""
    sc = make_scene(90, 45, 38, 9, 71, opacity_one_every=7)
    sc["mean"] = sc["mean"].float() + (torch.rand(90, 2, generator=torch.Generator().manual_seed(72)) - 0.5)
    q = torch.zeros(90)
    for cx in (sc["start"][:, 0], sc["end"][:, 0]):
        for cy in (sc["start"][:, 1], sc["end"][:, 1]):  # a convex form is largest at a corner
            d = torch.stack([cx - sc["mean"][:, 0], cy - sc["mean"][:, 1]], 1)
            q = torch.maximum(q, torch.einsum("ni,nij,nj->n", d, sc["vinv"], d))
    sc["vinv"] = (sc["vinv"] * (2.0 * 13.8 / q).clamp(max=1.0)[:, None, None]).contiguous()
    return sc


BUILDERS = {f"stack_{n}": functools.partial(lambda n: stack_scene(n, *stack_opacity(n), 900 + n), n) for n in STACK_SIZES}
BUILDERS.update({
    "deep_300": lambda: golden_stack("deep_300"), "deep_700": lambda: golden_stack("deep_700"),
    "underflow_200": underflow_scene, "tiny_tn": tiny_tn_scene,
    "stack_4096": lambda: stack_scene(4096, 0.002, 0.02, 41),
    "opaque_layer": opaque_layer_scene, "frame17": frame17_scene, "subpixel": subpixel_scene,
})
# every scene of <= 700 layers with every depth set; the 4096-layer stack spread only
STACKS = [k for k in BUILDERS if k != "stack_4096"]
CASES = [(s, d) for s in STACKS for d in DEPTH_SETS] + [("stack_4096", "spread")]


@functools.lru_cache(maxsize=None)
def scene(name):
    return BUILDERS[name]()


def upstream(sc, seed=2):
    gI, gD, gA = random_grads(sc, seed)
    return gI, gD, gA, torch.randn(sc["height"] + 1, sc["width"] + 1, generator=torch.Generator().manual_seed(seed + 100))


@functools.lru_cache(maxsize=4)
def closed_forms(name, kind):
    """(float64 closed form, float32 formulation) of one case, computed once and left unchanged"""
    sc = scene(name)
    z = depths(kind, sc["start"].shape[0])
    ups = upstream(sc)
    return blend_rows(sc, z, BG, *ups), blend_rows(sc, z, BG, *ups, dtype=torch.float32)


def row_norm(t):
    return t.reshape(t.shape[0], -1).abs().amax(1) if t.dim() > 1 else t.abs()


def check_rows(tag, got, want, scale, f32, failures, rows=True):
    """The rule on every row (`rows`: dim 0 indexes rows; else the tensor is one row, or — a map — every element its own);
    prints the ROWS line, appends to `failures`."""
    if not rows:
        got, want, scale, f32 = (t.reshape(1, -1) for t in (got, want, scale, f32))
    got = got.double().reshape(want.shape)
    assert bool(torch.isfinite(got).all()), tag
    err, ferr, s = row_norm(got - want), row_norm(f32 - want), row_norm(scale)
    bound = RTOL * s + MARGIN * ferr
    dead = (s == 0) & (row_norm(want) == 0)
    outside = (err > bound) | (dead & (row_norm(got) != 0))
    live = s > 0
    rel, frel = (err[live] / s[live]), (ferr[live] / s[live])
    med = lambda t: float(t.median()) if t.numel() else 0.0  # noqa: E731
    mx = lambda t: float(t.max()) if t.numel() else 0.0  # noqa: E731
    print(f"ROWS {tag}: live {int(live.sum())}/{s.numel()} kernel err/scale median {med(rel):.2e} max {mx(rel):.2e} | formulation median "
          f"{med(frel):.2e} max {mx(frel):.2e} | outside {int(outside.sum())}")
    if bool(outside.any()):
        i = int(outside.nonzero()[0])
        failures.append(f"{tag}: {int(outside.sum())} rows outside the rule; first {i}: err {float(err[i]):.3e} scale {float(s[i]):.3e} "
                        f"formulation err {float(ferr[i]):.3e}; max err/scale {mx(rel):.2e}")


def check_maps(tag, maps, want, f32, failures):
    """image and alpha absolute at TOL; depth and dist per pixel under the rule"""
    torch.testing.assert_close(maps["image"].double(), want["image"], atol=TOL, rtol=0)
    torch.testing.assert_close(maps["alpha"].double(), want["alpha"], atol=TOL, rtol=0)
    for k in ("depth", "dist"):
        check_rows(f"{tag} map {k}", maps[k].reshape(-1), want[k].reshape(-1), want[k + "_scale"].reshape(-1), f32[k].reshape(-1), failures)


def hip_render(sc, z, device, ups):
    """cuda_kernel.render(background=, distortion=True) -> (maps, render rows: the gradient of <I,gI> + <D,gD> + <A,gA>,
    distortion rows: the gradient of <dist, G>), two backward passes over one forward"""
    import cuda_kernel as ck

    gI, gD, gA, G = (t.to(device) for t in ups)
    names = ["vinv", "opacity", "l_d", "z", "bg"]
    leaves = [t.to(device).clone().requires_grad_(True) for t in (sc["vinv"], sc["opacity"], sc["l_d"], z, BG)]
    mean = sc["mean"].to(device)
    if mean.is_floating_point():
        mean = mean.clone().requires_grad_(True)
        names.append("mean")
        leaves.append(mean)
    img, dep, alp, dist = ck.render(sc["start"].to(device), sc["end"].to(device), mean, *leaves[:4], sc["width"], sc["height"],
                                    background=leaves[4], distortion=True)
    r = torch.autograd.grad((img * gI).sum() + (dep * gD).sum() + (alp * gA).sum(), leaves, retain_graph=True)
    d = torch.autograd.grad((dist * G).sum(), leaves, allow_unused=True)
    maps = {k: t.detach().cpu() for k, t in (("image", img), ("depth", dep), ("alpha", alp), ("dist", dist))}
    return maps, {k: t.cpu() for k, t in zip(names, r)}, {k: t.cpu() for k, t in zip(names, d) if t is not None}


def hip_distort(sc, z, device, G):
    """raster.blend_distort_* on the bins and checkpoints of blend_forward_depth -> (dist, {mean, vinv, opacity, z}, b_n)"""
    from simplegaussiansplat_tk71_amd import raster

    d = {k: sc[k].to(device) for k in ("start", "end", "mean", "vinv", "opacity", "l_d")}
    zd = z.to(device)
    bins = raster.bin_tiles(d["start"], d["end"], sc["width"], sc["height"])
    geo = (d["start"], d["end"], d["mean"], d["vinv"], d["opacity"])
    *_, ck = raster.blend_forward_depth(bins, *geo, d["l_d"], zd, with_checkpoints=True)
    dist, a_n, b_n = raster.blend_distort_forward(bins, *geo, zd)
    g_mean, g_vinv, g_op, g_z = raster.blend_distort_backward(bins, *geo, zd, ck, a_n, b_n, G.to(device))
    return dist.cpu(), {"mean": g_mean.cpu(), "vinv": g_vinv.cpu(), "opacity": g_op.cpu(), "z": g_z.cpu()}, b_n.cpu()


@pytest.mark.parametrize("name,kind", CASES, ids=[f"{s}-{d}" for s, d in CASES])
def test_every_row_and_pixel_within_its_own_condition_scale(device, name, kind):
    sc = scene(name)
    z = depths(kind, sc["start"].shape[0])
    (want_r, want_d, want_m), (f32_r, f32_d, f32_m) = closed_forms(name, kind)
    maps, got_r, got_d = hip_render(sc, z, device, upstream(sc))
    tag = f"{name} {kind}"
    failures = []
    check_maps(tag, maps, want_m, f32_m, failures)
    for leaf, g in got_r.items():
        check_rows(f"{tag} render {leaf}", g, *want_r[leaf], f32_r[leaf][0], failures, rows=leaf != "bg")
    assert set(got_d) >= set(DIST_LEAVES) and "l_d" in got_d  # (l_d and bg get the zeros of the three maps' own backward)
    for leaf in [k for k in got_d if k in ("mean", *DIST_LEAVES)]:
        check_rows(f"{tag} distortion {leaf}", got_d[leaf], *want_d[leaf], f32_d[leaf][0], failures)
    assert float(got_d["l_d"].abs().max()) == 0.0 and float(got_d["bg"].abs().max()) == 0.0
    if name == "underflow_200":
        assert float((maps["alpha"] == 1.0).float().mean()) > 0.25  # T_N underflowed to exactly 0 in float32: the slow branch, R_N = 0
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", ["stack_33", "stack_257", "subpixel"])
def test_the_mean_row_of_the_distortion_and_the_forward_state(device, name):
    """raster.blend_distort_* directly: the mean's row for integer means too (the Function drops it), at the cluster that
    cancels most; b_n is sum_j w_j (z_L - z_j), L the pixel's last contributing pair."""
    sc = scene(name)
    kind = "z100_1e-2"
    z = depths(kind, sc["start"].shape[0])
    (_, want_d, want_m), (_, f32_d, f32_m) = closed_forms(name, kind)
    dist, got, b_n = hip_distort(sc, z, device, upstream(sc)[3])
    failures = []
    check_rows(f"{name} {kind} raster map dist", dist.reshape(-1), want_m["dist"].reshape(-1), want_m["dist_scale"].reshape(-1),
               f32_m["dist"].reshape(-1), failures)
    for leaf in ("mean", *DIST_LEAVES):
        check_rows(f"{name} {kind} raster distortion {leaf}", got[leaf], *want_d[leaf], f32_d[leaf][0], failures)
    assert not failures, "\n".join(failures)
    if name != "subpixel":  # one tile, every box over it, nothing dropped: L is the last layer and A_n = alpha
        want_b = float(z[-1].double()) * want_m["alpha"] - want_m["depth"]
        assert float((b_n.double() - want_b).abs().max()) <= 1e-5 * 1e-2  # the spread, not the depth, sets its size
        assert float(b_n.abs().max()) <= 1e-2


def test_distortion_is_the_same_64_units_further_away(device):
    """Metamorphic: the (20, 1e-2) cluster on a dyadic grid, so that z and z + 64 are both exact in float32.  dist and its four
    gradients do not depend on the offset: both runs satisfy the rule against the SAME float64 rows."""
    name = "stack_257"
    sc = scene(name)
    z = depths("dyadic", sc["start"].shape[0])
    assert bool(((z.double() * 4096) % 1 == 0).all()) and bool((((z + 64.0).double() - z.double()) == 64.0).all())
    ups = upstream(sc)
    _, want_d, want_m = blend_rows(sc, z, BG, *ups)
    _, f32_d, f32_m = blend_rows(sc, z, BG, *ups, dtype=torch.float32)
    failures = []
    for shift in (0.0, 64.0):
        dist, got, _ = hip_distort(sc, z + shift, device, ups[3])
        check_rows(f"{name} dyadic +{shift:g} map dist", dist.reshape(-1), want_m["dist"].reshape(-1), want_m["dist_scale"].reshape(-1),
                   f32_m["dist"].reshape(-1), failures)
        for leaf in ("mean", *DIST_LEAVES):
            check_rows(f"{name} dyadic +{shift:g} distortion {leaf}", got[leaf], *want_d[leaf], f32_d[leaf][0], failures)
    assert not failures, "\n".join(failures)


def test_model_render_maps_within_the_pixel_rule(device):
    """GS_model_with_param.render(distortion=True, background=): the depth and distortion maps of both cameras, pixel by pixel
    under the rule, against the closed form on the camera lists the model's own projection made (copied from the device)."""
    from simplegaussiansplat_tk71_amd import gs_model as gm

    zf = np.load(os.path.join(GOLD, "forward_golden.npz"))
    name = "fwd_40g_2cam_32x24"
    w = {k: torch.from_numpy(zf[f"{name}/{k}"]).to(device) for k in ("mean", "variance_q", "variance_scale", "opacity", "color", "P", "K", "wh")}
    model = gm.GS_model_with_param(w["mean"].clone(), w["variance_q"].clone(), w["variance_scale"].clone(), w["opacity"].clone())
    with torch.no_grad():
        model.color.copy_(w["color"])
        images, depth, alpha, dist, names, _ = model.render(w["P"], w["K"], w["wh"], background=BG.to(device), distortion=True)
        cams, _, (width, height) = model.camera_inputs(w["P"], w["K"], w["wh"], with_depth=True)
    failures = []
    for c, cam in enumerate(cams):
        sc = {"start": cam["startpoint"].cpu(), "end": cam["endpoint"].cpu(), "mean": cam["mean"].cpu(), "vinv": cam["variance_inverse"].cpu(),
              "opacity": cam["opacity"].cpu(), "l_d": cam["l_d"].cpu(), "width": int(width), "height": int(height)}
        zc = cam["depth"].cpu()
        assert bool((zc[1:] >= zc[:-1]).all())
        ups = upstream(sc)
        want = blend_rows(sc, zc, BG, *ups)[2]
        f32 = blend_rows(sc, zc, BG, *ups, dtype=torch.float32)[2]
        maps = {"image": images[c].permute(1, 2, 0).cpu(), "depth": depth[c, 0].cpu(), "alpha": alpha[c, 0].cpu(), "dist": dist[c, 0].cpu()}
        crop = {k: (v[1:, 1:] if v.dim() >= 2 else v) for k, v in want.items()}  # the model drops the frame's row 0 and column 0
        crop32 = {k: (v[1:, 1:] if v.dim() >= 2 else v) for k, v in f32.items()}
        assert float(crop["dist"].max()) > 0
        check_maps(f"model camera {c}", maps, crop, crop32, failures)
    assert not failures, "\n".join(failures)
