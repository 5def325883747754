"""The depth distortion map on the GPU (csrc/gcp_distort.hip: k_distort_fwd / k_distort_bwd / k_distort_reduce) through
raster.blend_distort_*, cuda_kernel.render(distortion=True), GS_model_with_param.render(distortion=True) and the training
example, against the dense float64 oracle of tests/distortion_torch.py.  Depths are sorted ascending, as the camera depth of
a depth-ordered list is.  Tolerances are those of the depth map (tests/test_render_depth_gpu.py): TOL * z_max on the map,
2e-4 of its own largest magnitude on every gradient.
Per-Gaussian accuracy, each row against its own condition scale and at clustered depths: tests/test_blend_rows_gpu.py."""
import math
import os

import numpy as np
import pytest
import torch

from tests.distortion_torch import dense_render_distortion
from tests.test_render_depth_gpu import SCENES, dense_render_depth, depths_for, opaque_layer_scene, random_grads
from tests.util import TOL, make_scene

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def subpixel_scene():
    """float means off the pixel grid: the mean is a leaf and gets its gradient"""
    sc = make_scene(90, 45, 38, 9, 71)
    sc["mean"] = sc["mean"].float() + (torch.rand(90, 2, generator=torch.Generator().manual_seed(72)) - 0.5)
    return sc


def all_scenes():
    out = list(SCENES)
    for side in (15, 16, 17, 33):  # frames of `side` pixels: the last tile is full, one short, one pixel wide
        out.append((f"frame{side}", make_scene(60, side - 1, side - 1, 6, 600 + side)))
    out.append(("subpixel", subpixel_scene()))
    return out


ALL = all_scenes()
_oracle_cache = {}


def sorted_depths(sc, seed=1):
    return torch.sort(depths_for(sc, seed)).values


def grad_map(sc, seed=2):
    return torch.randn(sc["height"] + 1, sc["width"] + 1, generator=torch.Generator().manual_seed(seed))


def oracle(name, sc):
    """fp64 (dist, a_n, {vinv, opacity, z[, mean]: gradient of <dist, G>}, the same of <depth map, G> where dist is identically
    0), computed once per scene."""
    if name in _oracle_cache:
        return _oracle_cache[name]
    z, G = sorted_depths(sc), grad_map(sc).double()
    with_mean = sc["mean"].is_floating_point()

    def leaves():
        ls = {"vinv": sc["vinv"], "opacity": sc["opacity"], "z": z}
        if with_mean:
            ls["mean"] = sc["mean"]
        return {k: v.detach().double().clone().requires_grad_(True) for k, v in ls.items()}

    lv = leaves()
    _, _, _, dist, a_n = dense_render_distortion(sc["start"], sc["end"], lv.get("mean", sc["mean"]), lv["vinv"], lv["opacity"],
                                                 sc["l_d"].double(), lv["z"], sc["width"], sc["height"])
    (dist * G).sum().backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in lv.items()}
    depth_grads = None
    if float(dist.detach().abs().max()) == 0.0:
        lv2 = leaves()
        _, dep, _ = dense_render_depth(sc["start"], sc["end"], lv2.get("mean", sc["mean"]), lv2["vinv"], lv2["opacity"], sc["l_d"].double(),
                                       lv2["z"], sc["width"], sc["height"])
        (dep * G).sum().backward()
        depth_grads = {k: v.grad for k, v in lv2.items()}
    _oracle_cache[name] = (dist.detach(), a_n.detach(), grads, depth_grads)
    return _oracle_cache[name]


def hip_raster(sc, device, z=None, G=None):
    """-> (dist, a_n, b_n, {vinv, opacity, z, mean: gradient of <dist, G>}) from raster.blend_distort_* on the bins and
    checkpoints of blend_forward_depth"""
    from simplegaussiansplat_tk71_amd import raster

    z = sorted_depths(sc) if z is None else z
    G = grad_map(sc) if G is None else G
    d = {k: sc[k].to(device) for k in ("start", "end", "mean", "vinv", "opacity", "l_d")}
    zd = z.to(device)
    bins = raster.bin_tiles(d["start"], d["end"], sc["width"], sc["height"])
    *_, ck = raster.blend_forward_depth(bins, d["start"], d["end"], d["mean"], d["vinv"], d["opacity"], d["l_d"], zd, with_checkpoints=True)
    dist, a_n, b_n = raster.blend_distort_forward(bins, d["start"], d["end"], d["mean"], d["vinv"], d["opacity"], zd)
    g_mean, g_vinv, g_op, g_z = raster.blend_distort_backward(bins, d["start"], d["end"], d["mean"], d["vinv"], d["opacity"], zd, ck, a_n, b_n,
                                                              G.to(device))
    return dist.cpu(), a_n.cpu(), b_n.cpu(), {"vinv": g_vinv.cpu(), "opacity": g_op.cpu(), "z": g_z.cpu(), "mean": g_mean.cpu()}


@pytest.mark.parametrize("name,sc", ALL, ids=[n for n, _ in ALL])
def test_forward_and_backward_vs_dense_oracle(device, name, sc):
    dist64, a64, want, depth_want = oracle(name, sc)
    dist, a_n, b_n, got = hip_raster(sc, device)
    z_max = float(sorted_depths(sc).max())
    err = float((dist.double() - dist64).abs().max())
    print(name, "map err", err, "bound", TOL * z_max, "scale", float(dist64.abs().max()))
    torch.testing.assert_close(dist.double(), dist64, atol=TOL * z_max, rtol=0)
    torch.testing.assert_close(a_n.double(), a64, atol=TOL, rtol=0)
    if depth_want is not None:
        # no pixel with two kept layers: the map is exactly 0 and the gradients are what is left of terms that cancel, whose
        # condition scale is the gradient of the depth map
        assert float(dist.abs().max()) == 0.0, name
        for what, w in depth_want.items():
            scale = float(w.abs().max())
            err = float(got[what].double().abs().max())
            print(name, what, "residue", err, "depth-gradient scale", scale)
            assert scale > 0 and err <= 1e-5 * scale, (name, what, err, scale)
        return
    assert float(dist64.abs().max()) > 0, name
    for what, w in want.items():
        scale = float(w.abs().max())
        assert scale > 0, (name, what)
        err = float((got[what].double().reshape(w.shape) - w).abs().max())
        print(name, what, "err", err, "scale", scale, "ratio", err / scale)
        assert err <= 2e-4 * scale, (name, what, err, scale)


def test_random3_is_the_scene_without_a_pair():
    name, sc = ALL[3]
    assert name == "random3" and oracle(name, sc)[3] is not None


def test_layers_behind_an_exactly_opaque_full_frame_layer_get_zero_and_change_nothing_in_front(device):
    sc = opaque_layer_scene()
    n_front, n = 20, sc["start"].shape[0]
    sc["end"][n_front] = torch.tensor([sc["width"], sc["height"]])  # the opaque layer over the whole image
    z, G = sorted_depths(sc, 8), grad_map(sc, 9)
    dist, a_n, b_n, got = hip_raster(sc, device, z, G)
    assert float(dist.abs().max()) > 0 and float(a_n.max()) < 1.0
    for what, g in got.items():
        assert float(g[n_front:].abs().max()) == 0.0, what  # the opaque layer (dropped) and everything behind it
    assert all(float(got[k][:n_front].abs().max()) > 0 for k in ("vinv", "opacity", "z"))
    front = {k: (v[: n_front + 1] if torch.is_tensor(v) and v.shape[0] == n else v) for k, v in sc.items()}
    dist2, a2, b2, got2 = hip_raster(front, device, z[: n_front + 1], G)
    assert torch.equal(dist, dist2) and torch.equal(a_n, a2) and torch.equal(b_n, b2)
    for k in got:
        assert torch.equal(got[k][: n_front + 1], got2[k]), k


def _render(sc, z, bg, device, distortion, absgrad=None):
    import cuda_kernel as ck

    leaves = [t.to(device).clone().requires_grad_(True) for t in (sc["vinv"], sc["opacity"], sc["l_d"], z, bg)]
    out = ck.render(sc["start"].to(device), sc["end"].to(device), sc["mean"].to(device), *leaves[:4], sc["width"], sc["height"],
                    background=leaves[4], absgrad=absgrad, distortion=distortion)
    return leaves, out


def test_render_with_distortion_keeps_the_three_maps_and_matches_the_oracle_on_all_four(device):
    import cuda_kernel as ck

    name, sc = SCENES[1]
    z, bg = sorted_depths(sc, 4), torch.tensor([0.9, 0.35, 0.6])
    gI, gD, gA = random_grads(sc, 5)
    gG = grad_map(sc, 6)
    l3, (img3, dep3, alp3) = _render(sc, z, bg, device, False)
    ((img3 * gI.to(device)).sum() + (dep3 * gD.to(device)).sum() + (alp3 * gA.to(device)).sum()).backward()
    l4, (img, dep, alp, dist) = _render(sc, z, bg, device, True)
    assert torch.equal(img, img3) and torch.equal(dep, dep3) and torch.equal(alp, alp3)
    assert dist.shape == dep.shape
    # a loss that ignores dist: the gradients of the three-map call, bit for bit
    ((img * gI.to(device)).sum() + (dep * gD.to(device)).sum() + (alp * gA.to(device)).sum()).backward()
    for a, b in zip(l3, l4):
        assert torch.equal(a.grad, b.grad)
    # a loss on all four maps against the oracle
    l4, (img, dep, alp, dist) = _render(sc, z, bg, device, True)
    ((img * gI.to(device)).sum() + (dep * gD.to(device)).sum() + (alp * gA.to(device)).sum() + (dist * gG.to(device)).sum()).backward()
    o = [t.detach().double().clone().requires_grad_(True) for t in (sc["vinv"], sc["opacity"], sc["l_d"], z, bg)]
    i64, d64, a64, g64, _ = dense_render_distortion(sc["start"], sc["end"], sc["mean"], *o[:4], sc["width"], sc["height"], o[4])
    ((i64 * gI.double()).sum() + (d64 * gD.double()).sum() + (a64 * gA.double()).sum() + (g64 * gG.double()).sum()).backward()
    torch.testing.assert_close(dist.detach().cpu().double(), g64.detach(), atol=TOL * float(z.max()), rtol=0)
    assert float(g64.detach().abs().max()) > 0
    for what, leaf, w in zip(("vinv", "opacity", "l_d", "z", "bg"), l4, o):
        scale = float(w.grad.abs().max())
        err = float((leaf.grad.cpu().double() - w.grad).abs().max())
        assert scale > 0 and err <= 2e-4 * scale, (what, err, scale)
    # with an absgrad buffer: the buffer of the three-map call, bit for bit (the regulariser is not part of the statistic)
    buf3, buf4 = ck.absgrad_buffer(sc["start"].to(device)), ck.absgrad_buffer(sc["start"].to(device))
    _, (img3, dep3, alp3) = _render(sc, z, bg, device, False, buf3)
    ((img3 * gI.to(device)).sum() + (dep3 * gD.to(device)).sum() + (alp3 * gA.to(device)).sum()).backward()
    _, (img, dep, alp, dist) = _render(sc, z, bg, device, True, buf4)
    ((img * gI.to(device)).sum() + (dep * gD.to(device)).sum() + (alp * gA.to(device)).sum() + (dist * gG.to(device)).sum()).backward()
    assert float(buf3.abs().max()) > 0 and torch.equal(buf3, buf4)


def test_eager_runs_are_bit_identical_and_a_captured_step_replays_them(device):
    import cuda_kernel as ck

    sc = make_scene(400, 100, 70, 9, 3)
    st = {k: sc[k].to(device) for k in ("start", "end", "mean")}
    params = [t.to(device).clone().requires_grad_(True) for t in (sc["vinv"], sc["opacity"], sc["l_d"], sorted_depths(sc, 6))]
    gI, gD, gA = (t.to(device) for t in random_grads(sc, 7))
    gG = grad_map(sc, 8).to(device)

    def body(v, o, l, z):
        img, dep, alp, dist = ck.render(st["start"], st["end"], st["mean"], v, o, l, z, sc["width"], sc["height"], distortion=True)
        return (img * gI).sum() + (dep * gD).sum() + (alp * gA).sum() + (dist * gG).sum(), img, dep, alp, dist

    def eager():
        leaves = [p.detach().clone().requires_grad_(True) for p in params]
        loss, *maps = body(*leaves)
        return tuple(m.detach() for m in maps), torch.autograd.grad(loss, leaves)

    first, second = eager(), eager()
    assert float(first[0][3].abs().max()) > 0
    for a, b in zip(first[0] + first[1], second[0] + second[1]):
        assert torch.equal(a, b)  # no atomics: the same bits on every run
    n = sc["start"].shape[0]
    step = ck.GraphedStep(body, params, capacity=4 * n + 1024)
    assert not ck.capacity_exceeded()
    for factor in (0.9, 1.05):
        with torch.no_grad():
            params[1].mul_(factor).clamp_(max=1.0)
            params[3].add_(0.25)
        (_, *maps), grads = step.replay()
        torch.cuda.synchronize()
        assert not ck.capacity_exceeded()
        e_maps, e_grads = eager()
        for a, b in zip(tuple(maps) + tuple(grads), e_maps + e_grads):
            assert torch.equal(a, b)
    with ck.tile_capacity(50):  # a bound that is too small is reported as for the other Functions
        eager()
    assert ck.capacity_exceeded()
    assert not ck.capacity_exceeded()


def test_model_render_gradients_of_image_plus_distortion_match_the_dense_oracle(device):
    from oracle import gs_forward_torch as gft
    from simplegaussiansplat_tk71_amd import gs_model as gm

    zf = np.load(os.path.join(GOLD, "forward_golden.npz"))
    name = "fwd_40g_2cam_32x24"
    w = {k: torch.from_numpy(zf[f"{name}/{k}"]) for k in ("mean", "variance_q", "variance_scale", "opacity", "color", "P", "K", "wh")}
    n_cam = w["P"].shape[0]
    h, wd = int(w["wh"][0, 1]), int(w["wh"][0, 0])
    g = torch.Generator().manual_seed(4)
    wimg, wdist = torch.randn(n_cam, 3, h, wd, generator=g), torch.randn(n_cam, 1, h, wd, generator=g)
    wgpu = {k: v.to(device) for k, v in w.items()}
    model = gm.GS_model_with_param(wgpu["mean"].clone(), wgpu["variance_q"].clone(), wgpu["variance_scale"].clone(), wgpu["opacity"].clone())
    with torch.no_grad():
        model.color.copy_(wgpu["color"])
    plain = model.render(wgpu["P"], wgpu["K"], wgpu["wh"])
    images, depth, alpha, dist, names, _ = model.render(wgpu["P"], wgpu["K"], wgpu["wh"], distortion=True)
    assert images.shape == (n_cam, 3, h, wd) and depth.shape == alpha.shape == dist.shape == (n_cam, 1, h, wd) and names == list(range(n_cam))
    assert torch.equal(images, plain[0]) and torch.equal(depth, plain[1]) and torch.equal(alpha, plain[2])
    ((images * wimg.to(device)).sum() + (dist * wdist.to(device)).sum()).backward()

    names5 = ("mean", "variance_q", "variance_scale", "opacity", "color")
    leaves = {k: w[k].clone().requires_grad_(True) for k in names5}
    cams, _, _ = gft.camera_inputs(*(leaves[k] for k in names5), w["P"], w["K"], w["wh"], math.log(0.04 / 0.96))
    outs = []
    for c, cam in enumerate(cams):
        zc = (leaves["mean"] @ w["P"][c, 2, :3] + w["P"][c, 2, 3])[cam["index"]]
        outs.append(dense_render_distortion(cam["startpoint"], cam["endpoint"], cam["mean"], cam["variance_inverse"].double(),
                                            cam["opacity"].double(), cam["l_d"].double(), zc.double(), wd, h))
    img64 = torch.stack([o[0] for o in outs])[:, 1:, 1:, :].permute(0, 3, 1, 2)
    dist64 = torch.stack([o[3] for o in outs])[:, None, 1:, 1:]
    dep64 = torch.stack([o[1] for o in outs])[:, None, 1:, 1:]
    assert float(dist64.detach().abs().max()) > 0
    torch.testing.assert_close(images.detach().cpu().double(), img64.detach(), atol=TOL, rtol=0)
    torch.testing.assert_close(dist.detach().cpu().double(), dist64.detach(), atol=TOL * float(dep64.detach().abs().max()), rtol=0)
    ((img64 * wimg.double()).sum() + (dist64 * wdist.double()).sum()).backward()
    for k in names5:
        got, want = getattr(model, k).grad.cpu().double(), leaves[k].grad.double()
        scale = want.abs().max().item()
        assert torch.isfinite(got).all() and scale > 0, k
        assert (got - want).abs().max().item() <= 2e-4 * scale, (k, (got - want).abs().max().item(), scale)


def test_training_with_the_regulariser_runs_and_a_zero_weight_changes_nothing(device):
    from examples.train_cameras import synthetic_scene, train

    start, P, K, wh, targets = synthetic_scene(300, 4, 48, 32, 0, device)
    kw = dict(iterations=6, densify_from_iter=1000, opacity_reset_interval=0, log=lambda *_: None)
    _, base = train(start, P, K, wh, targets, **kw)
    _, zero = train(start, P, K, wh, targets, distortion_reg=0.0, distortion_from=2, **kw)
    _, late = train(start, P, K, wh, targets, distortion_reg=0.5, distortion_from=3, **kw)
    assert zero == base
    assert all(math.isfinite(l) for l in late) and late[:3] == base[:3] and late[3:] != base[3:]
