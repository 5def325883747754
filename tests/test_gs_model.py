"""Caller side on CPU: the oracle's PyTorch restatement of the camera projection against the
reference's own forward, the small closed forms, the model's host logic (densify / prune) against the reference, and
the COLMAP binary reader.  The projection and loss KERNELS are checked against these restatements in
test_gs_model_gpu.py."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import gs_forward_torch as gft
from oracle import loss_torch
from simplegaussiansplat_tk71_amd import colmap_io
from simplegaussiansplat_tk71_amd import gs_model as gm

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "forward_golden.npz")
CASES = ("fwd_40g_2cam_32x24", "fwd_600g_3cam_96x64")
TILE_LOGIT = math.log(0.04 / 0.96)  # variance_pixel_tile_max_width = 0.04 (gs_control.py:40)


def golden_world(z, name):
    return {k: torch.from_numpy(z[f"{name}/{k}"]) for k in ("mean", "variance_q", "variance_scale", "opacity", "color", "P", "K", "wh")}


def _sh_condition_scale(w, c):
    """Per Gaussian and channel, the sum of |term| of the degree-2 SH expansion that gives l_d in camera c (fp64, view
    direction from the camera-space mean): the magnitude of the sum with every term taken in absolute value."""
    mean = w["mean"].double()
    P = w["P"][c].double()
    mc = mean @ P[:, :3].T + P[:, 3]
    x, y, z = (-mc / mc.norm(dim=1, keepdim=True)).unbind(1)
    basis = torch.stack([torch.full_like(x, gft._SH_C0), gft._SH_C1 * y, gft._SH_C1 * z, gft._SH_C1 * x,
                         gft._SH_C2[0] * x * y, gft._SH_C2[1] * y * z, gft._SH_C2[2] * (2 * z * z - x * x - y * y),
                         gft._SH_C2[3] * x * z, gft._SH_C2[4] * (x * x - y * y)], 1)      # (N, 9)
    return (basis.abs()[:, :, None] * w["color"].double().abs()).sum(1).numpy()        # (N, 3)


@pytest.mark.parametrize("name", CASES)
def test_camera_inputs_match_reference_forward(name):
    """Arguments the reference's GS_model_with_param.forward hands to the Function (captured by
    tests/golden/make_forward_golden.py): integers bit-exact, floats within 1e-6 relative."""
    z = np.load(GOLDEN)
    w = golden_world(z, name)
    cams, grad_iter, (width, height) = gft.camera_inputs(w["mean"], w["variance_q"], w["variance_scale"], w["opacity"],
                                                        w["color"], w["P"], w["K"], w["wh"], TILE_LOGIT)
    assert int(z[f"{name}/n_rendered"]) == sum(c is not None for c in cams)
    assert np.array_equal(grad_iter.numpy(), z[f"{name}/grad_iter"])
    for c, cam in enumerate(cams):
        ref = lambda k: z[f"{name}/cam{c}/{k}"]  # noqa: E731
        assert (int(width), int(height)) == (int(ref("width")), int(ref("height")))
        for mine, theirs in (("boxsize", "boxsize"), ("startpoint", "startpoint"), ("endpoint", "endpoint"), ("mean", "mean_pixel")):
            got = cam[mine].numpy()
            assert got.dtype == ref(theirs).dtype and np.array_equal(got, ref(theirs)), (c, mine)
        for mine, theirs in (("variance_inverse", "variance_inverse"), ("opacity", "opacity_sigmoid")):
            np.testing.assert_allclose(cam[mine].numpy(), ref(theirs), rtol=1e-6, atol=1e-7)
        # l_d went through the build's own eval_sh on both sides (sh_utility.py is absent from the reference).  It is a sum
        # of SH terms that can cancel, and its fp32 inputs (camera-space means through a CPU matmul) differ in the last bits
        # with the host's vector kernels: 1e-6 of the sum's condition scale, the rule tests/util.py states for sums.
        scale = _sh_condition_scale(w, c)[cam["index"].numpy()]
        err = np.abs(cam["l_d"].numpy().astype(np.float64) - ref("l_d_STAND_IN_SH"))
        assert (err <= 1e-6 * scale + 1e-7).all(), (c, float(err.max()), float((err / scale).max()))
        assert int(ref("batch")[-1]) == cam["boxsize"].numel()  # the reference's single memory chunk


def test_camera_inputs_gradients_reach_every_parameter():
    z = np.load(GOLDEN)
    w = golden_world(z, CASES[0])
    leaves = {k: w[k].clone().requires_grad_(True) for k in ("mean", "variance_q", "variance_scale", "opacity", "color")}
    cams, _, _ = gft.camera_inputs(leaves["mean"], leaves["variance_q"], leaves["variance_scale"], leaves["opacity"],
                                  leaves["color"], w["P"], w["K"], w["wh"], TILE_LOGIT)
    sum((c["variance_inverse"].sum() + c["opacity"].sum() + c["l_d"].sum()) for c in cams).backward()
    for k, v in leaves.items():
        assert v.grad is not None and torch.isfinite(v.grad).all() and v.grad.abs().sum() > 0, k


def test_box_halfsize_equals_eigh_formula():
    """3*sqrt(V^2 |lambda|) of gs_model.py:327-332, including indefinite and isotropic matrices."""
    g = torch.Generator().manual_seed(0)
    a = torch.randn(4000, 2, 2, generator=g, dtype=torch.float64)
    psd = a @ a.transpose(1, 2) + 1e-6 * torch.eye(2, dtype=torch.float64)
    indefinite = a + a.transpose(1, 2)
    iso = torch.eye(2, dtype=torch.float64)[None] * torch.rand(50, 1, 1, generator=g, dtype=torch.float64)
    for m in (psd, indefinite, iso):
        lam, vec = torch.linalg.eigh(m)
        want = 3 * torch.sqrt(vec**2 @ lam.abs()[..., None]).squeeze(-1)
        torch.testing.assert_close(gft.box_halfsize(m), want, rtol=1e-9, atol=1e-12)
    torch.testing.assert_close(gft.box_halfsize(psd.float()), (3 * torch.sqrt(torch.diagonal(psd, dim1=1, dim2=2))).float())


def test_eval_sh_basis_is_orthonormal():
    """The nine real-SH functions integrate to the identity over the sphere (midpoint rule in cos(theta), phi)."""
    nt, nphi = 400, 800
    ct = (torch.arange(nt, dtype=torch.float64) + 0.5) / nt * 2 - 1
    phi = (torch.arange(nphi, dtype=torch.float64) + 0.5) / nphi * 2 * math.pi
    st = torch.sqrt(1 - ct**2)
    d = torch.stack([st[:, None] * torch.cos(phi)[None], st[:, None] * torch.sin(phi)[None], ct[:, None].expand(nt, nphi)], dim=-1)
    basis = []
    for k in range(9):
        sh = torch.zeros(1, 1, 3, 9, dtype=torch.float64)
        sh[..., k] = 1
        basis.append(gft.eval_sh(2, sh, d)[..., 0])
    b = torch.stack(basis).reshape(9, -1)
    gram = b @ b.T * (2.0 / nt) * (2 * math.pi / nphi)
    torch.testing.assert_close(gram, torch.eye(9, dtype=torch.float64), atol=1e-4, rtol=0)  # quadrature error
    # lower degrees are prefixes of the same expansion; too few coefficients or degree 3 are refused
    sh = torch.randn(5, 3, 9, dtype=torch.float64)
    dirs = torch.nn.functional.normalize(torch.randn(5, 3, dtype=torch.float64), dim=-1)
    torch.testing.assert_close(gft.eval_sh(0, sh, dirs), 0.28209479177387814 * sh[..., 0])
    with pytest.raises(ValueError):
        gft.eval_sh(3, sh, dirs)
    with pytest.raises(ValueError):
        gft.eval_sh(2, sh[..., :4], dirs)


def test_small_closed_forms():
    g = torch.Generator().manual_seed(1)
    q = torch.nn.functional.normalize(torch.randn(64, 4, generator=g, dtype=torch.float64), dim=1)
    R = gm.qvec_to_rotmat_batch(q)
    torch.testing.assert_close(R @ R.transpose(1, 2), torch.eye(3, dtype=torch.float64).expand(64, 3, 3), atol=1e-12, rtol=0)
    torch.testing.assert_close(torch.linalg.det(R), torch.ones(64, dtype=torch.float64))
    ident = gm.qvec_to_rotmat_batch(torch.tensor([[0.0, 0.0, 0.0, 1.0]]))  # (x, y, z, w): w last (uitility.py:236)
    torch.testing.assert_close(ident[0], torch.eye(3))
    torch.testing.assert_close(gft.qvec_to_rotmat_batch(q), R)
    A = torch.randn(32, 2, 2, generator=g, dtype=torch.float64) + 3 * torch.eye(2, dtype=torch.float64)
    torch.testing.assert_close(gft.invert_2x2_batch(A, eps=0.0), torch.linalg.inv(A))
    # Jacobian of the pinhole projection, against autograd
    K = torch.tensor([[[50.0, 0, 16], [0, 40.0, 12], [0, 0, 1]]], dtype=torch.float64)
    xyz = (torch.randn(1, 6, 3, generator=g, dtype=torch.float64) + torch.tensor([0, 0, 4.0])).requires_grad_(True)
    proj = lambda p: (p @ K[0].T)[..., :2] / (p @ K[0].T)[..., 2:3]  # noqa: E731
    J = gft.pixel_jacobian_batch(K, xyz.detach())
    for i in range(6):
        torch.testing.assert_close(J[0, i], torch.autograd.functional.jacobian(proj, xyz.detach()[0, i]))
    lr = gm.get_expon_lr_func(1.6e-4, 1.6e-6, lr_delay_mult=0.01, max_steps=30000)
    assert lr(0) == pytest.approx(1.6e-4) and lr(30000) == pytest.approx(1.6e-6) and lr(15000) == pytest.approx(1.6e-5)
    assert lr(-1) == 0.0 and lr(10**9) == pytest.approx(1.6e-6)
    cloud = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 2, 0], [5, 5, 5]])
    d = gm.mean_neighbour_distance(2, cloud)  # self (0) + nearest neighbour, as the reference's kyori2 does
    torch.testing.assert_close(d[:3, 0], torch.tensor([0.5, 0.5, 1.0]))
    assert d.shape == (4, 3)


def test_ssim_and_loss():
    g = torch.Generator().manual_seed(2)
    a = torch.rand(2, 3, 24, 32, generator=g)
    b = (a + 0.2 * torch.randn(a.shape, generator=g)).clamp(0, 1)
    same = loss_torch.ssim(a, a)
    assert same.shape == a.shape
    torch.testing.assert_close(same, torch.ones_like(same), atol=1e-5, rtol=0)
    torch.testing.assert_close(loss_torch.ssim(a, b), loss_torch.ssim(b, a))
    assert loss_torch.ssim(a, b).mean() < 0.9
    assert float(loss_torch.splat_loss(a, a)) == pytest.approx(0.0, abs=1e-6)
    assert float(loss_torch.splat_loss(a, b)) > float(loss_torch.splat_loss(a, (a + b) / 2))
    const = torch.full((1, 3, 16, 16), 0.25)
    torch.testing.assert_close(loss_torch.ssim(const, const * 2).mean(), torch.tensor((2 * 0.25 * 0.5 + 1e-4) / (0.25**2 + 0.5**2 + 1e-4)), atol=1e-5, rtol=0)


def test_colmap_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    cameras = {1: {"model": "OPENCV", "width": 640, "height": 427, "params": rng.random(8) * 500},
               7: {"model": "SIMPLE_RADIAL", "width": 320, "height": 200, "params": np.array([300.0, 160, 100, 0.01])}}
    images = {3: {"qvec": np.array([0.5, 0.5, -0.5, 0.5]), "tvec": np.array([1.0, 2, 3]), "camera_id": 7, "name": "a/b c.JPG"},
              9: {"qvec": np.array([1.0, 0, 0, 0]), "tvec": np.array([0.0, 0, 0]), "camera_id": 1, "name": "z.png"}}
    points = {"id": np.array([5, 11, 12]), "xyz": rng.standard_normal((3, 3)), "rgb": rng.integers(0, 256, (3, 3)).astype(np.uint8),
              "error": rng.random(3)}
    colmap_io.write_model(tmp_path, cameras, images, points)
    cams = colmap_io.read_cameras(tmp_path / "cameras.bin")
    assert list(cams) == [1, 7] and cams[7]["model"] == "SIMPLE_RADIAL" and cams[1]["width"] == 640
    np.testing.assert_array_equal(cams[1]["params"], cameras[1]["params"])
    ims = colmap_io.read_images(tmp_path / "images.bin")
    assert ims[3]["name"] == "a/b c.JPG" and ims[9]["camera_id"] == 1
    pts = colmap_io.read_points3d(tmp_path / "points3D.bin")
    for k in points:
        np.testing.assert_array_equal(pts[k], points[k])
    xyz, P, K, wh, names = colmap_io.load_colmap_tensors(tmp_path)
    assert xyz.shape == (3, 3) and P.shape == (2, 3, 4) and K.shape == (2, 3, 3) and names == ["a/b c.JPG", "z.png"]
    torch.testing.assert_close(K[0], torch.tensor([[300.0, 0, 160], [0, 300.0, 100], [0, 0, 1]]))  # single focal length
    torch.testing.assert_close(K[1, 1, 1], torch.tensor(float(cameras[1]["params"][1])))
    torch.testing.assert_close(P[1], torch.eye(3, 4))
    R = P[0, :, :3].double()
    torch.testing.assert_close(R @ R.T, torch.eye(3, dtype=torch.float64), atol=1e-6, rtol=0)
    torch.testing.assert_close(wh, torch.tensor([[320.0, 200.0], [640.0, 427.0]]))
    (tmp_path / "cameras.bin").write_bytes((tmp_path / "cameras.bin").read_bytes()[:-3])
    with pytest.raises(ValueError):
        colmap_io.read_cameras(tmp_path / "cameras.bin")


def test_colmap_reads_the_reference_scene():
    """The files the reference's checkout does hold, byte for byte in tests/golden/colmap_scene
    (make_colmap_fixture.py): 100 OPENCV cameras 640x427, 10 409 points."""
    sparse = os.path.join(os.path.dirname(__file__), "golden", "colmap_scene", "sparse", "0")
    cams = colmap_io.read_cameras(os.path.join(sparse, "cameras.bin"))
    assert len(cams) == 100 and {c["model"] for c in cams.values()} == {"OPENCV"}
    assert {(c["width"], c["height"]) for c in cams.values()} == {(640, 427)}
    pts = colmap_io.read_points3d(os.path.join(sparse, "points3D.bin"))
    assert pts["xyz"].shape == (10409, 3) and np.isfinite(pts["xyz"]).all() and len(np.unique(pts["id"])) == 10409


def test_camera_extent_uses_camera_centres():
    # two cameras at (+-2, 0, 0) looking at the origin: centres 4 apart, translation columns identical
    R0 = torch.tensor([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])  # forward = -x
    R1 = torch.tensor([[0.0, 0, -1], [0, 1, 0], [1, 0, 0]])  # forward = +x
    P = torch.stack([torch.cat([R0, -(R0 @ torch.tensor([2.0, 0, 0]))[:, None]], 1), torch.cat([R1, -(R1 @ torch.tensor([-2.0, 0, 0]))[:, None]], 1)])
    data = gm.GS_dataset(P, torch.eye(3).expand(2, 3, 3), torch.tensor([[8.0, 8.0]] * 2), ["a", "b"])
    assert len(data) == 2 and data[1][3] == "b"
    assert data.get_camera_extent() == pytest.approx(2.0)
    assert data.get_camera_extent(reference_translation=True) == pytest.approx(0.0, abs=1e-6)


def _densify_model(z):
    t = lambda k: torch.from_numpy(z[f"densify/{k}"]).clone()  # noqa: E731
    m = gm.GS_model_with_param(t("mean"), t("variance_q"), t("variance_scale"), t("opacity"))  # the reference's defaults
    with torch.no_grad():
        m.color.copy_(t("color"))
    m.mean_grads_norm, m.mean_grads_iter = t("mean_grads_norm"), t("mean_grads_iter")
    return m


def _assert_model_equals(z, tag, m):
    for k in ("mean", "variance_q", "variance_scale", "opacity", "color", "mean_grads_norm", "mean_grads_iter"):
        got = getattr(m, k).detach().numpy()
        want = z[f"densify/{tag}/{k}"]
        assert got.shape == want.shape and got.dtype == want.dtype, (tag, k, got.shape, want.shape)
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7, err_msg=f"{tag}/{k}")


def test_densify_prune_reset_match_reference():
    """The reference's densify_and_clone / _split / _prune and reset_opacity (gs_model.py:190-271) run on CPU by
    make_forward_golden.py, same seeds: the same Gaussians are split, cloned and pruned, rows in the same order,
    the split samples drawn identically."""
    z = np.load(GOLDEN)
    extent = float(z["densify/extent"])
    m = _densify_model(z)
    np.testing.assert_allclose(m.param_grads_per_iter_norm().numpy(), z["densify/grads_per_iter_norm"], rtol=1e-6)
    m.densify_and_clone(extent)
    _assert_model_equals(z, "clone", m)
    m = _densify_model(z)
    torch.manual_seed(123)
    m.densify_and_split(extent)
    _assert_model_equals(z, "split_seed123", m)
    m = _densify_model(z)
    torch.manual_seed(321)
    m.densify_and_prune(extent)
    _assert_model_equals(z, "prune_seed321", m)
    assert len(m._optimizer.param_groups) == 5 and m._optimizer.param_groups[0]["params"][0] is m.mean
    m = _densify_model(z)
    m.reset_opacity(0.01)
    _assert_model_equals(z, "reset_opacity", m)
    assert 0 < z["densify/clone/mean"].shape[0] - 160 and z["densify/prune_seed321/mean"].shape[0] != 160


def test_projection_and_loss_have_no_cpu_path():
    """The product's camera_inputs / splat_loss are HIP kernels: CPU tensors raise instead of falling back."""
    z = np.load(GOLDEN)
    w = golden_world(z, CASES[0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        gm.camera_inputs(w["mean"], w["variance_q"], w["variance_scale"], w["opacity"], w["color"], w["P"], w["K"], w["wh"], TILE_LOGIT)
    img = torch.rand(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gm.splat_loss(img, img)
