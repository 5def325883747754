"""Normals (csrc/gcp_normal.hip, simplegaussiansplat_tk71_amd/normals.py) without a GPU: options and defaults, re-exports, the
refusal of CPU tensors, the five entry points bound, exported and declared and validating before any HIP call, the closed-form
gradients the kernels implement against float64 autograd of tests/normal_torch.py, the identity that keeps |c| > 0 — and the
input conditions of tests/test_normals_gpu.py, built here exactly as that file builds them: with these margins no row or pixel
is left out of any comparison there."""
import ctypes
import inspect
import re

import pytest
import torch
import torch.nn.functional as F

from tests import normal_cases as nc
from tests import normal_torch as nt

NAMES = ("gcp_normals_forward", "gcp_normals_backward", "gcp_normal_consistency_forward", "gcp_normal_consistency_backward",
         "gcp_normal_consistency_blocks")
OK, INVALID = 0, 1
NORMAL_CASES = [(n, full) for n in nc.NORMAL_SIZES for full in (False, True)]
MAP_CASES = [(b, h, w) for b in nc.BATCHES for h, w in nc.FRAMES]


# ---- options, exports, refusals ----------------------------------------------------------------------------------------------
def test_options_and_defaults():
    from examples import train_cameras as tc
    from simplegaussiansplat_tk71_amd import gs_model as gm
    from simplegaussiansplat_tk71_amd import normals
    from simplegaussiansplat_tk71_amd.cuda_kernel import render

    assert inspect.signature(gm.GS_model_with_param.render).parameters["normals"].default is False
    assert inspect.signature(render).parameters["normal"].default is None
    a = tc.build_parser().parse_args([])
    assert a.normal_reg == 0.0 and a.normal_from == 7000
    a = tc.build_parser().parse_args(["--normal-reg", "0.05", "--normal-from", "2"])
    assert a.normal_reg == 0.05 and a.normal_from == 2
    sig = inspect.signature(tc.train).parameters
    assert sig["normal_reg"].default == 0.0 and sig["normal_from"].default == 7000
    for fn in (normals.normal_consistency, normals.normal_consistency_map, normals.depth_normals):
        assert inspect.signature(fn).parameters["alpha_min"].default == 1e-3 == nc.ALPHA_MIN
    assert "not tuned" in normals.normal_consistency.__doc__


def test_reexports_and_cpu_tensors_are_refused():
    import cuda_kernel as ck
    from simplegaussiansplat_tk71_amd import gs_model as gm
    from simplegaussiansplat_tk71_amd import normals

    for name in ("gaussian_normals", "normal_consistency", "normal_consistency_map", "depth_normals"):
        assert name in gm.__all__ and getattr(gm, name) is getattr(normals, name)
    assert "RenderNormal" in ck.__all__ and issubclass(ck.RenderNormal, torch.autograd.Function)
    q, scale, mean, P_c, index, _ = nc.normals_case(64, False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        normals.gaussian_normals(q, scale, mean, P_c, index)
    D, A, N, K = nc.consistency_case(1, 5, 7)
    with pytest.raises(RuntimeError, match="no CPU path"):
        normals.normal_consistency(D, A, N, K)
    with pytest.raises(RuntimeError, match="no CPU path"):
        normals.normal_consistency_map(D, A, N, K)
    with pytest.raises(RuntimeError, match="no CPU path"):
        normals.depth_normals(D, A, K)
    with pytest.raises(RuntimeError, match="expects"):
        normals.normal_consistency(D, A, N[:, :2], K)
    z = torch.zeros(3, 2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ck.render(z, z, z, torch.zeros(3, 2, 2), torch.zeros(3, 1), torch.zeros(3, 3), torch.zeros(3), 8, 8, normal=torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="normal: expected"):
        ck.render(z, z, z, torch.zeros(3, 2, 2), torch.zeros(3, 1), torch.zeros(3, 3), torch.zeros(3), 8, 8, normal=torch.zeros(4, 3))


@pytest.fixture(scope="module")
def lib():
    from simplegaussiansplat_tk71_amd import _lib

    return _lib.load()


def test_the_source_and_its_five_entry_points_are_built_bound_and_declared(lib):
    from simplegaussiansplat_tk71_amd import _build, _lib

    assert any(s.endswith("gcp_normal.hip") for s in _build.SRCS)
    with open(_build.INCLUDE + "/grouped_cumprod_hip.h") as f:
        header = f.read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.gcp_abi_version() == _lib.ABI_VERSION
    tiles = lambda h, w: ((w + nc.TILE_W - 1) // nc.TILE_W) * ((h + nc.TILE_H - 1) // nc.TILE_H)  # noqa: E731
    for b, h, w in ((1, 1, 1), (3, 16, 32), (3, 17, 33), (8, 1080, 1920)):
        assert lib.gcp_normal_consistency_blocks(b, h, w) == b * tiles(h, w)
    assert lib.gcp_normal_consistency_blocks(-1, 4, 4) == 0 and lib.gcp_normal_consistency_blocks(1, 0, 4) == 0


def test_entry_points_validate_before_any_hip_call(lib):
    """Host memory stands in for device arrays: every call that gets it must return before anything would read it."""
    buf = ctypes.create_string_buffer(8192)
    base = (ctypes.addressof(buf) + 63) & ~63
    p = [base + 256 * k for k in range(12)]
    fwd = lambda n=4, m=3, a=p: lib.gcp_normals_forward(a[0], a[1], a[2], a[3], a[4], n, m, a[5], a[6], None)  # noqa: E731
    bwd = lambda n=4, m=3, a=p: lib.gcp_normals_backward(a[0], a[1], a[2], a[3], a[4], n, m, a[5], None)  # noqa: E731
    assert fwd(m=0) == OK and fwd(n=-1) == INVALID and fwd(m=-1) == INVALID and fwd(m=2 ** 31) == INVALID
    assert bwd(n=0, m=0) == OK and bwd(n=-1) == INVALID and bwd(m=-1) == INVALID and bwd(n=2 ** 31) == INVALID
    for missing in range(7):
        a = list(p)
        a[missing] = None
        assert fwd(a=a) == INVALID, missing
    a = list(p)
    a[5] = None
    assert bwd(a=a) == INVALID
    cf = lambda b=2, h=5, w=7, am=1e-3, a=p: lib.gcp_normal_consistency_forward(a[0], a[1], a[2], a[3], b, h, w, am, a[4], a[5], a[6], None)  # noqa: E731
    cb = lambda b=2, h=5, w=7, am=1e-3, a=p: lib.gcp_normal_consistency_backward(a[0], a[1], a[2], a[3], b, h, w, am, a[4], a[5], a[6], a[7], None)  # noqa: E731
    for call in (cf, cb):
        assert call(b=0) == OK and call(b=-1) == INVALID and call(h=0) == INVALID and call(w=0) == INVALID
        assert call(am=0.0) == INVALID and call(am=float("nan")) == INVALID and call(h=2 ** 16, w=2 ** 16) == INVALID
    for missing in (0, 1, 2, 3, 6):  # e_map (4) and depth_normal (5) are optional
        a = list(p)
        a[missing] = None
        assert cf(a=a) == INVALID, missing
    for missing in range(8):
        a = list(p)
        a[missing] = None
        assert cb(a=a) == INVALID, missing


# ---- the closed forms of the kernels, in float64 -----------------------------------------------------------------------------
def closed_form_normals_grad(q, scale, mean, P_c, index, G):
    """What k_normals_bwd computes -> g_q (N, 4)."""
    _, k, flipped, _ = nt.gaussian_normals(q, scale, mean, P_c, index)
    g = torch.where(flipped[:, None], -G, G) @ P_c[:, :3]  # P[:, :3]^T g, row by row
    a, b, c = g.unbind(dim=1)
    qi = q[index]
    length = qi.norm(dim=1, keepdim=True).clamp_min(1e-8)
    qn = qi / length
    x, y, z, w = qn.unbind(dim=1)
    per_axis = torch.stack([
        torch.stack([2 * (b * y + c * z), 2 * (b * x - c * w - 2 * a * y), 2 * (b * w + c * x - 2 * a * z), 2 * (b * z - c * y)], dim=1),
        torch.stack([2 * (a * y + c * w - 2 * b * x), 2 * (a * x + c * z), 2 * (c * y - a * w - 2 * b * z), 2 * (c * x - a * z)], dim=1),
        torch.stack([2 * (a * z - b * w - 2 * c * x), 2 * (a * w + b * z - 2 * c * y), 2 * (a * x + b * y), 2 * (a * y - b * x)], dim=1)])
    gq = per_axis[k, torch.arange(k.shape[0])]
    out = torch.zeros_like(q)
    out[index] = (gq - qn * (gq * qn).sum(dim=1, keepdim=True)) / length
    return out


def closed_form_consistency_grads(D, A, N, K, alpha_min, upstream=1.0):
    """What k_nc_bwd computes, as a gather -> (g_D, g_A, g_N)."""
    n, defined, c, pt = nt.depth_normals(D, A, K, alpha_min)
    s = upstream / D.numel()
    pad = lambda t: F.pad(t, (1, 1, 1, 1))  # noqa: E731
    ptp = pad(pt)
    u = ptp[:, :, 2:, 1:-1] - ptp[:, :, :-2, 1:-1]
    v = ptp[:, :, 1:-1, 2:] - ptp[:, :, 1:-1, :-2]
    length = torch.where(defined, c.norm(dim=1, keepdim=True), torch.ones_like(D))
    h = -s * A * N
    gc = torch.where(defined, (h - n * (h * n).sum(dim=1, keepdim=True)) / length, torch.zeros_like(h))
    gu, gv = pad(torch.linalg.cross(v, gc, dim=1)), pad(torch.linalg.cross(gc, u, dim=1))
    g_pt = (gu[:, :, :-2, 1:-1] - gu[:, :, 2:, 1:-1]) + (gv[:, :, 1:-1, :-2] - gv[:, :, 1:-1, 2:])
    g_z = (g_pt * nt.rays(K, D.shape[2], D.shape[3])).sum(dim=1, keepdim=True)
    valid = (A >= alpha_min) & (D > 0)
    safe = torch.where(valid, A, torch.ones_like(A))
    zero = torch.zeros_like(D)
    return (torch.where(valid, g_z / safe, zero), torch.where(valid, -(g_z * (D / safe)) / safe, zero),
            torch.where(defined, -s * A * n, torch.zeros_like(N)))


@pytest.mark.parametrize("n,full", NORMAL_CASES)
def test_normals_closed_form_gradient_equals_autograd(n, full):
    q, scale, mean, P_c, index, G = (t.double() if t.is_floating_point() else t for t in nc.normals_case(n, full))
    leaf = q.clone().requires_grad_(True)
    normal = nt.gaussian_normals(leaf, scale, mean, P_c, index)[0]
    assert normal.shape == (index.shape[0], 3)
    (normal * G).sum().backward()
    want = leaf.grad if leaf.grad is not None else torch.zeros_like(q)
    got = closed_form_normals_grad(q, scale, mean, P_c, index, G)
    assert float((got - want).abs().max()) <= 1e-10 * max(1.0, float(want.abs().max()))
    absent = torch.ones(n, dtype=torch.bool)
    absent[index] = False
    assert bool(absent.any()) != full
    if not full:
        assert float(got[absent].abs().max()) == 0.0
    if index.numel():
        assert float((normal.detach().norm(dim=1) - 1).abs().max()) <= 1e-6  # P[:, :3] is a rotation, rounded to float32


@pytest.mark.parametrize("b,h,w", MAP_CASES)
def test_consistency_closed_form_gradients_equal_autograd_and_the_identity_holds(b, h, w):
    D, A, N, K = (t.double() for t in nc.consistency_case(b, h, w))
    leaves = [t.clone().requires_grad_(True) for t in (D, A, N)]
    loss, e, defined, n = nt.normal_consistency(*leaves, K, nc.ALPHA_MIN)
    (3.0 * loss).backward()
    got = closed_form_consistency_grads(D, A, N, K, nc.ALPHA_MIN, upstream=3.0)
    for what, g, leaf in zip("DAN", got, leaves):
        scale = max(1.0, float(leaf.grad.abs().max()))
        assert float((g - leaf.grad).abs().max()) <= 1e-10 * scale, what
    count = int(defined.sum())
    if (h, w) == (3, 3):
        assert count == b and bool(defined[:, 0, 1, 1].all())
    elif (h, w) == (2, 9):
        assert count == 0 and bool((e == 1).all()) and all(float(leaf.grad.abs().max()) == 0.0 for leaf in leaves)
    else:
        assert count > 0
    # c . r = -(z(x+1,y) + z(x-1,y)) (z(x,y+1) + z(x,y-1)) / (fx fy): |c| > 0 wherever the stencil is defined
    _, _, c, pt = nt.depth_normals(D, A, K, nc.ALPHA_MIN)
    z = F.pad(pt[:, 2:3], (1, 1, 1, 1))
    want = -(z[:, :, 1:-1, 2:] + z[:, :, 1:-1, :-2]) * (z[:, :, 2:, 1:-1] + z[:, :, :-2, 1:-1]) / (K[:, 0, 0] * K[:, 1, 1])[:, None, None, None]
    dot = (c * nt.rays(K, h, w)).sum(dim=1, keepdim=True)
    assert float(torch.where(defined, dot - want, torch.zeros_like(dot)).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert bool((dot[defined] < 0).all())
    # a fronto-parallel surface faces the camera
    flat = nt.depth_normals(torch.full((1, 1, 4, 5), 1.5, dtype=torch.float64), torch.full((1, 1, 4, 5), 0.5, dtype=torch.float64), K[:1])[0]
    assert torch.allclose(flat[0, :, 1, 2], torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64), atol=1e-12)


# ---- the input conditions of the GPU tests -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,full", NORMAL_CASES)
def test_gpu_inputs_normals_keep_their_margins(n, full):
    q, scale, mean, P_c, index, G = nc.normals_case(n, full)
    assert index.shape[0] == (n if full else (2 * n) // 3) and index.unique().numel() == index.numel() and G.shape == (index.shape[0], 3)
    two = torch.sort(scale.double(), dim=1).values
    assert float((two[:, 1] - two[:, 0]).min()) >= 0.1
    dots = nt.gaussian_normals(q.double(), scale.double(), mean.double(), P_c.double(), index)[3]
    assert index.numel() == 0 or float(dots.abs().min()) >= 0.05
    R = P_c[:, :3].double()
    assert float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-6
    assert float((q.norm(dim=1) - 1).abs().max()) > 0.1  # not normalised


@pytest.mark.parametrize("b,h,w", MAP_CASES)
def test_gpu_inputs_maps_keep_their_margins(b, h, w):
    D, A, N, K = nc.consistency_case(b, h, w)
    assert D.shape == A.shape == (b, 1, h, w) and N.shape == (b, 3, h, w) and K.shape == (b, 3, 3)
    assert not bool(((A > 0.9 * nc.ALPHA_MIN) & (A < 1.1 * nc.ALPHA_MIN)).any())
    assert bool((D[A > 0] > 0).all()) and bool((D[A == 0] == 0).all())
    assert bool(((A == 0) | ((A >= 0.3) & (A <= 1.0))).all())
    holes = A == 0
    assert bool(holes.any())
    if h > nc.TILE_H and w > nc.TILE_W:
        assert bool(holes[:, 0, nc.TILE_H - 1, nc.TILE_W - 1].all()) and bool(holes[:, 0, nc.TILE_H, nc.TILE_W].all())
    if (h, w) != (3, 3):
        assert bool(holes[:, 0, h // 2, 1].all())  # next to the frame's edge
        assert 0.02 < float(holes.float().mean()) < 0.35
    assert float((N.norm(dim=1, keepdim=True) - A).max()) <= 1e-6  # |N| <= A
    assert b == 1 or len({tuple(K[i].flatten().tolist()) for i in range(b)}) == b  # a K of its own per image


@pytest.mark.parametrize("variant", ["plain", "filter_3d", "distortion"])
def test_gpu_inputs_model_scene_keeps_its_margins(variant):
    sc = nc.model_scene()
    assert sc["mean"].shape[0] <= 100 and int(sc["wh"].max()) <= 33
    two = torch.sort(sc["variance_scale"].double(), dim=1).values
    assert float((two[:, 1] - two[:, 0]).min()) >= 0.1
    ref = nc.model_reference(sc, phi=nc.model_phi(sc) if variant == "filter_3d" else None, distortion=variant == "distortion")
    for dot in ref["dots"]:
        assert float(dot.abs().min()) >= 0.05
    A, D = ref["alpha"], ref["depth"]
    assert not bool(((A > 0.9 * nc.ALPHA_MIN) & (A < 1.1 * nc.ALPHA_MIN)).any())
    assert bool((D[A > 0] > 0).all())
    defined = nt.depth_normals(D, A, sc["K"].double(), nc.ALPHA_MIN)[1]
    assert float(defined.double().mean()) > 0.5  # the regulariser sees most of the frame
    for k, g in ref["grads"].items():
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
