"""Mip-Splatting's 3-D smoothing filter without a GPU: the option and its errors, the bindings, the float64 formulation the
kernels are held to (mass conservation, closed-form gradients against autograd), and the INPUT CONDITIONS of
tests/test_filter3d_gpu.py — its worlds are built here, on the host, exactly as it builds them."""
import inspect
import re

import pytest
import torch

import filter3d_torch as ft

NAMES = ("gcp_filter3d_rate", "gcp_filter3d_apply", "gcp_filter3d_apply_backward")
RATE_CAMERAS = (1, 3, 65)


def cpu_model(**kw):
    from simplegaussiansplat_tk71_amd import gs_model as gm

    g = torch.Generator().manual_seed(0)
    return gm.GS_model_with_param(torch.randn(8, 3, generator=g), torch.randn(8, 4, generator=g), torch.full((8, 3), -3.0), torch.zeros(8, 1), **kw)


# ---- the option ----------------------------------------------------------------------------------------------------------------
def test_filter_3d_is_validated_as_a_bool_and_off_by_default():
    from simplegaussiansplat_tk71_amd import gs_model as gm

    assert inspect.signature(gm.GS_model_with_param.__init__).parameters["filter_3d"].default is False
    for bad in (1, 0, "yes", None, 0.2):
        with pytest.raises(ValueError, match="filter_3d"):
            cpu_model(filter_3d=bad)
    model = cpu_model()
    assert model.use_filter_3d is False and model.filter_3d is None
    assert "filter_3d" not in dict(model.named_parameters()) and len(list(model.parameters())) == 5
    with pytest.raises(RuntimeError, match="filter_3d=True"):
        model.update_filter_3d(torch.zeros(1, 3, 4), torch.zeros(1, 3, 3), torch.tensor([[8, 8]]))
    assert inspect.signature(gm.GS_model_with_param.save_ply).parameters["bake_filter"].default is True
    assert inspect.signature(gm.GS_model_with_param.update_filter_3d).parameters["variance"].default == 0.2


def test_a_cpu_model_with_the_filter_raises_on_draw_and_on_update():
    from simplegaussiansplat_tk71_amd.synthetic import ring_cameras

    model = cpu_model(filter_3d=True)
    P, K, wh = ring_cameras(2, 16, 12)
    for draw in (lambda: model(P, K, wh, [0, 1]), lambda: model.render(P, K, wh), lambda: model.camera_inputs(P, K, wh),
                 lambda: model.contribution(P, K, wh), lambda: model.update_filter_3d(P, K, wh)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            draw()


def test_the_module_is_re_exported_and_cpu_tensors_raise():
    from simplegaussiansplat_tk71_amd import filter3d
    from simplegaussiansplat_tk71_amd import gs_model as gm

    for name in ("sampling_rate", "filter_from_rate", "apply_filter"):
        assert name in gm.__all__ and getattr(gm, name) is getattr(filter3d, name)
    sig = inspect.signature(filter3d.sampling_rate).parameters
    assert sig["near"].default == 0.2 and sig["margin"].default == 0.15
    assert inspect.signature(filter3d.filter_from_rate).parameters["variance"].default == 0.2
    with pytest.raises(RuntimeError, match="no CPU path"):
        filter3d.apply_filter(torch.zeros(4, 3), torch.zeros(4, 1), torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        filter3d.sampling_rate(torch.zeros(4, 3), torch.zeros(1, 3, 4), torch.zeros(1, 3, 3), torch.tensor([[8, 8]]))


def test_filter_from_rate_on_the_host():
    """Device-side torch ops only, so the same statements run on CPU tensors: unseen rows get the largest seen phi, an
    all-unseen world all zeros, and a seen row's phi is ONE float32 division."""
    from simplegaussiansplat_tk71_amd.filter3d import filter_from_rate

    rate = torch.tensor([0.0, 30.0, 7.5, 0.0, 120.0])
    phi = filter_from_rate(rate)
    want = torch.tensor(0.2 ** 0.5, dtype=torch.float32) / rate[[2, 1, 2, 2, 4]]
    assert phi.dtype == torch.float32 and torch.equal(phi, want) and float(phi[0]) == float(phi.max())
    assert torch.equal(filter_from_rate(torch.zeros(5)), torch.zeros(5))
    assert torch.equal(filter_from_rate(rate, variance=0.05), torch.tensor(0.05 ** 0.5, dtype=torch.float32) / rate[[2, 1, 2, 2, 4]])
    assert filter_from_rate(torch.zeros(0)).shape == (0,)


def test_the_example_has_the_flags_and_they_default_to_off():
    from examples import train_cameras

    params = inspect.signature(train_cameras.train).parameters
    assert params["filter_3d"].default is False and params["filter_every"].default == 100
    ap = train_cameras.build_parser()
    off, on = ap.parse_args([]), ap.parse_args(["--filter-3d", "--filter-every", "25"])
    assert off.filter_3d is False and off.filter_every == 100 and on.filter_3d is True and on.filter_every == 25
    text = [a.help for a in ap._actions if a.dest == "filter_3d"][0]
    assert "--filter-3d --centres subpixel --dilation 0.1 --antialias" in text  # what full Mip-Splatting is


# ---- the bindings ----------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_bound_and_exported():
    from simplegaussiansplat_tk71_amd import _build, _lib

    lib = _lib.load()
    with open(_build.INCLUDE + "/grouped_cumprod_hip.h") as f:
        declared = sorted(set(re.findall(r"\b(gcp_filter3d_\w+)\(", f.read())))
    assert declared == sorted(NAMES)
    for name in declared:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert any(s.endswith("gcp_filter3d.hip") for s in _build.SRCS)  # the source hash covers it
    assert lib.gcp_abi_version() == _lib.ABI_VERSION


def test_the_entry_points_validate_before_any_hip_call():
    """Host memory stands in for device arrays: every call below must return before anything would read it."""
    import ctypes

    from simplegaussiansplat_tk71_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = [((ctypes.addressof(buf) + 63) & ~63) + 256 * k for k in range(9)]

    def rate(n=4, c=2, near=0.2, margin=0.15, ptrs=None):
        a = list(p[:5]) if ptrs is None else ptrs  # mean P K wh | rate
        return lib.gcp_filter3d_rate(a[0], a[1], a[2], a[3], n, c, near, margin, a[4], None)

    def apply(n=4, ptrs=None):
        a = list(p[:5]) if ptrs is None else ptrs  # log_scale opacity filter | the two outputs
        return lib.gcp_filter3d_apply(a[0], a[1], a[2], n, a[3], a[4], None)

    def backward(n=4, ptrs=None):
        a = list(p[:7]) if ptrs is None else ptrs
        return lib.gcp_filter3d_apply_backward(a[0], a[1], a[2], a[3], a[4], n, a[5], a[6], None)

    assert rate(n=0, ptrs=[None] * 5) == 0 and rate(c=0, ptrs=[None] * 5) == 0  # nothing to do: no launch, nothing touched
    assert apply(n=0, ptrs=[None] * 5) == 0 and backward(n=0, ptrs=[None] * 7) == 0
    assert rate(n=-1) == 1 and rate(c=-1) == 1 and rate(n=2 ** 31) == 1 and rate(c=2 ** 31) == 1
    assert apply(n=-1) == 1 and apply(n=2 ** 31) == 1 and backward(n=-1) == 1 and backward(n=2 ** 31) == 1
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert rate(near=bad) == 1 and rate(margin=bad) == 1 and rate(n=0, near=bad) == 1
    assert rate(margin=-0.1) == 1
    for call, n_ptrs in ((rate, 5), (apply, 5), (backward, 7)):
        for missing in range(n_ptrs):
            a = list(p[:n_ptrs])
            a[missing] = None
            assert call(ptrs=a) == 1, (call.__name__, missing)


# ---- the float64 formulation -------------------------------------------------------------------------------------------------------
def test_float64_formulation_conserves_mass():
    """sigmoid(x') prod s' = sigmoid(x) prod s to 1e-12 relative, over the whole domain and on every planted row."""
    w = {k: t.double() for k, t in ft.apply_world().items()}
    v_out, x_out, _, _ = ft.apply(w["v"], w["x"], w["phi"])
    assert torch.isfinite(v_out).all() and torch.isfinite(x_out).all()
    before = torch.sigmoid(w["x"]) * torch.exp(w["v"].sum(dim=1))
    after = torch.sigmoid(x_out) * torch.exp(v_out.sum(dim=1))
    rel = ((after - before).abs() / before).max()
    print("mass: worst relative difference", float(rel))
    assert float(before.min()) > 0 and float(rel) <= 1e-12
    # and the scale is what the formula says: s'^2 = s^2 + phi^2, to the same bound
    s2 = torch.exp(2 * w["v"]) + (w["phi"] ** 2)[:, None]
    assert float(((torch.exp(2 * v_out) - s2).abs() / s2).max()) <= 1e-12
    zero = w["phi"] == 0
    assert int(zero.sum()) >= 30 and torch.equal(v_out[zero], w["v"][zero]) and torch.equal(x_out[zero], w["x"][zero])


def test_float64_autograd_equals_the_closed_form_gradients():
    """To 1e-10 relative.  g_v is a sum of two terms that may cancel: relative to the sum of their absolute values.  g_x is one
    term in the closed form, but autograd through the formulation as stated forms it as g - g u / (1 + u) and is itself only
    good to 1e-16 (1 + u) of it (6e-8 at x = 20, measured): against that formulation relative to |g| + |g u / (1 + u)|, and
    against the formulation with the opacity as a logaddexp (the same values to 1e-12), whose autograd forms 1 / (1 + u)
    directly, relative to |g_x| itself."""
    w = {k: t.double() for k, t in ft.apply_world().items()}
    auto_v, auto_x = ft.apply_backward_autograd(w["v"], w["x"], w["phi"], w["g_v"], w["g_x"])
    g_v, g_x, scale_v, scale_x = ft.apply_backward(w["v"], w["x"], w["phi"], w["g_v"], w["g_x"])
    assert torch.isfinite(g_v).all() and torch.isfinite(g_x).all()
    terms_x = w["g_x"].abs() + (w["g_x"] - g_x).abs()
    print("closed forms against autograd as stated: g_v", ft.worst(auto_v, g_v, scale_v), "g_x", ft.worst(auto_x, g_x, terms_x),
          "(relative to |g_x| alone:", ft.worst(auto_x, g_x, scale_x), ")")
    assert ft.worst(auto_v, g_v, scale_v) <= 1e-10 and ft.worst(auto_x, g_x, terms_x) <= 1e-10
    v_out, x_out, s_v, s_x = ft.apply(w["v"], w["x"], w["phi"])
    v_st, x_st = ft.apply_stable(w["v"], w["x"], w["phi"])
    assert ft.worst(v_st, v_out, s_v) <= 1e-12 and ft.worst(x_st, x_out, s_x) <= 1e-12
    st_v, st_x = ft.apply_backward_autograd(w["v"], w["x"], w["phi"], w["g_v"], w["g_x"], ft.apply_stable)
    print("closed forms against autograd of the logaddexp form: g_v", ft.worst(st_v, g_v, scale_v), "g_x", ft.worst(st_x, g_x, scale_x))
    assert ft.worst(st_v, g_v, scale_v) <= 1e-10 and ft.worst(st_x, g_x, scale_x) <= 1e-10
    zero = w["phi"] == 0
    assert torch.equal(g_v[zero], w["g_v"][zero]) and torch.equal(g_x[zero], w["g_x"][zero])


def test_float32_restatement_is_finite_on_the_domain():
    """The yardstick itself: finite on every row, and within 1e-5 of float64 relative to the condition scales — were it not, four
    times its error would be no bound on a kernel."""
    w = ft.apply_world()
    ref = ft.apply(*(w[k].double() for k in ("v", "x", "phi")))
    got = ft.apply(w["v"], w["x"], w["phi"])
    assert all(torch.isfinite(t).all() for t in got[:2])
    err_v, err_x = ft.worst(got[0], ref[0], ref[2]), ft.worst(got[1], ref[1], ref[3])
    bref = ft.apply_backward(*(w[k].double() for k in ("v", "x", "phi", "g_v", "g_x")))
    bgot = ft.apply_backward(*(w[k] for k in ("v", "x", "phi", "g_v", "g_x")))
    assert all(torch.isfinite(t).all() for t in bgot[:2])
    err_gv, err_gx = ft.worst(bgot[0], bref[0], bref[2]), ft.worst(bgot[1], bref[1], bref[3])
    print("float32 restatement, in eps32: v'", err_v / ft.EPS32, "x'", err_x / ft.EPS32, "g_v", err_gv / ft.EPS32, "g_x", err_gx / ft.EPS32)
    assert 0 < max(err_v, err_x, err_gv, err_gx) <= 1e-5


# ---- the input conditions of the GPU tests -----------------------------------------------------------------------------------------
def test_apply_world_holds_its_planted_rows_and_stays_in_the_domain():
    w = ft.apply_world()
    assert all(t.dtype == torch.float32 and t.shape[0] == ft.WORLD_ROWS for t in w.values())
    v, x, phi = w["v"].double(), w["x"].double(), w["phi"].double()
    assert float(v.min()) >= -30 and float(v.max()) <= 10 and float(x.abs().max()) <= 20
    assert bool(((phi == 0) | ((phi >= 0.99e-6) & (phi <= 1e2))).all())
    r = (phi ** 2)[:, None] * torch.exp(-2 * v)
    assert float(phi[0]) == 0 and float(phi[6]) == 0
    assert float(r[1].max()) < 1e-20 and float(v[1].min()) == 10                      # r is lost against 1
    assert float(r[2].min()) > 1e29 and float(v[2].max()) == -30
    assert float(x[3]) == 20 and float(x[4]) == -20 and float(phi[3]) > 0
    assert float(r[5, 0]) > 1e6 and float(r[5, 1:].max()) < 1e-3                      # one axis far below phi, two far above
    both = ((r > 1e-3) & (r < 1e3)).any(dim=1)
    assert int(both.sum()) >= 100                                                    # rows where neither term is negligible
    for n in ft.APPLY_SIZES:  # every size is the first n rows of the one world
        part = ft.apply_world(n)
        assert all(torch.equal(part[k], w[k][:n]) for k in w)


@pytest.mark.parametrize("n_cam", RATE_CAMERAS)
def test_rate_world_is_clear_of_every_decision_boundary_and_holds_its_planted_rows(n_cam):
    mean, P, K, wh = ft.rate_world(n_cam)
    assert mean.shape == (ft.WORLD_ROWS, 3) and mean.dtype == torch.float32 and P.shape == (n_cam, 3, 4) and wh.dtype == torch.int32
    ref = ft.rate(mean, P, K, wh)
    print(n_cam, "cameras: smallest clearance", float(ref["clearance"].min()), "rows seen", int(ref["seen"].any(dim=1).sum()),
          "largest rate tolerance", float(ft.rate_tolerance(ref).max()))
    assert float(ref["clearance"].min()) > ft.CLEARANCE  # ZERO rows left out: float64 alone decides every (row, camera)
    assert ft.CLEARANCE > 100 * ft.EPS32  # a float32 evaluation is off by a few eps32 of the same sums
    seen, tz = ref["seen"], ref["tz"]
    last = n_cam - 1
    assert not seen[0].any() and bool((tz[0] <= ft.NEAR).all())                         # behind every camera
    only_last = torch.zeros(n_cam, dtype=torch.bool)
    only_last[last] = True
    W = float(wh[last, 0])
    assert torch.equal(seen[1], only_last) and W < float(ref["u"][1, last]) < (1 + ft.BAND) * W     # in the margin band only
    assert torch.equal(seen[2], only_last) and 0 < float(ref["u"][2, last]) < W                  # in the image of the last camera only
    assert not seen[3].any() and (n_cam == 1 or bool((tz[3] > ft.NEAR).any()))                   # in front of some, seen by none
    n_seen = int(seen.any(dim=1).sum())
    assert 60 <= n_seen <= ft.WORLD_ROWS - 40  # both outcomes are well represented
    # the cameras differ, fx != fy, and the skew is there to be ignored
    assert bool((K[:, 0, 0] != K[:, 1, 1]).all()) and bool((K[:, 0, 1] != 0).all())
    if n_cam > 1:
        assert len({tuple(r) for r in wh.tolist()}) > 1 and len(set(K[:, 0, 0].tolist())) > 1
    assert float(ft.rate_tolerance(ref).max()) < 1e-3 and float(ref["rate"].max()) > 0
