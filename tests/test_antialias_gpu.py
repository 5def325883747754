"""Opacity compensation of the covariance dilation on the GPU (csrc/gcp_splat.hip with GCP_SPLAT_ANTIALIAS, gs_model's
`antialias`): opacity = sigmoid(o) rho, rho = sqrt(det Sigma / det Sigma'), against the PyTorch formulation of
tests/test_splat_gpu.py with rho formed from the same clamped covariance and invert_2x2_batch's det + 1e-6
(`formulation(antialias=True)`, `compensation`); what the option must leave alone; degenerate covariances; the energy of a
splat; and end to end.
The per-row checks of rho and its gradient chain — the row rule against float64, sub-pixel, large and thin splats, pixel
centres, the edge scene, position and alignment — live in tests/test_projection_rows_gpu.py."""
import math

import numpy as np
import pytest
import torch

from oracle import dense_render as dr
from simplegaussiansplat_tk71_amd import gs_model as gm
from tests import test_projection_rows_gpu as row_checks
from tests.test_sh3_gpu import NAMES, SHAPES, TILE_LOGIT, random_world, torch_sh
from tests.test_splat_gpu import formulation, small_model, world
from tests.util import assert_parity

pytestmark = pytest.mark.gpu

DILATION = 0.3
# (options of gm.camera_inputs besides antialias, SH degree, frame)
CONFIGS = {"subpixel-dilated-deg2-camera": ({"centres": "subpixel", "cov_dilation": DILATION}, 2, "camera"),
           "all-deg3-world": ({"centres": "subpixel", "cov_dilation": DILATION, "clamp_colour": True}, 3, "world")}
OUTPUTS = ("variance_inverse", "opacity", "l_d", "mean")
IDS = dict(ids=lambda s: "x".join(map(str, s)))


def antialiased_formulation(leaves, w, degree, frame, options, fixed, dtype):
    """tests/test_splat_gpu.formulation(antialias=True) in `dtype` on the lists `fixed`: its "opacity" is sigmoid(o) rho.
    -> (cams, rho (C, N), det0 (C, N))"""
    P, K = w["P"].to(dtype), w["K"].to(dtype)
    cams, _ = formulation(*(leaves[k] for k in NAMES), P, K, w["wh"], TILE_LOGIT, degree, torch_sh(frame, P), cov_eps=options["cov_dilation"],
                          clamp_colour=options.get("clamp_colour", False), fixed=fixed, antialias=True)
    return cams, torch.stack([cam["rho_all"] for cam in cams]), torch.stack([cam["det0_all"] for cam in cams])


def upstream_loss(cams, n, upstream, seed=1):
    """sum_k <cam[k], random per Gaussian> over `upstream`; the draws are made for every output, so they are the same whatever
    `upstream` is and whichever side (kernels, formulation, dtype) asks."""
    gen = torch.Generator().manual_seed(seed)
    loss = 0
    for cam in cams:
        for k in OUTPUTS:
            g = torch.randn((n, *cam[k].shape[1:]), generator=gen).to(cam[k].device)[cam["index"]]
            if k in upstream:
                loss = loss + (cam[k] * g.to(cam[k].dtype)).sum()
    return loss


def fused(w, config, antialias, with_depth=False, grad=False):
    options, degree, frame = CONFIGS[config]
    leaves = {k: w[k].clone().requires_grad_(grad) for k in NAMES}
    cams, grad_iter, _ = gm.camera_inputs(*(leaves[k] for k in NAMES), w["P"], w["K"], w["wh"], TILE_LOGIT, L_max=degree, sh_frame=frame,
                                          with_depth=with_depth, antialias=antialias, **options)
    return cams, grad_iter, leaves


# ---- 1. nothing else moves ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_only_the_opacity_changes(shape, config, device):
    """Every entry of every camera but "opacity" — index, startpoint, endpoint, boxsize, mean, variance_inverse, l_d, depth —
    and grad_iter are bit-equal with the option on and off; "opacity" is never larger and is smaller somewhere."""
    w = world(shape, device)
    with torch.no_grad():
        on, g_on, _ = fused(w, config, True, with_depth=True)
        off, g_off, _ = fused(w, config, False, with_depth=True)
    assert torch.equal(g_on, g_off) and len(on) == len(off) == shape[1]
    for a, b in zip(on, off):
        assert a.keys() == b.keys() and "depth" in a
        for k in ("index", "startpoint", "endpoint", "boxsize", "mean", "variance_inverse", "l_d", "depth"):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        assert bool((a["opacity"] <= b["opacity"]).all()) and bool((a["opacity"] < 0.999 * b["opacity"]).any())
        assert bool((a["opacity"] >= 0).all())


@pytest.mark.parametrize("frame", ("camera", "world"))
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_flags_with_the_clamp_bit_alone_is_the_old_entry_point(shape, frame, device):
    """gcp_splat_forward_flags(flags = GCP_SPLAT_CLAMP_COLOUR) writes the record, sort key, keep and row_of of
    gcp_splat_forward(clamp_colour = 1) bit for bit (and flags = 0 those of clamp_colour = 0); with GCP_SPLAT_ANTIALIAS
    added only word 10 of the record, the opacity, differs."""
    from simplegaussiansplat_tk71_amd import _lib

    n, _, width, height = shape
    w = world(shape, device)
    lib = _lib.load()
    params = [w[k].contiguous() for k in NAMES] + [w["P"][0].contiguous(), w["K"][0].contiguous()]
    clamp = gm._box_clamp(width, height, TILE_LOGIT)

    def run(entry, last):
        record = torch.full((n, 16), float("nan"), dtype=torch.float32, device=device)
        sort_key, row_of = (torch.full((n,), 12345, dtype=torch.int32, device=device) for _ in range(2))
        keep = torch.full((n,), 7, dtype=torch.uint8, device=device)
        _lib.check(getattr(lib, entry)(*(t.data_ptr() for t in params), n, 3, 16, gm.SH_FRAMES[frame], width, height, clamp, DILATION, 0.5, last,
                                       record.data_ptr(), sort_key.data_ptr(), keep.data_ptr(), row_of.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), entry)
        torch.cuda.synchronize()
        return record.view(torch.int32), sort_key, keep, row_of

    for bit in (0, 1):
        old, new = run("gcp_splat_forward", bit), run("gcp_splat_forward_flags", bit)
        for a, b in zip(old, new):
            assert torch.equal(a, b), bit
        aa = run("gcp_splat_forward_flags", bit | _lib.SPLAT_ANTIALIAS)
        others = [c for c in range(16) if c != 10]
        assert torch.equal(aa[0][:, others], old[0][:, others]) and not torch.equal(aa[0][:, 10], old[0][:, 10])
        for a, b in zip(old[1:], aa[1:]):
            assert torch.equal(a, b), bit


# ---- 2. rho and its gradient against the PyTorch formulation ----------------------------------------------------------------------
def _reference_run(w, config, cams, upstream, dtype):
    options, degree, frame = CONFIGS[config]
    n = w["mean"].shape[0]
    leaves = {k: w[k].to(dtype).clone().requires_grad_(True) for k in NAMES}
    fixed = [(cam["index"], cam["startpoint"], cam["endpoint"]) for cam in cams]
    ref, rho, det0 = antialiased_formulation(leaves, w, degree, frame, options, fixed, dtype)
    upstream_loss(ref, n, upstream).backward()
    ref = [{k: v.detach() for k, v in cam.items()} for cam in ref]
    # a leaf the loss does not depend on (the colour, with "opacity" alone) has no gradient: zero
    return ref, rho.detach(), det0.detach(), {k: torch.zeros_like(v) if v.grad is None else v.grad for k, v in leaves.items()}


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_opacity_and_gradients_equal_the_torch_formulation(shape, config, device):
    """On the lists the kernels made (fixed=: every kept Gaussian is compared, none left out), "opacity" is the float32
    formulation's within the rtol 2e-4 / atol 1e-6 the project holds this output to, and all five parameter gradients — random
    upstream gradients on all four outputs, then on "opacity" alone, which isolates the rho chain — stay within 5e-4 of the
    largest entry of the float64 formulation's gradient; with "opacity" alone color.grad is exactly zero.
    Printed before they are asserted: the kernel's and the float32 formulation's deviation from float64, for rho (as
    opacity / sigmoid) and for both gradients.  float32 formulation against float64 on the CPU: rho 2.6e-7 absolute, the rho
    chain's gradient 1.2e-6 of its scale; the kernel on the MI355X: profiles/r14_antialias.md."""
    w = world(shape, device)
    n = shape[0]
    tag = (shape, config)
    for upstream in (OUTPUTS, ("opacity",)):
        cams, _, leaves = fused(w, config, True, grad=True)
        upstream_loss(cams, n, upstream).backward()
        got = {k: v.grad for k, v in leaves.items()}
        cams = [{k: v.detach() for k, v in cam.items()} for cam in cams]
        r32, _, _, g32 = _reference_run(w, config, cams, upstream, torch.float32)
        r64, rho64, det0, g64 = _reference_run(w, config, cams, upstream, torch.float64)
        if upstream is OUTPUTS:
            for c, (a, b, d) in enumerate(zip(cams, r32, r64)):
                kept0 = det0[c, a["index"]]
                print(tag, "camera", c, "kept", a["index"].numel(), "det0 <= 0:", int((kept0 <= 0).sum()), "det0 < 1e-4:", int((kept0 < 1e-4).sum()),
                      "rho min / median / max", float(rho64[c, a["index"]].min()), float(rho64[c, a["index"]].median()),
                      float(rho64[c, a["index"]].max()))
                sig = torch.sigmoid(w["opacity"].double())[a["index"]]
                print(tag, "rho: kernel vs float64", float((a["opacity"].double() / sig - d["opacity"] / sig).abs().max()),
                      "| float32 formulation vs float64", float((b["opacity"].double() / sig - d["opacity"] / sig).abs().max()))
                print(tag, "opacity: kernel vs float32 formulation, max abs diff", float((a["opacity"] - b["opacity"]).abs().max()))
                torch.testing.assert_close(a["opacity"], b["opacity"], rtol=2e-4, atol=1e-6)
                for k in ("variance_inverse", "l_d"):
                    torch.testing.assert_close(a[k], b[k], rtol=2e-4, atol=1e-6)
        for k in NAMES:
            scale = float(g64[k].abs().max())
            err = float((got[k].double() - g64[k]).abs().max())
            print(tag, "upstream", "all" if upstream is OUTPUTS else "opacity", "grad", k, "kernel err / scale", err / scale if scale else err,
                  "| float32 formulation", float((g32[k].double() - g64[k]).abs().max()) / scale if scale else 0.0, "scale", scale)
            if upstream is not OUTPUTS and k == "color":
                assert scale == 0.0 and float(got[k].abs().max()) == 0.0
                continue
            assert scale > 0, k
            assert err <= 5e-4 * scale, (k, err, scale)


# ---- 3. degenerate rows ----------------------------------------------------------------------------------------------------------
def _degenerate_scene(device):
    """60 ordinary Gaussians in front of one hand-made camera on the z axis (P = [I | (0, 0, 3.2)]), and three more on its
    optical axis, placed between them so that every lane after the first moves:
      A  all log-scales -50: every entry of the pixel covariance underflows, det0 = 0;
      B  log-scale -50 on its x axis only, unrotated: a disc seen edge-on — the covariance is diag(~1e-41, d), det0 a
         denormal or 0;
      C  the same disc turned 30 degrees about the view axis: a rank-1 covariance with all four entries of ordinary size,
         det0 = a d - b c is what rounding leaves, of either sign."""
    width, height, n = 40, 30, 60
    w = random_world(n, 1, width, height, 41, device, n_basis=9)
    P = torch.eye(3, 4)[None].clone()
    P[0, 2, 3] = 3.2
    w["P"] = P.to(device)
    extra = {"mean": torch.zeros(3, 3), "variance_q": torch.tensor([[0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0, 1.0],
                                                                     [0.0, 0.0, math.sin(math.pi / 12), math.cos(math.pi / 12)]]),
             "variance_scale": torch.tensor([[-50.0, -50.0, -50.0], [-50.0, math.log(0.18), math.log(0.1)], [-50.0, math.log(0.18), math.log(0.1)]]),
             "opacity": torch.zeros(3, 1), "color": 0.5 * torch.ones(3, 9, 3)}
    at = (5, 17, 40)  # rows of A, B, C in the combined scene
    ordinary = [i for i in range(n + 3) if i not in at]
    both = {}
    for k in NAMES:
        t = torch.empty((n + 3, *w[k].shape[1:]), device=device)
        t[ordinary] = w[k]
        t[list(at)] = extra[k].to(device)
        both[k] = t
    return w, both, at, ordinary


def test_degenerate_covariances(device):
    """Row A (det0 = 0) has "opacity" exactly 0; B and C, whose det0 is at most what rounding leaves of a rank-1 matrix
    (|det0| <= a few 2^-24 a d ~ 1e-5 here, det >= 0.3 d ~ 1.2: rho <= 3e-3), have an opacity below 1e-2 sigmoid(o), and
    wherever an opacity is exactly 0 the logit's gradient is exactly 0.  Every output and every gradient of every row is
    finite, and the ordinary rows — outputs and gradients — are bit-equal to the scene without the three.
    With "opacity" alone upstream the three are also held one by one: the logit identity, an exactly zero gradient row in every
    parameter where rho is exactly 0, and the rank-deficient row's bound on rho (the comment in the body)."""
    w, both, at, ordinary = _degenerate_scene(device)
    n = len(ordinary)
    opts = dict(L_max=2, centres="subpixel", cov_dilation=DILATION, antialias=True, with_depth=True)
    gen = torch.Generator().manual_seed(3)
    ups = {k: torch.randn((n + 3, *shape), generator=gen).to(device) for k, shape in
           (("variance_inverse", (2, 2)), ("opacity", (1,)), ("l_d", (3,)), ("mean", (2,)), ("depth", ()))}

    def run(params, ids, upstream=tuple(ups)):
        """ids: the combined scene's row of every Gaussian of `params` -> per-Gaussian outputs and gradients"""
        leaves = [params[k].clone().requires_grad_(True) for k in NAMES]
        cams, grad_iter, _ = gm.camera_inputs(*leaves, w["P"], w["K"], w["wh"], TILE_LOGIT, **opts)
        cam = cams[0]
        ids = torch.tensor(ids, device=device)
        sum(((cam[k] * ups[k][ids[cam["index"]]]).sum() for k in upstream)).backward()
        cam = {k: v.detach() for k, v in cam.items()}
        rows = torch.full((len(ids),), -1, dtype=torch.long, device=device)
        rows[cam["index"]] = torch.arange(cam["index"].numel(), device=device)
        return cam, rows, grad_iter, [t.grad for t in leaves]

    cam, rows, kept, grads = run(both, list(range(n + 3)))
    ref, rows_ref, kept_ref, grads_ref = run({k: w[k] for k in NAMES}, ordinary)
    assert bool(kept[list(at)].all())  # the three are in the list: 0.3 px^2 of dilation is all their box is made of
    for k in ("variance_inverse", "opacity", "l_d", "mean", "depth"):
        assert bool(torch.isfinite(cam[k]).all()), k
    for g, k in zip(grads, NAMES):
        assert bool(torch.isfinite(g).all()), k
    alpha = cam["opacity"][rows[list(at)], 0]
    print("opacity of A, B, C:", alpha.tolist(), "| gradients of their logits:", grads[3][list(at), 0].tolist())
    print("largest gradient entry of A, B, C per parameter:", [float(g[list(at)].abs().max()) for g in grads])
    assert float(alpha[0]) == 0.0
    assert bool((alpha >= 0).all()) and bool((alpha <= 1e-2 * 0.5).all())
    zero = cam["opacity"][:, 0] == 0
    assert float(grads[3][cam["index"][zero]].abs().max()) == 0.0
    # the three rows one by one, with "opacity" alone upstream (tests/test_projection_rows_gpu.py's conditions on a row whose
    # det0 is round-off).  Rank-deficient by that file's definition, det0 <= 2^-20 a0 d0 in float64 on the float32 parameters,
    # is C alone: A and B are diagonal covariances, whose det0 = a0 d0 is exact in any precision that holds it (float64:
    # rho = 1e-40 and 3.9e-21; in float32 A underflows to 0 and B's a0 is a denormal of three bits).  So the bound
    # rho <= sqrt(2^-20 a0 d0 / det) is C's; all three are held to rho >= 0, the logit identity at 4 x the float32
    # formulation's own figure on this scene, finite gradients, and an exactly zero gradient row in every parameter where
    # the kernel's rho is exactly 0 (A, by the assertion above; on the MI355X also C: profiles/r26_antialias_rows.md).
    cam_o, _, _, grads_o = run(both, list(range(n + 3)), upstream=("opacity",))
    host = {k: both[k].cpu() for k in NAMES}
    host.update(P=w["P"].cpu(), K=w["K"].cpu(), wh=w["wh"].cpu())
    cfg = ("splat", {"centres": "subpixel", "cov_dilation": DILATION, "antialias": True}, 2, 9, "camera", True)
    fixed = row_checks.lists_of([cam_o])
    _, c64 = row_checks.run_formulation(host, cfg, torch.float64, fixed)
    l32, c32 = row_checks.run_formulation(host, cfg, torch.float32, fixed)
    up = ups["opacity"].cpu()[None]
    f32 = row_checks.path_gradients(l32, c32, {"opacity": up}, ("opacity",))["opacity"]
    got = {k: (torch.zeros_like(both[k]) if g is None else g).detach().cpu().double().reshape(n + 3, -1) for k, g in zip(NAMES, grads_o)}
    deficient = row_checks.rank_deficient(c64)
    print("rank-deficient rows of the scene:", sorted(deficient), "| A, B, C are", at, "| float64 rho of the three", c64[0]["rho_all"][list(at)].tolist())
    assert deficient == {at[2]}
    failures = []
    row_checks.check_logit_identity("degenerate scene", host, [cam_o], got["opacity"], c32, f32["opacity"], up, failures)
    dark = row_checks.check_nothing_passes_a_zero("degenerate scene", n + 3, [cam_o], got, failures)
    row_checks.check_rank_deficient_rows("degenerate scene", [at[2]], [cam_o], c64, host["opacity"], failures)
    print("rows whose rho is exactly 0:", dark.nonzero().flatten().tolist())
    assert bool(dark[at[0]]) and all(bool(torch.isfinite(got[k][list(at)]).all()) for k in NAMES)
    assert not failures, "\n".join(failures)
    # the ordinary rows do not notice their neighbours
    o = torch.tensor(ordinary, device=device)
    assert torch.equal(kept[o], kept_ref)
    seen = kept_ref.nonzero().flatten()
    assert seen.numel() >= 30
    for k in ("variance_inverse", "opacity", "l_d", "mean", "depth", "startpoint", "endpoint"):
        assert torch.equal(cam[k][rows[o[seen]]], ref[k][rows_ref[seen]]), k
    for g, g_ref, k in zip(grads, grads_ref, NAMES):
        assert torch.equal(g[o], g_ref), k


# ---- 4. energy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma_px", (0.2, 0.5, 1.0, 2.0))
def test_a_splat_keeps_the_energy_it_had_before_the_dilation(sigma_px, device):
    """One isotropic Gaussian on the optical axis of a 64 x 64 camera, sigmoid(o) = 0.5, pixel covariance (f s / z)^2 I =
    sigma_px^2 I.  With antialias the alpha map sums to 2 pi 0.5 sqrt(det0) within 3 %: the 3 sigma' box loses at most
    exp(-4.5) = 1.1 % of the mass, and sampling a Gaussian of sigma' >= 0.55 px on the pixel grid adds at most
    2 exp(-2 pi^2 sigma'^2) = 0.6 %.  Without it the sum is 1 / rho times that (8.5 x at 0.2 px): the ratio of the two sums is
    rho within 1e-4."""
    import cuda_kernel as ck

    size, f, z = 64, 64.0, 4.0
    s = sigma_px * z / f
    P = torch.eye(3, 4)[None].clone()
    P[0, 2, 3] = z
    K = torch.tensor([[[f, 0.0, size / 2], [0.0, f, size / 2], [0.0, 0.0, 1.0]]])
    params = [torch.zeros(1, 3), torch.tensor([[0.0, 0.0, 0.0, 1.0]]), torch.full((1, 3), math.log(s)), torch.zeros(1, 1), torch.ones(1, 9, 3)]
    params = [t.to(device) for t in params]
    sums = {}
    with torch.no_grad():
        for antialias in (True, False):
            cams, _, (wd, ht) = gm.camera_inputs(*params, P.to(device), K.to(device), [[size, size]], TILE_LOGIT, with_depth=True,
                                                 centres="subpixel", cov_dilation=DILATION, antialias=antialias)
            cam = cams[0]
            assert cam["index"].numel() == 1
            _, _, alpha = ck.render(cam["startpoint"], cam["endpoint"], cam["mean"], cam["variance_inverse"], cam["opacity"], cam["l_d"],
                                    cam["depth"], wd, ht)
            sums[antialias] = float(alpha.double().sum())
    var = (f * s / z) ** 2
    det0 = var * var
    det = (var + DILATION) ** 2 + 1e-6
    rho = math.sqrt(det0 / det)
    want = 2 * math.pi * 0.5 * math.sqrt(det0)
    print("sigma", sigma_px, "px: alpha sum with antialias", sums[True], "expected", want, "ratio", sums[True] / want, "| without",
          sums[False], "| ratio of the sums", sums[True] / sums[False], "rho", rho)
    assert abs(sums[True] / want - 1) <= 0.03
    assert abs(sums[True] / sums[False] / rho - 1) <= 1e-4


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------
def test_model_forward_and_mean_gradient_against_the_dense_oracle(device):
    """tests/test_splat_gpu.py's model test with antialias=True: the image is the dense float64 renderer's on the kernel's own
    lists within the absolute 1e-5 of colour, and mean.grad of <image, G> is float64 autograd through the formulation with rho
    and the dense renderer, lists and boxes held at the kernel's, under |got - want| <= 1e-5 (1 + |want| + mean |want|).
    The image is not the one the model renders without the option."""
    model, w, width, height = small_model(device, centres="subpixel", cov_dilation=DILATION, antialias=True)
    G = torch.randn(1, 3, height, width, generator=torch.Generator().manual_seed(2))
    images, _, _ = model(w["P"], w["K"], w["wh"], ["a"])
    (images * G.to(device)).sum().backward()
    with torch.no_grad():
        cam = model.camera_inputs(w["P"], w["K"], w["wh"])[0][0]
        plain = small_model(device, centres="subpixel", cov_dilation=DILATION)[0](w["P"], w["K"], w["wh"], ["a"])[0]
    assert float((images.detach() - plain).abs().max()) > 1e-3
    assert cam["index"].numel() >= 24
    host = {k: v.cpu() for k, v in cam.items()}
    want = dr.render(host["startpoint"], host["endpoint"], host["mean"], host["variance_inverse"], host["opacity"], host["l_d"], width, height,
                     dtype=torch.float64)[1:, 1:].permute(2, 0, 1)[None]
    assert_parity(images, want, None, "image")

    leaves = {k: getattr(model, k).detach().cpu().double().requires_grad_(k == "mean") for k in NAMES}
    w_host = {"P": w["P"].cpu(), "K": w["K"].cpu(), "wh": w["wh"].cpu()}
    c64, _, _ = antialiased_formulation(leaves, w_host, 2, "camera", {"cov_dilation": DILATION},
                                        [(host["index"], host["startpoint"], host["endpoint"])], torch.float64)
    c = c64[0]
    torch.testing.assert_close(c["opacity"].detach().float(), host["opacity"], rtol=2e-4, atol=1e-6)
    img64 = dr.render(c["startpoint"], c["endpoint"], c["mean"], c["variance_inverse"], c["opacity"], c["l_d"], width, height,
                      dtype=torch.float64)[1:, 1:].permute(2, 0, 1)[None]
    (img64 * G.double()).sum().backward()
    g64 = leaves["mean"].grad
    got = model.mean.grad.cpu().double()
    print("mean.grad: largest", float(g64.abs().max()), "mean", float(g64.abs().mean()), "max err", float((got - g64).abs().max()))
    assert float(g64.abs().max()) > 0
    assert_parity(got, g64, g64.abs() + g64.abs().mean(), "mean.grad")


def test_captured_step_with_antialias_equals_the_eager_step(device):
    """tests/test_splat_gpu.py's captured step with antialias=True: capture-safe lists through GraphedStep, replayed on moved
    Gaussians — image and all five parameter gradients bit-equal to the eager step."""
    import cuda_kernel as ck

    n, width, height = 2000, 64, 48
    w = random_world(n, 2, width, height, 13, device)
    wh_host = [[width, height]] * 2
    target_f = torch.rand(2, height + 1, width + 1, 3, device=device)

    def run(leaves, capture_safe, with_grads=True):
        cams, _, (wd, ht) = gm.camera_inputs(*leaves, w["P"], w["K"], wh_host if capture_safe else w["wh"], TILE_LOGIT, L_max=3,
                                             capture_safe=capture_safe, sh_frame="world", centres="subpixel", cov_dilation=DILATION,
                                             clamp_colour=True, antialias=True)
        img = torch.stack([ck.custom_autograd_grouped_cumprod.apply(cam["boxsize"], None, cam["startpoint"], cam["endpoint"], cam["mean"],
                                                                    cam["variance_inverse"], cam["opacity"], cam["l_d"], wd, ht)
                           for cam in cams])
        loss = ((img - target_f) ** 2).sum()
        return (loss, img) if not with_grads else (img, torch.autograd.grad(loss, leaves))

    leaves = [w[k].clone().requires_grad_(True) for k in NAMES]
    step = ck.GraphedStep(lambda *ls: run(list(ls), True, with_grads=False), leaves, capacity=16 * n)
    with torch.no_grad():
        leaves[0].add_(0.05 * torch.randn_like(leaves[0]))
        leaves[4].mul_(0.9)
    (_, got_img), got_grads = step.replay()
    torch.cuda.synchronize()
    assert not ck.capacity_exceeded()
    got_img, got_grads = got_img.clone(), [g.clone() for g in got_grads]
    img, grads = run(leaves, False)
    assert torch.equal(got_img, img)
    for a, b, k in zip(got_grads, grads, NAMES):
        assert torch.equal(a, b), k


# ---- 6. the example ----------------------------------------------------------------------------------------------------------------
def test_training_with_antialias_learns(device):
    from examples.train_cameras import synthetic_scene, train

    start, P, K, wh, targets = synthetic_scene(600, 6, 64, 48, 0, device)
    model, losses = train(start, P, K, wh, targets, iterations=30, log=lambda *_: None, centres="subpixel", dilation=DILATION, antialias=True)
    assert model.antialias is True and len(losses) == 30
    assert all(math.isfinite(l) for l in losses)
    print("loss: first five", np.mean(losses[:5]), "last five", np.mean(losses[-5:]))
    assert np.mean(losses[-5:]) < np.mean(losses[:5])
