"""The conditions tests/test_projection_rows_gpu.py puts on its inputs, checked where no GPU is needed: on every world, shape and
configuration of that file the float32 formulation agrees with the float64 one to 1e-3 of every row (so that the row rule's
measured term stays a round-off term), the hand-built edge scene keeps and culls exactly the rows it is meant to, and both
precisions are finite on every row.  The float32 formulation's own lists stand in for the kernels'."""
import pytest
import torch

from oracle import gs_forward_torch as gft
from tests.test_projection_rows_gpu import (BIG, CASES, CLAMP_LOG_SCALE, CONFIGS, EDGE_CONFIGS, EDGE_CULLED, EDGE_RANK_DEFICIENT, EDGE_ROWS, MARGIN,
                                            NAMES, ROW_CASES, RTOL, SHAPES, SIZES, row_case_id, check_case, edge_scene, lists_of, path_gradients, paths_of,
                                            position_config, row_norm, run_formulation, shape_id, sub_world, upstreams, world)


def own_lists_run(w, cfg):
    """The float32 formulation on its own lists -> (leaves, cams), in the place of the kernels."""
    with torch.no_grad():
        _, cams = run_formulation(w, cfg, torch.float32)
    return run_formulation(w, cfg, torch.float32, lists_of(cams))


@pytest.mark.parametrize("shape,case", ROW_CASES, ids=row_case_id)
def test_float32_formulation_stays_under_the_cap(shape, case, capsys):
    """Every (configuration, kind of world, shape) of the GPU file.  Under antialias also: det0 > 0 in float32 and in float64
    on every kept row (no row of a world is rank-deficient: `check_case`), and rho is where the kind is meant to put it: a
    median below 0.05 on the subpixel worlds, above 0.9 on the large ones.  Prints rho min / median / max per camera."""
    config, kind = CASES[case]
    cfg = CONFIGS[config]
    w = world(shape, cfg[3], kind)
    failures = []
    leaves, cams = own_lists_run(w, cfg)
    got, want, _ = check_case(f"{shape_id(shape)} {case}", w, cfg, (leaves, cams), failures, median=False, who="(float32 again)")
    assert not failures, "\n".join(failures)
    for path in paths_of(cfg):
        assert all(torch.isfinite(g[path][k]).all() for g in (got, want) for k in NAMES)
    if cfg[1].get("antialias"):
        _, c64 = run_formulation(w, cfg, torch.float64, lists_of(cams))
        for c, (a, b) in enumerate(zip(cams, c64)):
            index = a["index"]
            assert bool((a["det0_all"][index] > 0).all()) and bool((b["det0_all"][index] > 0).all())
            rho = b["rho_all"].detach()[index]
            print(f"RHO {shape_id(shape)} {case} camera {c}: kept {index.numel()} | rho min {float(rho.min()):.2e} median {float(rho.median()):.2e} "
                  f"max {float(rho.max()):.2e}")
            if kind == "subpixel":
                assert float(rho.median()) < 0.05
            if kind == "large":
                assert float(rho.median()) > 0.9


@pytest.mark.parametrize("family", EDGE_CONFIGS)
def test_edge_scene_keeps_and_culls_what_it_is_meant_to(family):
    cfg = EDGE_CONFIGS[family]
    w, row = edge_scene()
    assert sorted(row) == sorted(EDGE_ROWS) and all(torch.isfinite(w[k]).all() for k in NAMES if k != "opacity")
    leaves, cams = own_lists_run(w, cfg)
    assert set(cams[0]["index"].tolist()) == {row[k] for k in EDGE_ROWS if k not in EDGE_CULLED}
    depth = {int(i): float(z) for i, z in zip(cams[0]["index"], cams[0]["depth"])}
    assert 0 < depth[row["depth 0.005"]] < 1e-2 < depth[row["depth just above 1e-2"]] < 1.1e-2
    # the culled ones: depth exactly 0 with the product rounded before the sum, and never positive
    P = w["P"][0]
    z = (w["mean"][row["depth 0"]] * P[2, :3])
    assert float((z[0] + z[1]) + z[2] + P[2, 3]) == 0.0
    assert float((w["mean"].double() @ P[2, :3].double() + P[2, 3].double())[row["depth 0"]]) <= 0.0
    failures = []
    antialias = cfg[1].get("antialias", False)
    got, want, f32 = check_case(f"edge {family}", w, cfg, (leaves, cams), failures, median=False, who="(float32 again)", cap=False,
                                deficient=[row[k] for k in EDGE_RANK_DEFICIENT] if antialias else ())
    assert not failures, "\n".join(failures)
    if antialias:  # what EDGE_RANK_DEFICIENT's comment says of the two rows float32 cannot follow float64 on
        _, c64 = run_formulation(w, cfg, torch.float64, lists_of(cams))
        a, b = cams[0], c64[0]
        i, j = row["covariance clamp"], row["needle"]
        print("edge", family, "covariance clamp: float64 det0, det", float(b["det0_all"][i]), float(b["det_all"][i]), "| float32 rho", float(a["rho_all"][i]),
              "| needle: float64 det0 / (a0 d0)", float(b["det0_all"][j] / (b["cov0_all"][j, 0, 0] * b["cov0_all"][j, 1, 1])), "rho", float(b["rho_all"][j]),
              "| float32 d0, det0, rho", float(a["cov0_all"][j, 1, 1]), float(a["det0_all"][j]), float(a["rho_all"][j]))
        assert float(b["det0_all"][i]) < 0 and float(b["det_all"][i]) < 0 and float(b["rho_all"][i]) == 0.0
        a0 = float(a["cov0_all"][i, 0, 0])
        assert abs(float(a["cov0_all"][i, 0, 1])) < 1e-2 and float(a["rho_all"][i]) == pytest.approx((a0 / (a0 + 0.3)) ** 0.5, rel=1e-6)
        assert float(b["det0_all"][j]) > 0.5 * float(b["cov0_all"][j, 0, 0] * b["cov0_all"][j, 1, 1]) and 1e-6 < float(b["rho_all"][j]) < 1e-5
        assert 0.0 <= float(a["rho_all"][j]) <= 5 * float(b["rho_all"][j])  # the row rule's reach with the float32 formulation at 0
        for cam in (a, b):
            assert torch.isfinite(cam["rho_all"][cam["index"]]).all()
    for path in got:
        for k in NAMES:
            assert torch.isfinite(f32[path][k]).all(), (path, k)
            if antialias and path == "opacity":  # EDGE_RANK_DEFICIENT: float64 has det < 0 there and no gradient of rho
                assert bool(torch.isnan(want[path][k][i]).any()) == (k in ("mean", "variance_q", "variance_scale")), k
                assert torch.isfinite(want[path][k][:i]).all(), k
            else:
                assert torch.isfinite(want[path][k]).all(), (path, k)
            for name in EDGE_CULLED:
                assert float(want[path][k][row[name]].abs().max()) == 0.0
        for side in (want, f32):
            assert float(side[path]["variance_q"][row["q = 0"]].abs().max()) == 0.0
            assert float(side[path]["opacity"][row["opacity +100"]].abs().max()) == 0.0
            assert float(side[path]["opacity"][row["opacity -inf"]].abs().max()) == 0.0
    assert float(want["variance_inverse"]["variance_q"][row["|q| = 1e-9"]].abs().max()) > 1e5
    assert float(want["l_d"]["color"][row["zero SH"]].abs().max()) > 0
    for cam in (cams[0],):
        for key in ("variance_inverse", "opacity", "l_d", "depth", "mean"):
            assert torch.isfinite(cam[key]).all(), key


def test_row_rule_resolves_one_wrong_degree_3_constant(monkeypatch):
    """The resolution of the row rule.  The float64 formulation with ONE degree-3 constant off by a quarter (the z (xx - yy)
    term) stands in for the kernel: most rows of l_d -> mean fall outside the rule.  Printed beside it: how many rows the
    per-tensor bound the suite had (5e-4 of the largest entry of mean.grad with all paths summed) would have noticed."""
    import tests.test_sh3_gpu as sh3

    cfg = CONFIGS["splat-all-deg3of16-world-depth"]
    shape = SHAPES[1]
    w = world(shape, 16)
    fixed = lists_of(own_lists_run(w, cfg)[1])
    ups, paths = upstreams(w, cfg), paths_of(cfg)
    want = path_gradients(*run_formulation(w, cfg, torch.float64, fixed), ups, paths)
    f32 = path_gradients(*run_formulation(w, cfg, torch.float32, fixed), ups, paths)
    monkeypatch.setattr(sh3, "C3", (*sh3.C3[:5], 1.25 * sh3.C3[5], sh3.C3[6]))
    got = path_gradients(*run_formulation(w, cfg, torch.float64, fixed), ups, paths)
    a, b, c = got["l_d"]["mean"], want["l_d"]["mean"], f32["l_d"]["mean"]
    live = row_norm(b) > 0
    change = (row_norm(a - b) / row_norm(b))[live]
    outside = ~(row_norm(a - b) <= RTOL * row_norm(b) + MARGIN * row_norm(c - b))
    summed = sum(want[path]["mean"] for path in ("variance_inverse", "opacity", "l_d", "mean"))
    old_bound = 5e-4 * float(summed.abs().max())
    print("rows", int(live.sum()), "outside the row rule", int(outside.sum()), "median row-relative change", float(change.median()),
          "| rows whose change exceeds the per-tensor bound", int(((a - b).abs().amax(dim=1) > old_bound).sum()), "bound", old_bound)
    assert int(outside.sum()) > 0.5 * int(live.sum())


def test_row_rule_resolves_a_compensation_a_tenth_of_a_percent_off(monkeypatch):
    """The resolution of the row rule on the rho chain.  The float64 formulation with rho (1 + 1e-3 rho) in the place of rho
    stands in for a kernel whose compensation is a tenth of a percent off on the larger splats, on the ordinary 1291 world:
    more than half of the live rows of opacity -> mean, -> variance_q and -> variance_scale fall outside the rule.  Printed
    beside each: how many rows the per-tensor bound of tests/test_antialias_gpu.py (5e-4 of the largest entry of the float64
    gradient with "opacity" alone upstream) would have noticed."""
    import tests.test_splat_gpu as splat

    cfg = CONFIGS["splat-all-antialias-deg3of16-world-depth"]
    w = world(SHAPES[1], 16)
    fixed = lists_of(own_lists_run(w, cfg)[1])
    ups = upstreams(w, cfg)
    want = path_gradients(*run_formulation(w, cfg, torch.float64, fixed), ups, ("opacity",))["opacity"]
    f32 = path_gradients(*run_formulation(w, cfg, torch.float32, fixed), ups, ("opacity",))["opacity"]
    exact = splat.compensation

    def off(cov0, cov_pix):
        rho, det0, det = exact(cov0, cov_pix)
        return rho * (1 + 1e-3 * rho), det0, det

    monkeypatch.setattr(splat, "compensation", off)
    got = path_gradients(*run_formulation(w, cfg, torch.float64, fixed), ups, ("opacity",))["opacity"]
    for k in ("mean", "variance_q", "variance_scale"):
        a, b, c = got[k], want[k], f32[k]
        live = row_norm(b) > 0
        outside = ~(row_norm(a - b) <= RTOL * row_norm(b) + MARGIN * row_norm(c - b))
        old_bound = 5e-4 * float(b.abs().max())
        print("opacity ->", k, "rows", int(live.sum()), "outside the row rule", int(outside.sum()), "median row-relative change",
              float((row_norm(a - b) / row_norm(b))[live].median()), "| rows whose change exceeds the per-tensor bound",
              int(((a - b).abs().amax(dim=1) > old_bound).sum()), "bound", old_bound)
        assert int(live.sum()) > 1000 and int(outside.sum()) > 0.5 * int(live.sum()), k


def test_position_worlds_keep_something_and_cull_something():
    """Every sub-world of the position test has a kept Gaussian (camera_inputs returns None for an empty list), the larger
    ones a culled one too, in both families."""
    for family in EDGE_CONFIGS:
        cfg = position_config(family, 16)
        with torch.no_grad():
            _, cams = run_formulation(sub_world(world(SHAPES[0], 16), 0, BIG, 16), cfg, torch.float32)
        kept = torch.zeros(BIG, dtype=torch.bool)
        kept[cams[0]["index"]] = True
        for n in SIZES:
            assert bool(kept[BIG - 1 - n:BIG - 1].any()), (family, n)
        assert bool(kept[BIG - 2]) and not bool(kept[BIG - 256:BIG - 1].all()), family


@pytest.mark.parametrize("family", EDGE_CONFIGS)
def test_covariance_clamp_row_is_clamped_and_finite_in_float32(family):
    """The condition on the covariance-clamp row: cov[3] of its pixel covariance exceeds FLT_MAX / 1000 (float64 on the same
    float32 parameters, and the float32 formulation's variance_inverse[3] sits at 1000 / FLT_MAX), cov[0] does not, and the
    float32 formulation's outputs and all five gradient rows of every path are finite; the clamped axis' log-scale gets an exact
    zero from the covariance path.  Two log scales further on (CLAMP_LOG_SCALE + 3.5) the formulation is no longer finite: the
    chosen value has room on both sides (38.5 is the first that reaches the clamp)."""
    cfg = EDGE_CONFIGS[family]
    w, row = edge_scene()
    i = row["covariance clamp"]
    lim = torch.finfo(torch.float32).max / 1000
    # the pixel covariance in float64, with the camera coordinates the float32 arithmetic has (t[0] an exact zero)
    P, K = w["P"][0], w["K"].double()
    m = w["mean"][i]
    t32 = torch.stack([((m[0] * P[r, 0] + m[1] * P[r, 1]) + m[2] * P[r, 2]) + P[r, 3] for r in range(3)])
    assert float(t32[0]) == 0.0 and float(t32[2]) > 1.0
    J = gft.pixel_jacobian_batch(K, t32.double()[None, None])[0, 0]
    W = P[:, :3].double()
    S = torch.diag(torch.exp(2 * w["variance_scale"][i].double()))  # q = (0, 0, 0, 1)
    assert w["variance_q"][i].tolist() == [0.0, 0.0, 0.0, 1.0]
    cov = J @ W @ S @ W.T @ J.T
    print("covariance clamp: float64 pixel covariance", cov.flatten().tolist(), "limit", lim)
    assert float(cov[1, 1]) > lim and 0.11 < float(cov[0, 0]) < 1000 and float(cov[0, 1].abs()) < 1000
    leaves, cams = own_lists_run(w, cfg)
    r = cams[0]["index"].tolist().index(i)
    vinv = cams[0]["variance_inverse"].detach().reshape(-1, 4)[r]
    assert float(vinv[3]) == pytest.approx(1 / lim, rel=1e-5) and float(vinv[0]) == pytest.approx(1 / float(cov[0, 0] + cfg[1].get("cov_dilation", 1e-6)), rel=1e-4)
    ups, paths = upstreams(w, cfg), paths_of(cfg)
    grads = path_gradients(leaves, cams, ups, paths)
    for path in paths:
        assert torch.isfinite(cams[0][path][r]).all(), path
        for k in NAMES:
            assert torch.isfinite(grads[path][k][i]).all(), (path, k)
        assert float(grads[path]["variance_scale"][i][1]) == 0.0, path
    assert float(grads["variance_inverse"]["variance_scale"][i].abs().max()) > 0
    # the room above
    far = {k: v.clone() if k in NAMES else v for k, v in w.items()}
    far["variance_scale"][i, 1] = CLAMP_LOG_SCALE + 3.5
    l2, c2 = run_formulation(far, cfg, torch.float32, lists_of(cams))
    g2 = path_gradients(l2, c2, ups, ("variance_inverse",))
    assert not all(torch.isfinite(g2["variance_inverse"][k][i]).all() for k in NAMES)
