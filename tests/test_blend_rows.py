"""What tests/test_blend_rows_gpu.py rests on, checked where no GPU is needed.

1. The closed form of tests/blend_rows_torch.py is the autograd oracles' (`dense_render_depth`, `dense_render_distortion`): every
   kind of scene of the GPU file at <= 60 layers, every leaf, to 1e-10 of every row's condition scale.
2. The guard of the row rule.  The rule allows 4 |f32 - want| beside 2e-5 of the row's scale, f32 being the closed form run in
   float32; so that this measured term cannot hide a failure, the float32 formulation ALONE stays within 2e-5 of the scale on
   every row and every map pixel of every case of the GPU file, with no allowance.  A scene that cannot is reshaped: the
   underflow stack has 200 layers (at 300 rows behind the underflow miss it), the sub-pixel scene keeps 1e-6 of every Gaussian
   at the corners of its box (pixels that only tails of 1e-30 reach have dist = 1e-62).  Each case prints the figures per leaf.
3. The scenes are what they are named for: T_N in [1e-36, 1e-30] and non-zero in float32; T_N == 0 in float32 at a third of the
   pixels or more while float64 T_N is not; an exact zero over half the rows; semi-occluded stacks."""
import pytest
import torch

from tests.blend_rows_torch import FLT_MIN, blend_rows
from tests.distortion_torch import dense_render_distortion, dense_weights, distortion_pairs
from tests.test_blend_rows_gpu import BG, CASES, DEPTH_SETS, RTOL, STACK_SIZES, closed_forms, depths, row_norm, scene, stack_opacity, upstream
from tests.test_render_depth_gpu import dense_render_depth

SMALL = ["stack_31", "stack_32", "stack_33", "deep_300", "deep_700", "underflow_200", "tiny_tn", "opaque_layer", "frame17", "subpixel"]
SMALL_CASES = [(s, d) for s in SMALL for d in (DEPTH_SETS if s in ("stack_33", "subpixel") else ("spread", "z100_1e-2"))]


def truncated(name, n=60):
    """the first `n` layers of a scene (the opaque layer of opaque_layer is its 21st)"""
    sc = scene(name)
    full = sc["start"].shape[0]
    return {k: (v[:n] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == full and k != "wimg" else v) for k, v in sc.items()}


def autograd_rows(sc, z, ups):
    gI, gD, gA, G = (t.double() for t in ups)
    with_mean = sc["mean"].is_floating_point()

    def leaves():
        ls = {"vinv": sc["vinv"], "opacity": sc["opacity"], "l_d": sc["l_d"], "z": z, "bg": BG}
        if with_mean:
            ls["mean"] = sc["mean"]
        return {k: v.detach().double().clone().requires_grad_(True) for k, v in ls.items()}

    lv = leaves()
    img, dep, alp = dense_render_depth(sc["start"], sc["end"], lv.get("mean", sc["mean"]), lv["vinv"], lv["opacity"], lv["l_d"], lv["z"],
                                       sc["width"], sc["height"], lv["bg"])
    ((img * gI).sum() + (dep * gD).sum() + (alp * gA).sum()).backward()
    render = {k: v.grad for k, v in lv.items()}
    lv2 = leaves()
    out = dense_render_distortion(sc["start"], sc["end"], lv2.get("mean", sc["mean"]), lv2["vinv"], lv2["opacity"], lv2["l_d"], lv2["z"],
                                  sc["width"], sc["height"], lv2["bg"])
    (out[3] * G).sum().backward()
    dist = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in lv2.items() if k in ("mean", "vinv", "opacity", "z")}
    maps = {"image": img.detach(), "depth": dep.detach(), "alpha": alp.detach(), "dist": out[3].detach()}
    return render, dist, maps


@pytest.mark.parametrize("name,kind", SMALL_CASES, ids=[f"{s}-{d}" for s, d in SMALL_CASES])
def test_closed_form_is_the_autograd_oracles(name, kind):
    sc = truncated(name)
    n = sc["start"].shape[0]
    assert n <= 60
    z = depths(kind, n)
    ups = upstream(sc)
    want_r, want_d, want_m = autograd_rows(sc, z, ups)
    got_r, got_d, got_m = blend_rows(sc, z, BG, *ups)
    for k in ("image", "alpha"):  # sums of products in [0, 1] (the image's colours and background below 1.1)
        assert float((got_m[k] - want_m[k]).abs().max()) <= 1e-10, k
    # per pixel, relative to the pixel's own scale.  The recurrence oracle forms dist as 2 sum w_k (z_k A - B): its own float64
    # round-off is that of the numbers it subtracts, <= 2 eps sum w z per step, which at two layers 4e-6 apart at depth 50
    # exceeds 1e-10 of the pixel — so it gets that term, and the O(n^2) definition on the oracle's weights is held to the plain bound
    pairs = distortion_pairs(dense_weights(sc["start"], sc["end"], sc["mean"], sc["vinv"].double(), sc["opacity"].double(), sc["width"],
                                           sc["height"])[0], z.double())
    eps = torch.finfo(torch.float64).eps
    for k, want, own in (("depth", want_m["depth"], 0.0), ("dist", want_m["dist"], 64 * eps), ("dist", pairs, 0.0)):
        err = (got_m[k] - want).abs()
        assert bool((err <= 1e-10 * got_m[k + "_scale"] + own * got_m["depth_scale"]).all()), (k, own, float((err / got_m[k + "_scale"].clamp(min=1e-300)).max()))
    seen = 0
    for what, got, want in (("render", got_r, want_r), ("distortion", got_d, want_d)):
        for leaf, w in want.items():
            value, scale = got[leaf]
            if leaf == "bg":
                value, scale, w = value[None], scale[None], w[None]
            err, s = row_norm(value - w.reshape(value.shape)), row_norm(scale)
            assert bool((err <= 1e-10 * s).all()), (what, leaf, float((err / s.clamp(min=1e-300)).max()), int((err > 1e-10 * s).nonzero()[0]))
            assert bool((row_norm(w.reshape(value.shape)) <= s * (1 + 1e-12)).all()), (what, leaf)  # a scale bounds its value
            seen += int((s > 0).sum())
    assert seen > 0
    if name == "opaque_layer":  # the opaque layer is dropped wherever its box reaches: an exactly dead row
        for rows in (got_r, got_d):
            assert float(rows["opacity"][0][20].abs().max()) == 0.0 and float(rows["opacity"][1][20].abs().max()) == 0.0


@pytest.mark.parametrize("name,kind", CASES, ids=[f"{s}-{d}" for s, d in CASES])
def test_float32_formulation_alone_stays_within_the_rule(name, kind):
    (want_r, want_d, want_m), (f32_r, f32_d, f32_m) = closed_forms(name, kind)
    failures = []

    def guard(tag, want, scale, f32):
        if want.dim() == 1 and tag.endswith(" bg"):
            want, scale, f32 = (t[None] for t in (want, scale, f32))
        err, s = row_norm(f32 - want), row_norm(scale)
        live = s > 0
        rel = err[live] / s[live]
        print(f"ROWS {name} {kind} {tag}: live {int(live.sum())}/{s.numel()} formulation err/scale median {float(rel.median()) if rel.numel() else 0:.2e} "
              f"max {float(rel.max()) if rel.numel() else 0:.2e}")
        bad = err > RTOL * s
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            failures.append(f"{tag}: {int(bad.sum())} rows; first {i}: err {float(err[i]):.3e} scale {float(s[i]):.3e}")
        assert bool(((s == 0) <= (row_norm(f32) == 0)).all()), tag  # a dead row is an exact zero in float32 too

    for what, want, f32 in (("render", want_r, f32_r), ("distortion", want_d, f32_d)):
        for leaf in want:
            guard(f"{what} {leaf}", *want[leaf], f32[leaf][0])
    for k in ("depth", "dist"):  # per pixel
        guard(f"map {k}", want_m[k].reshape(-1), want_m[k + "_scale"].reshape(-1), f32_m[k].reshape(-1))
    assert float((f32_m["image"] - want_m["image"]).abs().max()) <= 1e-5 and float((f32_m["alpha"] - want_m["alpha"]).abs().max()) <= 1e-5
    assert not failures, "\n".join(failures)


def test_scenes_are_what_they_are_named_for():
    ups = lambda sc: upstream(sc)  # noqa: E731
    sc = scene("tiny_tn")
    z = depths("spread", sc["start"].shape[0])
    T64 = blend_rows(sc, z, BG, *ups(sc))[2]["T_N"]
    T32 = blend_rows(sc, z, BG, *ups(sc), dtype=torch.float32)[2]["T_N"]
    edge = (T64 > 1e-36) & (T64 < 1e-30)
    print("tiny_tn: T_N min", float(T64.min()), "max", float(T64.max()), "pixels in (1e-36, 1e-30):", int(edge.sum()))
    assert int(edge.sum()) >= 16 and bool((T32[edge] != 0).all()) and float(T64.min()) > 4 * FLT_MIN
    sc = scene("underflow_200")
    T64 = blend_rows(sc, depths("spread", 200), BG, *ups(sc))[2]["T_N"]
    T32 = blend_rows(sc, depths("spread", 200), BG, *ups(sc), dtype=torch.float32)[2]["T_N"]
    print("underflow_200: float32 T_N == 0 at", float((T32 == 0).double().mean()), "of the pixels; float64 T_N", float(T64.min()), "...", float(T64.max()))
    assert float((T32 == 0).double().mean()) > 0.33 and float(T64.min()) > 0 and float(T64.max()) < 1e-20
    sc = scene("opaque_layer")
    m = blend_rows(sc, depths("spread", sc["start"].shape[0]), BG, *ups(sc))[2]
    assert float(m["T_N"][:16].abs().max()) == 0.0 and float(m["T_N"][16:].min()) > 0
    for n in STACK_SIZES:
        sc = scene(f"stack_{n}")
        T = blend_rows(sc, depths("spread", n), BG, *ups(sc))[2]["T_N"]
        assert 1e-6 < float(T.median()) < 0.3, (n, stack_opacity(n), float(T.median()))
    sc = scene("frame17")
    assert (sc["width"], sc["height"]) == (16, 16) and bool((sc["end"] == 16).all())
