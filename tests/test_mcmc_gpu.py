"""MCMC density control (csrc/gcp_mcmc.hip, density.mcmc_rows / mcmc_noise, GS_model_with_param.relocate_and_grow_device /
add_position_noise) on the GPU, against the torch / numpy formulation of tests/mcmc_torch.py: the weights to +-1 and their
prefix sum exactly, the draw bit for bit, the relocated values and the noise against float64, Adam's state across the pass,
no device->host read, and the training loop."""
import math

import numpy as np
import pytest
import torch

from simplegaussiansplat_tk71_amd import density
from simplegaussiansplat_tk71_amd import gs_model as gm
from tests import density_torch as dt
from tests import mcmc_torch as mt

pytestmark = pytest.mark.gpu

# both sides of a 256-thread block and of the prefix sum's 2048-element chunk; (1, 80) draws the one source 79 times
SIZES = [(1, 1), (1, 80), (255, 255), (257, 300), (2049, 2151), (5000, 5250)]
SEEDS = (5, 2 ** 40 + 17)
_passes = {}


def run_pass(n, m, seed, device):
    """The scene of n Gaussians, what density.mcmc_rows made of it (on the CPU) and the formulation's draw from the DEVICE's
    cum; computed once per (n, m, seed) and shared, never changed."""
    key = (n, m, seed)
    if key not in _passes:
        sc = mt.scene(n)
        g = torch.Generator().manual_seed(n)
        moments = {k: (torch.randn(sc[k].shape, generator=g), torch.rand(sc[k].shape, generator=g)) for k in mt.NAMES}
        new, new_moments, info = density.mcmc_rows({k: sc[k].to(device) for k in mt.NAMES},
                                                   {k: tuple(t.to(device) for t in pair) for k, pair in moments.items()}, m, mt.MIN_OPACITY, seed)
        info = {k: v.cpu() for k, v in info.items()}
        _passes[key] = {"scene": sc, "moments": moments, "new": {k: v.cpu() for k, v in new.items()},
                        "new_moments": {k: tuple(t.cpu() for t in pair) for k, pair in new_moments.items()}, "info": info,
                        "want": mt.draw(info["cum"].numpy(), m, seed)}
    return _passes[key]


def make_model(sc, device, **kw):
    model = gm.GS_model_with_param(*(sc[k].clone().to(device) for k in mt.NAMES[:4]), L_max=math.isqrt(sc["color"].shape[1]) - 1,
                                   prunning_min_opacity=mt.MIN_OPACITY, **kw)
    with torch.no_grad():
        model.color.copy_(sc["color"].to(device))
    return model


def _state(model):
    return {k: {s: (v.clone() if torch.is_tensor(v) else v) for s, v in model._optimizer.state[p].items()} for k, p in model.named_parameters()}


def _five_steps(model, seed=0):
    g = torch.Generator().manual_seed(seed)
    grads = {k: torch.randn(p.shape, generator=g).to(p.device) for k, p in model.named_parameters()}
    for _ in range(5):
        for k, p in model.named_parameters():
            p.grad = grads[k].clone()
        model.train_step()


# ---- weights ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", SIZES)
def test_weights_and_their_prefix_sum(n, m, device):
    """Zero exactly on the dead rows; elsewhere within 1 of the formulation (the device's float32 expf may differ from torch's by
    an ulp at a floor boundary); cum is the exact cumulative sum of the device's own weights."""
    p = run_pass(n, m, SEEDS[0], device)
    got, cum = p["info"]["weight"].long(), p["info"]["cum"].long()
    want, dead = mt.weights(p["scene"]["opacity"])
    assert mt.weight_levels(n) == 1 << 16 and density.mcmc_weight_levels(n) == 1 << 16
    assert density.mcmc_weight_levels(32768) == 1 << 15 and density.mcmc_weight_levels(10 ** 6) == 1 << 11
    assert not got[dead].any() and bool((got[~dead] >= 1).all())
    assert int((got - want).abs().max()) <= 1
    assert int(cum[0]) == 0 and torch.equal(cum[1:], got.cumsum(0))
    if n >= 255:
        assert 0.1 * n <= int(dead.sum()) <= 0.3 * n


# ---- draw ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m", SIZES)
def test_draw_equals_the_formulation(n, m, seed, device):
    p = run_pass(n, m, seed, device)
    info, want = p["info"], p["want"]
    for k in ("src_row", "times", "kind"):
        assert torch.equal(info[k], want[k]), k
    dead, slot = info["weight"] == 0, want["slot"]
    assert int(slot.sum()) == int(dead.sum()) + m - n
    assert not dead[info["src_row"][slot].long()].any()          # no dead row is ever a source
    assert int(info["times"].sum()) == int(slot.sum())
    assert torch.equal(info["src_row"][~slot], torch.arange(m, dtype=torch.int32)[~slot])
    print(f"({n}, {m}) seed {seed}: {int(slot.sum())} slots, times up to {int(info['times'].max())}")
    # the same seed twice: bit-identical; another seed: another draw (where there is more than one source to choose from)
    sc = {k: p["scene"][k].to(device) for k in mt.NAMES}
    again = density.mcmc_rows(sc, {}, m, mt.MIN_OPACITY, seed)[2]
    other = density.mcmc_rows(sc, {}, m, mt.MIN_OPACITY, seed + 1)[2]
    for k in ("src_row", "times", "kind", "cum"):
        assert torch.equal(again[k].cpu(), info[k]), k
    assert torch.equal(other["cum"].cpu(), info["cum"])
    if n >= 255:
        assert not torch.equal(other["src_row"].cpu(), info["src_row"])


# ---- values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m", SIZES)
def test_relocated_values_equal_the_float64_formulation(n, m, seed, device):
    """Opacity and log scale of every touched row (its source was drawn at least once) within the project's absolute 1e-5 of
    float64 (the bound of test_split_children_equal_the_float64_formulation: logits <= 16, log scales of O(1)); every other
    row, and mean / variance_q / color of every row, bit-equal to the plain gather."""
    p = run_pass(n, m, seed, device)
    sc, new, info = p["scene"], p["new"], p["info"]
    src, times = info["src_row"].long(), info["times"].long()
    touched = times[src] > 0
    for k in ("mean", "variance_q", "color"):
        assert torch.equal(new[k], sc[k][src]), k
    for k in ("opacity", "variance_scale"):
        assert torch.equal(new[k][~touched], sc[k][src][~touched]), k
    sources = torch.nonzero(times > 0).reshape(-1)
    if (n, m) == (1, 80):
        assert int(times[0]) == 79 and bool(touched.all())   # n = min(79 + 1, 51): the cap
    elif n > 1:
        assert sources.numel() >= 8
    if not sources.numel():
        return
    want_op, want_scale = mt.relocated(sc["opacity"][sources], sc["variance_scale"][sources], times[sources])
    place = torch.zeros(n, dtype=torch.long)
    place[sources] = torch.arange(sources.numel())
    rows = place[src[touched]]
    err_op = (new["opacity"][touched].double() - want_op[rows]).abs().max().item()
    err_scale = (new["variance_scale"][touched].double() - want_scale[rows]).abs().max().item()
    print(f"({n}, {m}) seed {seed}: {int(touched.sum())} touched rows, max |logit error| {err_op:.3g}, max |log scale error| {err_scale:.3g}")
    assert err_op <= 1e-5 and err_scale <= 1e-5
    assert bool(torch.isfinite(new["opacity"]).all()) and bool(torch.isfinite(new["variance_scale"]).all())
    # drawn once (n = 2): the closed form D = 2 o' - o'^2 / sqrt(2)
    once = touched & (times[src] == 1)
    if once.any():
        o = torch.sigmoid(sc["opacity"][src][once].double()).reshape(-1)
        o_new = 1 - torch.sqrt(1 - o)
        shift = torch.log(o / (2 * o_new - o_new ** 2 / math.sqrt(2)))
        got_shift = new["variance_scale"][once].double() - sc["variance_scale"][src][once].double()
        assert (got_shift - shift[:, None]).abs().max().item() <= 1e-5
        assert (torch.sigmoid(new["opacity"][once].double()).reshape(-1) - o_new).abs().max().item() <= 1e-5


# ---- edges --------------------------------------------------------------------------------------------------------------
def test_nothing_dead_and_no_growth_is_the_identity(device):
    sc = mt.scene(2049, dead_share=0.0)
    info = density.mcmc_rows({k: sc[k].to(device) for k in mt.NAMES}, {}, 2049, mt.MIN_OPACITY, 1)[2]
    assert not info["kind"].any() and not info["times"].any()
    assert torch.equal(info["src_row"].cpu(), torch.arange(2049, dtype=torch.int32))
    model = make_model(sc, device)
    _five_steps(model)
    before, state = {k: p.detach().clone() for k, p in model.named_parameters()}, _state(model)
    assert model.relocate_and_grow_device(seed=1) == (2049, 2049)
    for k, p in model.named_parameters():
        assert torch.equal(p.detach(), before[k]), k
        st = model._optimizer.state[p]
        assert st["step"] == state[k]["step"] == 5
        assert torch.equal(st["exp_avg"], state[k]["exp_avg"]) and torch.equal(st["exp_avg_sq"], state[k]["exp_avg_sq"]), k


def test_everything_dead_returns_copies(device):
    sc = mt.scene(300)
    sc["opacity"][:] = -10.0
    new, _, info = density.mcmc_rows({k: sc[k].to(device) for k in mt.NAMES}, {}, 315, mt.MIN_OPACITY, 3)
    assert int(info["cum"][-1]) == 0 and not info["times"].any()
    assert torch.equal(info["src_row"].cpu(), (torch.arange(315) % 300).to(torch.int32))
    assert torch.equal(info["kind"].cpu(), (torch.arange(315) >= 300).to(torch.uint8))
    for k in mt.NAMES:
        assert torch.equal(new[k].cpu(), sc[k][torch.arange(315) % 300]), k
    model = make_model(sc, device)
    assert model.relocate_and_grow_device(seed=3, cap_max=400) == (300, 315)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_cap_max_bounds_the_growth(device):
    sc = mt.scene(300)
    for cap, want in ((None, 300), (100, 300), (300, 300), (307, 307), (315, 315), (316, 315), (10 ** 6, 315)):
        model = make_model(sc, device)
        assert model.relocate_and_grow_device(seed=2, cap_max=cap) == (300, want), cap
        for t in (*model.parameters(), model.mean_grads_norm, model.mean_grads_iter, model.screen_grads_norm, model.screen_grads_views):
            assert t.shape[0] == want
    with pytest.raises(RuntimeError, match="GPU"):
        density.mcmc_rows({k: sc[k] for k in mt.NAMES}, {}, 300, mt.MIN_OPACITY, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        density.mcmc_noise(sc["mean"], sc["variance_q"], sc["variance_scale"], sc["opacity"], 1.0, 0)


def test_antialias_does_not_change_what_is_dead(device):
    """The pass tests the raw sigmoid(opacity), also under antialias=True."""
    sc = mt.scene(2049)
    out = []
    for kw in ({}, {"centres": "subpixel", "cov_dilation": 0.3, "antialias": True}):
        model = make_model(sc, device, **kw)
        assert model.relocate_and_grow_device(seed=7, cap_max=2151) == (2049, 2151)
        out.append({k: p.detach().clone() for k, p in model.named_parameters()})
    for k in mt.NAMES:
        assert torch.equal(out[0][k], out[1][k]), k


# ---- Adam across the pass -----------------------------------------------------------------------------------------------
def test_adam_state_survives_the_pass(device):
    """Survivors keep both moments bit for bit, sources and fresh rows start at 0.0, every `step` is kept, and the next HipAdam
    step is torch.optim.Adam's from the transplanted state (the bound of test_hip_adam_equals_torch_adam: 1e-6 of the largest
    magnitude in each tensor)."""
    n, m, seed = 2049, 2151, 4
    sc = mt.scene(n)
    model = make_model(sc, device)
    _five_steps(model)
    state = _state(model)
    params = {k: p.detach().clone() for k, p in model.named_parameters()}
    lrs = {k: group["lr"] for group, (k, _) in zip(model._optimizer.param_groups, model.named_parameters())}
    info = {k: v.cpu() for k, v in density.mcmc_rows(params, {}, m, mt.MIN_OPACITY, seed)[2].items()}
    want = mt.draw(info["cum"].numpy(), m, seed)
    assert torch.equal(info["src_row"], want["src_row"]) and torch.equal(info["kind"], want["kind"])
    assert model.relocate_and_grow_device(seed=seed, cap_max=m) == (n, m)
    survivor, src = (want["kind"] == 0).to(device), want["src_row"].long().to(device)
    drawn_from = (want["times"] > 0).to(device)
    assert 8 <= int(drawn_from.sum()) and 8 <= int(survivor.sum()) < n
    for k, p in model.named_parameters():
        st = model._optimizer.state[p]
        assert st["step"] == 5, k
        for moment in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[moment][survivor], state[k][moment][src[survivor]]), (k, moment)
            assert not st[moment][~survivor].any(), (k, moment)
            assert not st[moment][:n][drawn_from].any(), (k, moment)  # the sources start again too
            assert torch.equal(st[moment].cpu(), mt.gather(want, state[k][moment].cpu(), moments=True)), (k, moment)
    for stat in (model.mean_grads_norm, model.mean_grads_iter, model.screen_grads_norm, model.screen_grads_views):
        assert stat.shape == (m,) and not stat.any()
    theirs = {k: p.detach().clone().requires_grad_(True) for k, p in model.named_parameters()}
    adam = torch.optim.Adam([{"params": [theirs[k]], "lr": lrs[k]} for k in mt.NAMES])
    g = torch.Generator().manual_seed(1)
    for k, p in model.named_parameters():
        adam.state[theirs[k]] = {"step": torch.tensor(5.0), "exp_avg": mt.gather(want, state[k]["exp_avg"].cpu(), moments=True).to(device),
                                 "exp_avg_sq": mt.gather(want, state[k]["exp_avg_sq"].cpu(), moments=True).to(device)}
        grad = torch.randn(p.shape, generator=g).to(device)
        p.grad, theirs[k].grad = grad.clone(), grad.clone()
    model.train_step()
    adam.step()
    for k, p in model.named_parameters():
        st = model._optimizer.state[p]
        assert st["step"] == 6
        for got, ref in ((p.detach(), theirs[k].detach()), (st["exp_avg"], adam.state[theirs[k]]["exp_avg"]),
                         (st["exp_avg_sq"], adam.state[theirs[k]]["exp_avg_sq"])):
            assert (got - ref).abs().max().item() <= 1e-6 * max(ref.abs().max().item(), 1e-30), k


# ---- no host read -------------------------------------------------------------------------------------------------------
def test_the_pass_and_the_noise_read_nothing_back(device):
    """Under torch's sync debug mode "error" every synchronising call of torch raises: the pass and the noise complete, a
    plain .item() does not (which shows the mode is armed).  The C entry points themselves contain no stream synchronise
    (csrc/gcp_mcmc.hip: launches and one hipMemsetAsync)."""
    model = make_model(mt.scene(2049), device)
    _five_steps(model)
    probe = torch.ones(1, device=device)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        sizes = model.relocate_and_grow_device(seed=3, cap_max=2100)
        model.add_position_noise(seed=3)
        with pytest.raises(RuntimeError):
            probe.item()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert sizes == (2049, 2100) and model.mean.shape[0] == 2100
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


# ---- noise --------------------------------------------------------------------------------------------------------------
def noise_scene(n):
    """Scales in [0.05, 0.3], random quaternions and one zero quaternion; half of the opacities in [0.001, 0.021] around
    o0 = 0.005 (gate 0.2 .. 0.6), a quarter in [0.05, 0.45] (gate e^-4.5 .. e^-44.5), a quarter in [0.8, 0.99]."""
    g = torch.Generator().manual_seed(n)
    u, v = torch.rand(n, 1, generator=g), torch.rand(n, 1, generator=g)
    u[0] = 0.0  # a scene of one moves
    o = torch.where(u < 0.5, 0.001 + 0.02 * v, torch.where(u < 0.75, 0.05 + 0.4 * v, 0.8 + 0.19 * v))
    q = torch.randn(n, 4, generator=g)
    q[n // 2] = 0.0
    return {"variance_q": q, "variance_scale": torch.log(0.05 + 0.25 * torch.rand(n, 3, generator=g)), "opacity": torch.logit(o)}


def device_noise(sc, mean, amount, seed, device, **kw):
    out = mean.clone().to(device)
    density.mcmc_noise(out, *(sc[k].to(device) for k in ("variance_q", "variance_scale", "opacity")), amount, seed, **kw)
    return out.cpu()


@pytest.mark.parametrize("n", [1, 257, 4097])
def test_noise_equals_the_float64_formulation(n, device):
    """The displacement within absolute 1e-5 of float64 from the numpy Philox draws.  Rows with sigmoid(opacity) >= 0.5 move by
    less than 1e-30: the gate e^(-100 (o - 0.005)) is e^-49.5 = 3e-22 at o = 0.5 itself, which bounds the move by 1e-21 only, so
    this scene's opaque rows sit at o >= 0.8 — gate <= e^-79.5 = 3e-35, times s^2 <= 0.09 and |z| <= 9.6 (the largest
    Box-Muller radius, sqrt(4 ln 2^33), on two axes) — and the rows in between are held to the formulation like the rest.  With a
    non-zero mean the result is float32(mean + displacement) to 1 ulp."""
    sc = noise_scene(n)
    for seed in SEEDS:
        got = device_noise(sc, torch.zeros(n, 3), 1.0, seed, device)
        want = mt.noise(sc["variance_q"], sc["variance_scale"], sc["opacity"], 1.0, seed)
        err = (got.double() - want).abs().max().item()
        opaque = torch.sigmoid(sc["opacity"]).reshape(-1) >= 0.5
        moved = got[opaque].abs().max().item() if opaque.any() else 0.0
        print(f"n {n} seed {seed}: max |error| {err:.3g}, largest move {want.abs().max().item():.3g}, largest opaque move {moved:.3g}")
        assert err <= 1e-5
        assert not opaque[0] and bool((got[~opaque].abs().max(dim=1).values > 0).all())  # every other row does move
        assert moved < 1e-30
        assert torch.equal(device_noise(sc, torch.zeros(n, 3), 1.0, seed, device), got)  # the seed alone decides
        mean = torch.randn(n, 3, generator=torch.Generator().manual_seed(1))
        with_mean = device_noise(sc, mean, 1.0, seed, device)
        exact = mean + got
        assert bool(((with_mean - exact).abs() <= 2.0 ** -23 * exact.abs()).all())
    if n > 1:
        assert not torch.equal(got, device_noise(sc, torch.zeros(n, 3), 1.0, SEEDS[0], device))


def test_noise_and_split_draw_from_distinct_counters(device):
    """k = 0 makes the gate 1/2, identity rotations and unit scales make the displacement 2 * 1/2 * z = z: for equal
    (seed, index) it is the draw of counter (i, 0, 0, 1), and differs from child 0 of a split of Gaussian i, counter (i, 0, 0, 0)."""
    n, seed = 257, 5
    q = torch.zeros(n, 4)
    q[:, 3] = 1
    sc = {"variance_q": q, "variance_scale": torch.zeros(n, 3), "opacity": torch.zeros(n, 1)}
    z = device_noise(sc, torch.zeros(n, 3), 2.0, seed, device, k=0.0).double()
    ours = torch.from_numpy(mt.normals(seed, np.arange(n)))
    split = torch.from_numpy(dt.split_normals(seed, np.arange(n), np.zeros(n, dtype=np.int64)))
    assert (z - ours).abs().max().item() <= 1e-5
    assert bool(((z - split).abs().max(dim=1).values > 1e-3).all())


# ---- the loop -----------------------------------------------------------------------------------------------------------
def test_training_loop_with_the_mcmc_strategy(device, monkeypatch):
    from examples.train_cameras import synthetic_scene, train

    sizes, noises = [], []
    relocate, noise = gm.GS_model_with_param.relocate_and_grow_device, gm.GS_model_with_param.add_position_noise

    def spy_relocate(self, *a, **kw):
        sizes.append(relocate(self, *a, **kw))
        return sizes[-1]

    def spy_noise(self, *a, **kw):
        noises.append(self.mean.shape[0])
        return noise(self, *a, **kw)

    monkeypatch.setattr(gm.GS_model_with_param, "relocate_and_grow_device", spy_relocate)
    monkeypatch.setattr(gm.GS_model_with_param, "add_position_noise", spy_noise)
    start, P, K, wh, targets = synthetic_scene(600, 6, 64, 48, 0, device)
    runs = []
    for _ in range(2):
        sizes.clear()
        noises.clear()
        model, losses = train(start, P, K, wh, targets, iterations=150, densify="mcmc", densify_from_iter=30, densification_interval=30,
                              cap_max=700, log=lambda *_: None)
        first, last = np.mean(losses[:10]), np.mean(losses[-10:])
        print(f"loss {first:.5f} -> {last:.5f}, Gaussians {sizes}")
        assert len(losses) == 150 and all(math.isfinite(l) for l in losses)
        assert last < first
        assert sizes == [(600, 630), (630, 661), (661, 694), (694, 700), (700, 700)]
        assert len(noises) == 150 and max(noises) <= 700  # after every optimiser step
        assert model.mean.shape[0] == 700
        assert all(st["step"] == 150 for st in model._optimizer.state.values())  # Adam was never restarted
        runs.append(model.opacity.detach().clone())
    assert torch.equal(runs[0], runs[1])


@pytest.mark.parametrize("mode", ["reference", "device"])
def test_the_other_modes_never_call_the_mcmc_methods(mode, device, monkeypatch):
    from examples.train_cameras import synthetic_scene, train

    calls = []
    for name in ("relocate_and_grow_device", "add_position_noise"):
        monkeypatch.setattr(gm.GS_model_with_param, name, lambda self, *a, _name=name, **kw: calls.append(_name))
    monkeypatch.setattr(density, "mcmc_rows", lambda *a, **kw: calls.append("mcmc_rows"))
    monkeypatch.setattr(density, "mcmc_noise", lambda *a, **kw: calls.append("mcmc_noise"))
    start, P, K, wh, targets = synthetic_scene(600, 6, 64, 48, 0, device)
    _, losses = train(start, P, K, wh, targets, iterations=20, densify_from_iter=10, densification_interval=10, opacity_reset_interval=20,
                      densify=mode, log=lambda *_: None)
    assert len(losses) == 20 and calls == []
    with pytest.raises(ValueError, match="'reference', 'device' or 'mcmc'"):
        train(start, P, K, wh, targets, iterations=1, densify="other", log=lambda *_: None)
