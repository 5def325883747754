"""Developer benchmark of the MCMC density control (csrc/gcp_mcmc.hip): the position noise, the relocation pass and what the
strategy adds to a training step.

1. `k_mcmc_noise` at 10^6 Gaussians: back-to-back launches inside one pair of device events, against its 56 bytes per
   Gaussian (44 read, 12 written) and against the torch op-by-op formulation of the same statement (normals from
   torch.randn) on the same GPU.
2. `GS_model_with_param.relocate_and_grow_device` at 10^6 Gaussians, SH degrees 2 and 3, 5 % dead and 5 % growth, Adam state
   present (one step taken): a fresh model per timed call; against `densify_and_prune_device` on densify_bench's world of the
   same size and against a torch formulation that draws with torch.multinomial; the three alternate in one process; medians.
   Then the pass stage by stage on fixed buffers (weights + prefix sum, draw + kind, the 5 parameter gathers, values, the 10
   moment gathers), each repeated inside one pair of events.  The pass is 22 stream operations: 1 + 2 (prefix sum) + 1 memset
   + 2 + 5 + 1 + 10.
3. One training step of examples/train_cameras.py at its synthetic default size with densify="mcmc" and without (no pass in
   either run: the difference is the noise kernel plus the two regulariser terms), whole runs alternating; and the noise
   kernel and the regularisers' torch ops (forward and backward) alone at that size.
One JSON line per measurement.

    python tools/mcmc_bench.py [--gaussians 1000000] [--degrees 2 3] [--rounds 7] [--iterations 300]
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from densify_bench import EXTENT, HBM_PEAK, median, timed  # noqa: E402
from densify_bench import make_model as make_densify_model  # noqa: E402
from densify_bench import make_world as make_densify_world  # noqa: E402
from simplegaussiansplat_tk71_amd import _lib, density  # noqa: E402
from simplegaussiansplat_tk71_amd import gs_model as gm  # noqa: E402

NAMES = ("mean", "variance_q", "variance_scale", "opacity", "color")
MIN_OPACITY = 0.005


def make_world(n, degree, dev, dead_share=0.05, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    rand = lambda *s: torch.rand(*s, device=dev, generator=g)  # noqa: E731
    opacity = torch.logit(0.01 + 0.98 * rand(n, 1))
    opacity[rand(n) < dead_share] = -7.0
    world = {"mean": torch.randn(n, 3, device=dev, generator=g), "variance_q": torch.randn(n, 4, device=dev, generator=g),
             "variance_scale": torch.log(0.03 + 0.3 * rand(n, 3)), "opacity": opacity,
             "color": torch.randn(n, (degree + 1) ** 2, 3, device=dev, generator=g)}
    world["grads"] = {k: torch.randn(world[k].shape, device=dev, generator=g) for k in NAMES}
    return world


def make_model(world, degree):
    model = gm.GS_model_with_param(*(world[k].clone() for k in NAMES[:4]), L_max=degree, prunning_min_opacity=MIN_OPACITY)
    with torch.no_grad():
        model.color.copy_(world["color"])
    for k, p in model.named_parameters():
        p.grad = world["grads"][k].clone()
    model.train_step()  # Adam state present
    return model


def repeated(call, launches=50, warmup=3):
    for _ in range(warmup):
        call()
    return timed(lambda: [call() for _ in range(launches)])[0] / launches


# ---- 1. the noise ---------------------------------------------------------------------------------------------------------
def torch_noise(mean, q, log_scale, opacity, amount, k=100.0, o0=0.005):
    o = torch.sigmoid(opacity)
    gate = 1 / (1 + torch.exp(-k * (o0 - o)))
    rot = gm.qvec_to_rotmat_batch(q / q.norm(dim=1, keepdim=True).clamp_min(1e-8))
    s2 = torch.exp(log_scale) ** 2
    inner = s2 * torch.bmm(rot.transpose(1, 2), torch.randn_like(mean).unsqueeze(-1)).squeeze(-1)
    mean += amount * gate * torch.bmm(rot, inner.unsqueeze(-1)).squeeze(-1)


def noise(n, dev):
    world = make_world(n, 0, dev)
    args = tuple(world[k] for k in ("mean", "variance_q", "variance_scale", "opacity"))
    ms = repeated(lambda: density.mcmc_noise(*args, 1e-3, 7))
    ms_torch = repeated(lambda: torch_noise(*args, 1e-3), launches=20)
    moved = 56 * n
    return {"measurement": "k_mcmc_noise", "gaussians": n, "ms_per_launch": round(ms, 4), "bytes": moved, "tb_per_s": round(moved / ms / 1e9, 3),
            "share_of_hbm_peak": round(moved / (ms * 1e-3) / HBM_PEAK, 3), "torch_formulation_ms": round(ms_torch, 4),
            "torch_over_kernel": round(ms_torch / ms, 1),
            "note": "back-to-back launches on one 56 MB working set: it stays in the 256 MB Infinity Cache, a cold call is not faster"}


# ---- 2. the relocation pass -----------------------------------------------------------------------------------------------
@torch.no_grad()
def torch_relocate(model, m, min_opacity=MIN_OPACITY):
    """The same rule op by op: torch.multinomial over float opacities, the binomial double sum as masked tensor ops in float64,
    index gathers of the parameters and of Adam's moments.  It reads sizes back to the host, as such code does."""
    old = {k: getattr(model, k) for k in NAMES}
    n, dev = model.mean.shape[0], model.mean.device
    o = torch.sigmoid(model.opacity.data.reshape(-1).double())
    dead = ~(o > min_opacity)
    slots = torch.cat([torch.nonzero(dead).reshape(-1), torch.arange(n, m, device=dev)])
    drawn = torch.multinomial(torch.where(dead, 0.0, o).float(), slots.numel(), replacement=True)
    times = torch.bincount(drawn, minlength=n)
    src_row = torch.arange(m, device=dev)
    src_row[slots] = drawn
    copies = (times + 1).clamp(max=51)
    o_new = 1 - (1 - o) ** (1.0 / copies.double())
    denom = torch.zeros_like(o)
    for i in range(1, int(copies.max()) + 1):
        for k in range(i):
            denom += torch.where(copies >= i, math.comb(i - 1, k) * (-1) ** k * o_new ** (k + 1) / math.sqrt(k + 1), 0.0)
    touched = times > 0
    scale = torch.where(touched[:, None], model.variance_scale.data.double() + torch.log(o / denom)[:, None], model.variance_scale.data.double()).float()
    opacity = torch.where(touched, torch.logit(o_new.clamp(min_opacity, 1 - 2.0 ** -23)), model.opacity.data.reshape(-1).double()).float()[:, None]
    new = {k: (scale if k == "variance_scale" else opacity if k == "opacity" else old[k].data)[src_row] for k in NAMES}
    fresh = torch.ones(m, dtype=torch.bool, device=dev)
    fresh[:n] = touched | dead
    states = {k: model._optimizer.state.get(p) for k, p in old.items()}
    for k in NAMES:
        setattr(model, k, torch.nn.Parameter(new[k]))
    model.changing_optimizer()
    for k, st in states.items():
        if st:
            keep = (~fresh).reshape(-1, *([1] * (old[k].dim() - 1)))
            model._optimizer.state[getattr(model, k)] = {"step": st["step"], "exp_avg": st["exp_avg"][src_row] * keep,
                                                         "exp_avg_sq": st["exp_avg_sq"][src_row] * keep}
    model._zero_density_stats(m)
    return n, m


def stages(world, m, dev, launches=20):
    """The pass's own stages on fixed buffers: ms per stage."""
    lib, n = _lib.load(), world["mean"].shape[0]
    stream = torch.cuda.current_stream(dev).cuda_stream
    weight, times, src_row = (torch.empty(k, dtype=torch.int32, device=dev) for k in (n, n, m))
    cum, kind = torch.zeros(n + 1, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.gcp_mcmc_workspace_bytes(n), dtype=torch.uint8, device=dev)
    out = {k: torch.empty((m, *world[k].shape[1:]), device=dev) for k in NAMES}
    w_max = density.mcmc_weight_levels(n)

    def weights():
        _lib.check(lib.gcp_mcmc_weights(world["opacity"].data_ptr(), n, MIN_OPACITY, w_max, weight.data_ptr(), cum.data_ptr(), ws.data_ptr(),
                                        ws.numel(), stream), "gcp_mcmc_weights")

    def draw():
        _lib.check(lib.gcp_mcmc_draw(cum.data_ptr(), n, m, 7, 0, src_row.data_ptr(), times.data_ptr(), kind.data_ptr(), stream), "gcp_mcmc_draw")

    def gathers(mode, repeat):
        for _ in range(repeat):
            for k in NAMES:
                _lib.check(lib.gcp_densify_rows(world[k].data_ptr(), n, src_row.data_ptr(), kind.data_ptr(), m, world[k][0].numel(), mode,
                                                out[k].data_ptr(), stream), "gcp_densify_rows")

    def values():
        _lib.check(lib.gcp_mcmc_values(world["opacity"].data_ptr(), world["variance_scale"].data_ptr(), src_row.data_ptr(), times.data_ptr(), n, m,
                                       MIN_OPACITY, out["opacity"].data_ptr(), out["variance_scale"].data_ptr(), stream), "gcp_mcmc_values")

    res = {"weights_and_prefix_sum": repeated(weights, launches), "draw_and_kind": repeated(draw, launches),
           "parameter_gathers_5": repeated(lambda: gathers(0, 1), launches), "values": repeated(values, launches),
           "moment_gathers_10": repeated(lambda: gathers(1, 2), launches)}
    return {k: round(v, 4) for k, v in res.items()}, int((times > 0).sum()), int(times.max())


def relocation(n, degree, rounds, dev):
    world, dworld = make_world(n, degree, dev), make_densify_world(n, degree, dev)
    m = int(1.05 * n)
    t = {"relocate_and_grow_device": [], "densify_and_prune_device": [], "torch_formulation": []}
    for r in range(rounds + 2):  # two warm-up rounds
        model = make_model(world, degree)
        a = timed(lambda: model.relocate_and_grow_device(seed=r, cap_max=m))[0]
        model = make_densify_model(dworld, degree)
        b = timed(lambda: model.densify_and_prune_device(EXTENT, seed=r))[0]
        model = make_model(world, degree)
        torch.manual_seed(r)
        c = timed(lambda: torch_relocate(model, m))[0]
        if r >= 2:
            for k, v in zip(t, (a, b, c)):
                t[k].append(v)
    per_stage, n_sources, most = stages(world, m, dev)
    floats = 10 + 1 + 3 * (degree + 1) ** 2
    return {"measurement": "relocation pass", "gaussians": n, "sh_degree": degree, "floats_per_gaussian": floats, "rows_after": m,
            "dead": int((torch.sigmoid(world["opacity"]) <= MIN_OPACITY).sum()), "sources_drawn": n_sources, "most_draws_of_one_source": most,
            **{k + "_ms_median": round(median(v), 3) for k, v in t.items()}, **{k + "_ms_all": [round(x, 3) for x in sorted(v)] for k, v in t.items()},
            "stage_ms": per_stage, "stream_operations": 22}


# ---- 3. the training step -------------------------------------------------------------------------------------------------
def training_step(iterations, rounds, dev):
    from examples.train_cameras import synthetic_scene, train

    n = 3000
    start, P, K, wh, targets = synthetic_scene(n, 12, 160, 120, 0, dev)
    t = {"reference": [], "mcmc": []}
    for r in range(rounds + 1):  # one warm-up round
        for mode in t:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            train(start, P, K, wh, targets, iterations=iterations, densify_from_iter=10 ** 9, densify=mode, log=lambda *_: None)
            if r >= 1:
                t[mode].append((time.perf_counter() - t0) * 1e3 / iterations)
    world = make_world(n, 2, dev)
    args = tuple(world[k] for k in ("mean", "variance_q", "variance_scale", "opacity"))
    ms_noise = repeated(lambda: density.mcmc_noise(*args, 1e-3, 7), launches=200)
    opacity, scale = world["opacity"].clone().requires_grad_(True), world["variance_scale"].clone().requires_grad_(True)

    def regularisers():
        (0.01 * torch.sigmoid(opacity).mean() + 0.01 * torch.exp(scale).mean()).backward()

    ms_reg = repeated(regularisers, launches=200)
    return {"measurement": "training step", "gaussians": n, "cameras": 12, "image": [160, 120], "iterations": iterations,
            "step_ms_reference_median": round(median(t["reference"]), 3), "step_ms_mcmc_median": round(median(t["mcmc"]), 3),
            "step_ms_reference_all": [round(x, 3) for x in sorted(t["reference"])], "step_ms_mcmc_all": [round(x, 3) for x in sorted(t["mcmc"])],
            "noise_kernel_alone_ms": round(ms_noise, 4), "regularisers_forward_backward_alone_ms": round(ms_reg, 4),
            "note": "whole runs of train() including the model's set-up, host clock around a final synchronise; the loop reads the loss back every step"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--degrees", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=300)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mcmc_bench measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    print(json.dumps(noise(a.gaussians, dev)), flush=True)
    for degree in a.degrees:
        print(json.dumps(relocation(a.gaussians, degree, a.rounds, dev)), flush=True)
    print(json.dumps(training_step(a.iterations, 3, dev)), flush=True)
