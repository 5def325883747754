"""Developer benchmark of Mip-Splatting's 3-D smoothing filter (csrc/gcp_filter3d.hip): its three kernels and what the option
adds to a training step.

1. `k_filter3d_apply` and `k_filter3d_backward` at 10^6 Gaussians: back-to-back launches inside one pair of device events,
   against their 36 / 52 bytes per Gaussian and the 8.0 TB/s HBM peak — once on ONE working set (36 / 52 MB: it stays in the
   256 MB Infinity Cache) and once rotating over enough separate working sets to exceed twice that cache, so that every launch
   reads from and writes to HBM; and against the torch op-by-op formulation of the same statements (autograd for the backward)
   on the same GPU.
2. `k_filter3d_rate` at 10^6 Gaussians and 100 cameras, with `filter_from_rate` behind it: what `update_filter_3d` costs every
   ~100 iterations.
3. One training step of the model (forward of one 1920x1080 camera, fused L1 + D-SSIM loss, backward; no optimiser step) at
   10^6 Gaussians with filter_3d=True and without, the two alternating in one process; device events around each step, medians.
One JSON line per measurement.

    python tools/filter3d_bench.py [--gaussians 1000000] [--cameras 100] [--rounds 9]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from densify_bench import HBM_PEAK, median, timed  # noqa: E402
from simplegaussiansplat_tk71_amd import _lib, filter3d  # noqa: E402
from simplegaussiansplat_tk71_amd import gs_model as gm  # noqa: E402
from simplegaussiansplat_tk71_amd.synthetic import make_world, ring_cameras  # noqa: E402

INFINITY_CACHE = 256 << 20


def repeated(calls, launches=200, warmup=10):
    """ms per launch of `calls[i % len(calls)]`, back to back inside one pair of events."""
    for i in range(warmup):
        calls[i % len(calls)]()
    return timed(lambda: [calls[i % len(calls)]() for i in range(launches)])[0] / launches


def working_set(n, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    rand = lambda *s: torch.rand(*s, device=dev, generator=g)  # noqa: E731
    return {"v": torch.log(0.005 + 0.05 * rand(n, 3)), "x": torch.logit(0.05 + 0.9 * rand(n)), "phi": 0.002 + 0.03 * rand(n),
            "g_v": torch.randn(n, 3, device=dev, generator=g), "g_x": torch.randn(n, device=dev, generator=g),
            "v_out": torch.empty(n, 3, device=dev), "x_out": torch.empty(n, device=dev), "gv_out": torch.empty(n, 3, device=dev),
            "gx_out": torch.empty(n, device=dev)}


def torch_apply(v, x, phi):
    half_l = 0.5 * torch.log1p((phi * phi)[:, None] * torch.exp(-2.0 * v))
    log_c = -half_l.sum(dim=1)
    return v + half_l, x + log_c - torch.log1p(torch.exp(x) * -torch.expm1(log_c))


def apply_kernels(n, dev):
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    sets = [working_set(n, dev, s) for s in range(max(2, -(-2 * INFINITY_CACHE // (36 * n))))]

    def forward(w):
        return lambda: _lib.check(lib.gcp_filter3d_apply(w["v"].data_ptr(), w["x"].data_ptr(), w["phi"].data_ptr(), n, w["v_out"].data_ptr(),
                                                         w["x_out"].data_ptr(), stream), "gcp_filter3d_apply")

    def backward(w):
        return lambda: _lib.check(lib.gcp_filter3d_apply_backward(w["v"].data_ptr(), w["x"].data_ptr(), w["phi"].data_ptr(), w["g_v"].data_ptr(),
                                                                  w["g_x"].data_ptr(), n, w["gv_out"].data_ptr(), w["gx_out"].data_ptr(), stream),
                                  "gcp_filter3d_apply_backward")

    w = sets[0]
    v, x = w["v"].clone().requires_grad_(True), w["x"].clone().requires_grad_(True)

    def torch_backward():
        v_out, x_out = torch_apply(v, x, w["phi"])
        torch.autograd.grad((v_out * w["g_v"]).sum() + (x_out * w["g_x"]).sum(), (v, x))

    with torch.no_grad():
        ms_torch_fwd = repeated([lambda: torch_apply(w["v"], w["x"], w["phi"])], launches=20, warmup=3)
    ms_torch_both = repeated([torch_backward], launches=20, warmup=3)
    for name, make, per_row in (("k_filter3d_apply", forward, 36), ("k_filter3d_backward", backward, 52)):
        warm, rotating = repeated([make(sets[0])]), repeated([make(s) for s in sets])
        moved = per_row * n
        yield {"measurement": name, "gaussians": n, "bytes": moved, "ms_per_launch_one_working_set": round(warm, 5),
               "ms_per_launch_rotating": round(rotating, 5), "working_sets": len(sets), "rotating_footprint_mb": round(len(sets) * 88 * n / 2 ** 20),
               "tb_per_s_one_working_set": round(moved / warm / 1e9, 3), "tb_per_s_rotating": round(moved / rotating / 1e9, 3),
               "share_of_hbm_peak_rotating": round(moved / (rotating * 1e-3) / HBM_PEAK, 3),
               "torch_formulation_ms": round(ms_torch_fwd if per_row == 36 else ms_torch_both - ms_torch_fwd, 4),
               "note": "one working set stays in the 256 MB Infinity Cache; the rotating figure is the one to hold against the HBM peak; "
                       "the torch backward is forward + autograd minus the forward"}


def rate_kernel(n, n_cam, dev):
    P, K, wh = ring_cameras(n_cam, 1920, 1080, device=dev)
    mean = make_world(n, 1920, seed=0, device=dev)[0]
    ms = repeated([lambda: filter3d.sampling_rate(mean, P, K, wh)], launches=20, warmup=3)
    rate = filter3d.sampling_rate(mean, P, K, wh)
    ms_phi = repeated([lambda: filter3d.filter_from_rate(rate)], launches=20, warmup=3)
    return {"measurement": "k_filter3d_rate", "gaussians": n, "cameras": n_cam, "ms_per_call": round(ms, 4), "filter_from_rate_ms": round(ms_phi, 4),
            "gaussian_camera_pairs_per_s": round(n * n_cam / (ms * 1e-3), 0), "rows_seen": int((rate > 0).sum()),
            "note": "the call includes the wrapper's output allocation and its zero fill; 12 + 4 bytes per Gaussian, the cameras through scalar loads"}


def training_step(n, rounds, dev):
    P, K, wh = ring_cameras(1, 1920, 1080, device=dev)
    world = make_world(n, 1920, 2.0, seed=0, device=dev)
    models = {"without": gm.GS_model_with_param(*(t.clone() for t in world)), "filter_3d": gm.GS_model_with_param(*(t.clone() for t in world), filter_3d=True)}
    models["filter_3d"].update_filter_3d(P, K, wh)
    with torch.no_grad():
        target = torch.rand_like(models["without"](P, K, wh, [0])[0])

    def step(model):
        gm.splat_loss(model(P, K, wh, [0])[0], target).backward()
        model._optimizer.zero_grad(set_to_none=True)

    t = {k: [] for k in models}
    for r in range(rounds + 2):  # two warm-up rounds
        for k, model in models.items():
            ms = timed(lambda: step(model))[0]
            if r >= 2:
                t[k].append(ms)
    return {"measurement": "training step (forward, loss, backward)", "gaussians": n, "image": [1920, 1080],
            **{f"step_ms_{k}_median": round(median(v), 3) for k, v in t.items()}, **{f"step_ms_{k}_all": [round(x, 3) for x in sorted(v)] for k, v in t.items()},
            "difference_ms": round(median(t["filter_3d"]) - median(t["without"]), 3),
            "note": "the two models alternate in one process; a step's host reads (the projection's kept count, the binning's) are in both"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--cameras", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("filter3d_bench measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    for line in apply_kernels(a.gaussians, dev):
        print(json.dumps(line), flush=True)
    print(json.dumps(rate_kernel(a.gaussians, a.cameras, dev)), flush=True)
    print(json.dumps(training_step(a.gaussians, a.rounds, dev)), flush=True)
