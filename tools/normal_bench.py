"""Developer benchmark of the normals (csrc/gcp_normal.hip, simplegaussiansplat_tk71_amd/normals.py); no effect on bench.py.

Three measurements, each forward + backward as a training step calls it, between two device events and followed by a
synchronise; the variants of a measurement ALTERNATE within every round; medians, minima and maxima over the rounds after the
warm-up rounds (every call runs at the timed shape before anything is timed); the ratios are those of the same run:

  consistency   `normal_consistency` (k_nc_fwd + the float64 fold, k_nc_bwd) at B x 1080 x 1920, B = 8 and B = 1, against the
                same statements in float32 PyTorch under autograd (tests/normal_torch.py) on the same maps; the two losses and
                gradients are compared, and the kernels' outputs bit for bit between the first and the last round;
  normals       `gaussian_normals` at 10^6 rows, the list a permutation of all of them;
  step          `cuda_kernel.render` forward + backward on the cfg3 scene with random upstream gradients on
                every map, without and with `normal=`: the difference is the price of the second colour blend in each direction.

    python tools/normal_bench.py [--rounds 15] [--skip-step]

One JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplegaussiansplat_tk71_amd import cuda_kernel as ck  # noqa: E402
from simplegaussiansplat_tk71_amd import normals, synthetic  # noqa: E402
from tests import normal_torch as nt  # noqa: E402


def timed(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stats(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "max": round(ts[-1], 4)}


def alternate(calls, rounds, warmup):
    """-> ({name: [ms]}, {name: first timed output}, {name: last output})"""
    times, first, last = {k: [] for k in calls}, {}, {}
    for r in range(rounds + warmup):
        for key, call in calls.items():
            ms, out = timed(call)
            if r >= warmup:
                times[key].append(ms)
                first.setdefault(key, out)
                last[key] = out
    return times, first, last


def maps(batch, height, width, dev, seed=0):
    """The maps of tests/normal_cases.py at a user's size: alpha in [0.3, 1] with 8 % exact zeros, depth = alpha * U(2, 5),
    normal = a direction * alpha * U(0, 1), a K per image."""
    g = torch.Generator(device=dev).manual_seed(seed)
    rand = lambda *s: torch.rand(*s, device=dev, generator=g)  # noqa: E731
    alpha = 0.3 + 0.7 * rand(batch, 1, height, width)
    alpha = torch.where(rand(batch, 1, height, width) < 0.08, torch.zeros_like(alpha), alpha)
    depth = alpha * (2.0 + 3.0 * rand(batch, 1, height, width))
    direction = torch.randn(batch, 3, height, width, device=dev, generator=g)
    normal = direction / direction.norm(dim=1, keepdim=True) * alpha * rand(batch, 1, height, width)
    K = torch.zeros(batch, 3, 3, device=dev)
    for b in range(batch):
        f = width * (0.8 + 0.05 * b)
        K[b] = torch.tensor([[f, 0, width / 2 + 0.3 + b], [0, 1.1 * f, height / 2 - 0.2 - 0.5 * b], [0, 0, 1.0]], device=dev)
    return depth, alpha, normal, K


def bench_consistency(batch, height, width, dev, rounds, warmup):
    D, A, N, K = maps(batch, height, width, dev)

    def run(loss_fn):
        leaves = [t.clone().requires_grad_(True) for t in (D, A, N)]
        loss = loss_fn(*leaves)
        loss.backward()
        return (loss.detach(), *(leaf.grad for leaf in leaves))

    calls = {"hip": lambda: run(lambda d, a, n: normals.normal_consistency(d, a, n, K)),
             "torch": lambda: run(lambda d, a, n: nt.normal_consistency(d, a, n, K)[0])}
    times, first, last = alternate(calls, rounds, warmup)
    hip, ref = last["hip"], last["torch"]
    pixels = batch * height * width
    med = {k: stats(v) for k, v in times.items()}
    return {"batch": batch, "height": height, "width": width, "ms": med,
            "torch_over_hip": round(med["torch"]["median"] / med["hip"]["median"], 2),
            # what the two kernels must move: 20 B read forward, 20 B read + 20 B written backward, per pixel
            "hip_gb_per_s_of_60_bytes_per_pixel": round(60 * pixels / (med["hip"]["median"] * 1e-3) / 1e9, 1),
            "loss_hip": float(hip[0]), "loss_torch": float(ref[0]),
            "grad_err_over_scale_vs_float32_torch": [float((a - b).abs().max() / b.abs().max()) for a, b in zip(hip[1:], ref[1:])],
            "bit_equal_first_and_last_round": all(torch.equal(a, b) for a, b in zip(first["hip"], last["hip"]))}


def bench_normals(n, dev, rounds, warmup):
    g = torch.Generator(device=dev).manual_seed(1)
    q = torch.randn(n, 4, device=dev, generator=g)
    scale = torch.randn(n, 3, device=dev, generator=g)
    mean = torch.randn(n, 3, device=dev, generator=g)
    P_c = synthetic.ring_cameras(1, 64, 64, device=dev)[0][0]
    index = torch.randperm(n, device=dev, generator=g)
    G = torch.randn(n, 3, device=dev, generator=g)

    def run():
        leaf = q.clone().requires_grad_(True)
        out = normals.gaussian_normals(leaf, scale, mean, P_c, index)
        out.backward(G)
        return out.detach(), leaf.grad

    times, first, last = alternate({"gaussian_normals": run}, rounds, warmup)
    med = stats(times["gaussian_normals"])
    return {"rows": n, "ms": med, "bit_equal_first_and_last_round": all(torch.equal(a, b) for a, b in zip(first["gaussian_normals"], last["gaussian_normals"]))}


def bench_step(config, dev, rounds, warmup):
    sc = synthetic.make_scene_config(config, seed=0, device=dev)
    w, h, n = sc["width"], sc["height"], sc["start"].size(0)
    z = 1.0 + 9.0 * torch.arange(n, device=dev, dtype=torch.float32) / max(n - 1, 1)  # depth order = index
    g = torch.Generator(device=dev).manual_seed(3)
    nrm = torch.randn(n, 3, device=dev, generator=g)
    nrm = nrm / nrm.norm(dim=1, keepdim=True)
    g_img, g_nmap = (torch.randn(h + 1, w + 1, 3, device=dev, generator=g) for _ in range(2))
    g_dep, g_alp = (torch.randn(h + 1, w + 1, device=dev, generator=g) for _ in range(2))

    def run(with_normal):
        leaves = [sc[k].clone().requires_grad_(True) for k in ("vinv", "opacity", "l_d")] + [z.clone().requires_grad_(True)]
        nl = nrm.clone().requires_grad_(True) if with_normal else None
        out = ck.render(sc["start"], sc["end"], sc["mean"], *leaves, w, h, normal=nl)
        loss = (out[0] * g_img).sum() + (out[1] * g_dep).sum() + (out[2] * g_alp).sum()
        if with_normal:
            loss = loss + (out[3] * g_nmap).sum()
        loss.backward()
        return tuple(leaf.grad for leaf in leaves)

    times, _, _ = alternate({"render": lambda: run(False), "render_with_normal": lambda: run(True)}, rounds, warmup)
    med = {k: stats(v) for k, v in times.items()}
    return {"scene": config, "width": w + 1, "height": h + 1, "gaussians": n, "ms": med,
            "second_blend_ms": round(med["render_with_normal"]["median"] - med["render"]["median"], 4),
            "with_normal_over_without": round(med["render_with_normal"]["median"] / med["render"]["median"], 3)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("normal_bench measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    out = {"rounds": a.rounds, "warmup": a.warmup,
           "consistency": [bench_consistency(b, 1080, 1920, dev, a.rounds, a.warmup) for b in (8, 1)],
           "normals": bench_normals(10 ** 6, dev, a.rounds, a.warmup)}
    if not a.skip_step:
        out["step"] = bench_step(a.config, dev, a.rounds, a.warmup)
    print(json.dumps(out), flush=True)
