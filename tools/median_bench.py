"""Developer benchmark of the median depth map (`raster.blend_median_forward` / `blend_median_backward`, csrc/gcp_median.hip:
k_median_fwd, k_median_bwd + k_median_reduce) next to the depth blend whose bins it walks, on the scene tools/distort_bench.py
times (N Gaussians, integer centres uniform in the image, boxes with mean area P*D/N, depth = index; z rises with
the index).

One process, one set of bins; per round the four calls run one after the other, ALTERNATING — blend_forward_depth WITHOUT
checkpoints (what `paint_maps` runs), blend_backward_depth, blend_median_forward, blend_median_backward — each between two
device events and followed by a synchronise; medians, minima and maxima over the rounds after the warm-up rounds (every call
runs at the timed shape before anything is timed).  The ratios are those of the same run.  The median's outputs are compared
bit for bit between the first and the last round.  The share of pixels whose alpha reaches 1/2 — the ones that let a tile's walk
stop — is reported with them.  One JSON line.

    python tools/median_bench.py [--config cfg3] [--rounds 15]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplegaussiansplat_tk71_amd import raster, synthetic  # noqa: E402


def timed(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def run(sc, name, rounds, warmup=3):
    w, h, n = sc["width"], sc["height"], sc["start"].size(0)
    dev = sc["start"].device
    bins = raster.bin_tiles(sc["start"], sc["end"], w, h)
    depth = bins.tile_start[1:] - bins.tile_start[:-1]
    geo = (sc["start"], sc["end"], sc["mean"], sc["vinv"], sc["opacity"])
    z = 1.0 + 9.0 * torch.arange(n, device=dev, dtype=torch.float32) / max(n - 1, 1)  # depth order = index
    image, dmap, alpha, ckpt = raster.blend_forward_depth(bins, *geo, sc["l_d"], z, with_checkpoints=True)
    gen = torch.Generator(device=dev).manual_seed(3)
    g_image = torch.randn(image.shape, device=dev, generator=gen)
    g_depth, g_alpha, g_median = (torch.randn(dmap.shape, device=dev, generator=gen) for _ in range(3))
    med_map, index = raster.blend_median_forward(bins, *geo, z)
    calls = {
        "blend_forward_depth": lambda: raster.blend_forward_depth(bins, *geo, sc["l_d"], z, with_checkpoints=False),
        "blend_backward_depth": lambda: raster.blend_backward_depth(bins, *geo, sc["l_d"], z, ckpt, g_image, g_depth, g_alpha),
        "median_forward": lambda: raster.blend_median_forward(bins, *geo, z),
        "median_backward": lambda: (raster.blend_median_backward(bins, sc["start"], sc["end"], index, g_median),),
    }
    times = {k: [] for k in calls}
    first, last = {}, {}
    for r in range(rounds + warmup):
        for key, call in calls.items():
            ms, out = timed(call)
            if r >= warmup:
                times[key].append(ms)
            if key.startswith("median"):
                first.setdefault(key, out)
                last[key] = out
    med = {k: median(v) for k, v in times.items()}
    crossed = float((alpha >= 0.5).float().mean())
    return {"scene": name, "width": w + 1, "height": h + 1, "gaussians": n, "tile_pairs": bins.n_tile_pairs,
            "deepest_tile_list": int(depth.max()), "mean_tile_list": round(float(depth.float().mean()), 1), "rounds": rounds, "warmup": warmup,
            "ms_median": {k: round(v, 4) for k, v in med.items()}, "ms_min": {k: round(min(v), 4) for k, v in times.items()},
            "ms_max": {k: round(max(v), 4) for k, v in times.items()},
            "median_forward_over_blend_forward": round(med["median_forward"] / med["blend_forward_depth"], 3),
            "median_backward_over_blend_backward": round(med["median_backward"] / med["blend_backward_depth"], 3),
            "bit_equal_first_and_last_round": all(torch.equal(a, b) for k in first for a, b in zip(first[k], last[k])),
            "pixels_with_alpha_at_least_half": round(crossed, 4), "pixels_without_a_pair": round(float((index < 0).float().mean()), 4),
            "gaussians_picked": int(torch.unique(index[index >= 0]).numel()), "median_mean": float(med_map.double().mean())}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--rounds", type=int, default=15)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("median_bench measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    scene = synthetic.make_scene_config(a.config, seed=0, device=dev)
    print(json.dumps(run(scene, a.config, a.rounds)), flush=True)
