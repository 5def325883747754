"""Developer benchmark of density control: `GS_model_with_param.densify_and_prune_device` (csrc/gcp_densify.hip: plan,
row gather with Adam's moments, split samples) against `densify_and_prune` (the reference's op-by-op formulation, which
drops the optimiser) on the same model.

10^6 Gaussians by default, SH degrees 2 and 3 (38 / 59 floats per Gaussian, three times that with Adam's two moments), a
statistic that makes about 5 % of the Gaussians split, 5 % clone and 5 % prune, Adam state present (one step taken).  Every
call changes the model, so each timed call gets a fresh model built outside the timed window; the two paths alternate in one
process; device events around the call plus a synchronise; medians.  Bytes moved are computed from the shapes: every output
row of every gathered tensor is read once and written once (fresh moments are only written), plus the row list.  The row
gather is also timed alone, launch by launch, on the colour tensor (the widest: 27 floats takes the word path, 48 the 16-byte
one) and on its moment, as a share of the 8.0 TB/s HBM peak.  One JSON line per degree.

    python tools/densify_bench.py [--gaussians 1000000] [--degrees 2 3] [--rounds 7]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplegaussiansplat_tk71_amd import _lib  # noqa: E402
from simplegaussiansplat_tk71_amd import gs_model as gm  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, the specification (a float4 copy reaches 6.3e12)
EXTENT = 10.0      # dense_extent 0.1, prune_extent 1.0


def make_world(n, degree, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    rand = lambda *s: torch.rand(*s, device=dev, generator=g)  # noqa: E731
    u = rand(n)
    # 5 % split (hot, large), 5 % clone (hot, small), 5 % pruned (half by opacity, half by scale), the rest kept
    split, clone, faint, huge = u < 0.05, (u >= 0.05) & (u < 0.10), (u >= 0.10) & (u < 0.125), (u >= 0.125) & (u < 0.15)
    largest = torch.full((n,), 0.05, device=dev)
    largest[split] = 0.3
    largest[huge] = 1.5
    scale = largest[:, None] * (0.3 + 0.7 * rand(n, 3))
    scale[:, 0] = largest
    opacity = torch.logit(0.1 + 0.8 * rand(n, 1))
    opacity[faint] = -7.0
    views = torch.randint(1, 6, (n,), device=dev, generator=g)
    norm = views.float() * torch.where(split | clone, 1.0 + rand(n), 0.1 * rand(n))
    world = {"mean": torch.randn(n, 3, device=dev, generator=g), "variance_q": torch.randn(n, 4, device=dev, generator=g),
             "variance_scale": torch.log(scale), "opacity": opacity, "color": torch.randn(n, (degree + 1) ** 2, 3, device=dev, generator=g),
             "norm": norm, "views": views.to(torch.int16)}
    world["grads"] = {k: torch.randn(world[k].shape, device=dev, generator=g) for k in ("mean", "variance_q", "variance_scale", "opacity", "color")}
    return world


def make_model(world, degree):
    model = gm.GS_model_with_param(*(world[k].clone() for k in ("mean", "variance_q", "variance_scale", "opacity")), L_max=degree,
                                   grad_threshold=0.5, percent_dense=0.01, prunning_min_opacity=0.005)
    with torch.no_grad():
        model.color.copy_(world["color"])
    for k, p in model.named_parameters():
        p.grad = world["grads"][k].clone()
    model.train_step()  # Adam state present
    model.mean_grads_norm, model.mean_grads_iter = world["norm"].clone(), world["views"].clone()
    return model


def timed(call):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def rows_alone(n, width, dev, launches=20):
    """One k_densify_rows launch on (n, width) floats with the benchmark's action mix, parameters and moments: ms per launch."""
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(1)
    u = torch.rand(n, device=dev, generator=g)
    count = torch.where(u < 0.10, 2, torch.where(u < 0.15, 0, 1))
    src_row = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int32), count)
    first = torch.ones_like(src_row, dtype=torch.bool)
    first[1:] = src_row[1:] != src_row[:-1]
    kind = torch.where(first & (u[src_row.long()] >= 0.05), 0, torch.where(u[src_row.long()] < 0.05, 2, 1)).to(torch.uint8)
    m = src_row.numel()
    src, dst = torch.randn(n, width, device=dev, generator=g), torch.empty(m, width, device=dev)
    out = {}
    for mode, name in ((0, "parameters"), (1, "moments")):
        def launch():
            _lib.check(lib.gcp_densify_rows(src.data_ptr(), n, src_row.data_ptr(), kind.data_ptr(), m, width, mode, dst.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream), "gcp_densify_rows")
        for _ in range(3):
            launch()
        ms = timed(lambda: [launch() for _ in range(launches)])[0] / launches
        carried = m if mode == 0 else int((kind == 0).sum())
        moved = 4 * width * (m + carried) + 5 * m
        out[name] = {"ms": round(ms, 4), "bytes": moved, "tb_per_s": round(moved / ms / 1e9, 3), "share_of_hbm_peak": round(moved / (ms * 1e-3) / HBM_PEAK, 3)}
    return out


def run(n, degree, rounds):
    dev = torch.device("cuda", 0)
    world = make_world(n, degree, dev)
    t_dev, t_ref, sizes = [], [], None
    for r in range(rounds + 2):  # two warm-up rounds
        model = make_model(world, degree)
        ms, (n0, n1) = timed(lambda: model.densify_and_prune_device(EXTENT, seed=r))
        model = make_model(world, degree)
        torch.manual_seed(r)
        ms_ref, _ = timed(lambda: model.densify_and_prune(EXTENT))
        if r >= 2:
            t_dev.append(ms)
            t_ref.append(ms_ref)
        sizes = (n0, n1, model.mean.shape[0])
    floats = 10 + 1 + 3 * (degree + 1) ** 2
    n0, n1, n_ref = sizes
    # per output row: parameters read + written, two moments read + written (fresh rows: written only, counted as carried: an upper bound),
    # the row list written and read by 15 launches
    moved = n1 * floats * 4 * 2 * 3 + n1 * 5 * 16 + n0 * (4 + 4 + 12 + 4 + 4 + 1 + 4)
    width = 3 * (degree + 1) ** 2
    return {"gaussians": n0, "sh_degree": degree, "floats_per_gaussian": floats, "rows_after_device": n1, "rows_after_reference": n_ref,
            "device_ms_median": round(median(t_dev), 3), "device_ms_all": [round(t, 3) for t in t_dev],
            "reference_ms_median": round(median(t_ref), 3), "reference_ms_all": [round(t, 3) for t in t_ref],
            "reference_over_device": round(median(t_ref) / median(t_dev), 2), "bytes_moved_device_upper_bound": moved,
            "device_tb_per_s_end_to_end": round(moved / median(t_dev) / 1e9, 3),
            f"gcp_densify_rows_alone_width_{width}": rows_alone(n0, width, dev),
            "note": "the reference path also rebuilds Adam without moments; its row count can differ (there a split child that is still small enough is cloned in the same call)"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--degrees", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("densify_bench measures on the GPU: no device visible")
    for degree in a.degrees:
        print(json.dumps(run(a.gaussians, degree, a.rounds)), flush=True)
