"""Developer benchmark of the mesh extraction (csrc/gcp_tsdf.hip, simplegaussiansplat_tk71_amd/mesh.py); no effect on bench.py.

Per volume size (256^3 and 512^3 lattice points over the cube [-1.2, 1.2]^3, trunc = 5 voxels), on analytic maps of a sphere of
radius 0.8 seen by 8 ring cameras at 1080 x 1920 (alpha in [0.6, 1] on the sphere, 0 beside it; a colour image):

  integrate   `TSDFVolume.integrate` of the 8 cameras in ONE launch, with and without the colour volume, against the same
              update rule written in float32 PyTorch (a gather by nearest pixel, `torch.where` per camera; the lattice
              coordinates are precomputed outside the timed window, which favours PyTorch) on the same inputs, ALTERNATING
              within every round.  The timed kernel call integrates into the volume as it stands (the work does not depend on
              what it holds); the PyTorch call is functional on a fresh state allocated outside the window.  The two results
              from a fresh volume are compared, and the kernel's bit for bit between a run before and a run after the rounds.
  extract     `extract_surface` of the fused volume (weights and colours) and of the analytic field alone: count, two scans,
              the host read, write.

Times are device events around the call followed by a synchronise; medians, minima and maxima over the rounds after the warm-up
rounds, every shape warmed first.  bytes_per_point is what the integration must move (state read + written); the share of the
HBM roof is that over the median time over 6.3 TB/s (the measured copy rate of the MI355X; 8 TB/s is the specification).

    python tools/mesh_bench.py [--rounds 7] [--warmup 2] [--sizes 256,512]

One JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplegaussiansplat_tk71_amd import mesh, synthetic  # noqa: E402

HBM_ROOF = 6.3e12
WIDTH, HEIGHT, CAMERAS, RADIUS, HALF = 1920, 1080, 8, 0.8, 1.2
DEPTH_MAX = 6.4  # twice the cameras' distance: 2DGS's bound; the sphere's depths are 2.4 .. 3.2


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
    times, first, last = {k: [] for k in calls}, {}, {}
    for r in range(rounds + warmup):
        for key, call in calls.items():
            ms, out = timed(call)
            if r >= warmup:
                times[key].append(ms)
                first.setdefault(key, out)
                last[key] = out
    return times, first, last


def sphere_maps(P, K, dev):
    """depth = z alpha, alpha, image of the sphere |x| = RADIUS, float32 on the device."""
    y, x = torch.meshgrid(torch.arange(HEIGHT, dtype=torch.float64, device=dev), torch.arange(WIDTH, dtype=torch.float64, device=dev),
                          indexing="ij")
    depth, alpha, image = [], [], []
    for c in range(P.shape[0]):
        R, t = P[c, :, :3].double(), P[c, :, 3].double()
        eye = -R.T @ t
        ray = torch.stack([(x + 0.5 - K[c, 0, 2]) / K[c, 0, 0], (y + 0.5 - K[c, 1, 2]) / K[c, 1, 1], torch.ones_like(x)], dim=-1) @ R
        a2, b, c0 = (ray * ray).sum(-1), ray @ eye, float(eye @ eye) - RADIUS * RADIUS
        disc = b * b - a2 * c0
        hit = (disc > 0) & (-b > 0)
        z = torch.where(hit, (-b - disc.clamp_min(0).sqrt()) / a2, torch.zeros_like(b))
        a = torch.where(hit, 0.6 + 0.4 * (0.5 + 0.5 * torch.sin(0.017 * x + 0.009 * y + c)), torch.zeros_like(b))
        depth.append((z * a)[None].float())
        alpha.append(a[None].float())
        image.append(torch.stack([0.5 + 0.5 * torch.sin(0.003 * x + c), 0.5 + 0.5 * torch.cos(0.004 * y - c), (x + y) / (WIDTH + HEIGHT)]).float())
    return torch.stack(depth), torch.stack(alpha), torch.stack(image)


def torch_integrate(state, xw, trunc, depth, alpha, image, P, K, alpha_min, depth_max):
    """The update rule of `TSDFVolume.integrate` in float32 PyTorch; state = (tsdf, weight, rgb or None) flat, returned new."""
    tsdf, weight, rgb = state
    h, w = depth.shape[-2:]
    for c in range(depth.shape[0]):
        p = xw @ P[c, :, :3].T + P[c, :, 3]
        z = p[:, 2]
        live = z > 0
        zs = torch.where(live, z, torch.ones_like(z))
        u = K[c, 0, 0] * p[:, 0] / zs + K[c, 0, 2]
        v = K[c, 1, 1] * p[:, 1] / zs + K[c, 1, 2]
        live = live & (u >= 0) & (u < w) & (v >= 0) & (v < h)
        pixel = v.clamp(0, h - 1).long() * w + u.clamp(0, w - 1).long()
        a, D = alpha[c, 0].reshape(-1)[pixel], depth[c, 0].reshape(-1)[pixel]
        live = live & (a >= alpha_min) & (D > 0)
        d = D / torch.where(live, a, torch.ones_like(a))
        if depth_max > 0:
            live = live & ~(d > depth_max)
        s = d - z
        live = live & ~(s < -trunc)
        tau = torch.clamp(s / trunc, max=1.0)
        w1 = weight + 1
        tsdf = torch.where(live, (tsdf * weight + tau) / w1, tsdf)
        if rgb is not None:
            rgb = torch.where(live, (rgb * weight + image[c].reshape(3, -1)[:, pixel]) / w1, rgb)
        weight = torch.where(live, w1, weight)
    return tsdf, weight, rgb


def bench_size(n, dev, rounds, warmup, maps, P, K):
    depth, alpha, image = maps
    voxel = 2 * HALF / (n - 1)
    trunc, origin = 5 * voxel, (-HALF, -HALF, -HALF)
    points = n ** 3
    axis = -HALF + voxel * torch.arange(n, dtype=torch.float32, device=dev)
    kk, jj, ii = torch.meshgrid(axis, axis, axis, indexing="ij")
    xw = torch.stack([ii, jj, kk], dim=-1).reshape(-1, 3)
    out = {"points": points, "voxel": voxel, "trunc": trunc, "integrate": {}}
    volumes = {}
    for colour in (False, True):
        vol = mesh.TSDFVolume(origin, voxel, (n, n, n), trunc, dev, colour=colour)
        volumes[colour] = vol

        def fused(vol=vol, colour=colour):
            vol.reset()
            vol.integrate(depth, alpha, P, K, image=image if colour else None, alpha_min=0.5, depth_max=DEPTH_MAX)
            return vol.tsdf.clone(), vol.weight.clone()

        def hip(vol=vol, colour=colour):  # into the volume as it stands: the same work whatever it holds
            vol.integrate(depth, alpha, P, K, image=image if colour else None, alpha_min=0.5, depth_max=DEPTH_MAX)

        fresh = (torch.ones(points, device=dev), torch.zeros(points, device=dev), torch.zeros(3, points, device=dev) if colour else None)

        def ref(colour=colour, fresh=fresh):
            return torch_integrate(fresh, xw, trunc, depth, alpha, image, P, K, 0.5, DEPTH_MAX)

        before = fused()
        times, first, last = alternate({"hip": hip, "torch": ref}, rounds, warmup)
        first["hip"], last["hip"] = before, fused()
        med = {k: stats(v) for k, v in times.items()}
        bytes_per_point = 40 if colour else 16
        got_f, got_w = last["hip"]
        want_f, want_w, _ = last["torch"]
        out["integrate"]["colour" if colour else "plain"] = {
            "ms": med, "torch_over_hip": round(med["torch"]["median"] / med["hip"]["median"], 2), "bytes_per_point": bytes_per_point,
            "hip_tb_per_s": round(bytes_per_point * points / (med["hip"]["median"] * 1e-3) / 1e12, 3),
            "hip_share_of_hbm_roof": round(bytes_per_point * points / (med["hip"]["median"] * 1e-3) / HBM_ROOF, 3),
            "weights_that_differ_from_float32_torch": int((got_w.reshape(-1) != want_w).sum()),
            "tsdf_max_abs_difference_where_weights_agree": float((got_f.reshape(-1) - want_f).abs()[got_w.reshape(-1) == want_w].max()),
            "observed_points": int((got_w > 0).sum()),
            "bit_equal_before_and_after_the_rounds": all(torch.equal(a, b) for a, b in zip(first["hip"], last["hip"]))}
        del times, first, last, got_f, got_w, want_f, want_w
    vol = volumes[True]
    field = ((xw.norm(dim=1) - RADIUS) / trunc).clamp(-1, 1).reshape(n, n, n)
    del xw
    calls = {"fused": lambda: vol.extract(), "analytic": lambda: mesh.extract_surface(field, origin=origin, voxel=voxel)}
    times, first, last = alternate(calls, rounds, warmup)
    out["extract"] = {k: {"ms": stats(times[k]), "vertices": int(last[k][0].shape[0]), "faces": int(last[k][1].shape[0]),
                          "bit_equal_first_and_last_round": all(torch.equal(a, b) for a, b in zip(first[k], last[k]) if a is not None)}
                      for k in calls}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="256,512")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    P, K, _ = synthetic.ring_cameras(CAMERAS, WIDTH, HEIGHT, radius=3.2, device=dev)
    maps = sphere_maps(P, K, dev)
    out = {"rounds": a.rounds, "warmup": a.warmup, "cameras": CAMERAS, "height": HEIGHT, "width": WIDTH,
           "hit_fraction": round(float((maps[1] > 0).float().mean()), 4), "hbm_roof_tb_per_s": HBM_ROOF / 1e12,
           "sizes": {str(n): bench_size(int(n), dev, a.rounds, a.warmup, maps, P, K) for n in a.sizes.split(",")}}
    print(json.dumps(out), flush=True)
