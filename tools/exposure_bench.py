"""Developer benchmark of the per-camera exposure compensation fused into the loss kernels (csrc/gcp_loss.hip), at
1 x 3 x 1080 x 1920 and 8 x 3 x 1080 x 1920, forward + backward through autograd, three variants in one process:

    (a) plain      splat_loss(x, b): the kernels this feature leaves as they are
    (b) fused      splat_loss(x, b, exposure=E): k_ssim_l1_fwd_exposure, k_ssim_l1_bwd_exposure, k_exposure_fold
    (c) unfused    splat_loss(apply_exposure(x, E), b): the composition that existed before, the einsum under autograd

x and E require a gradient in (b) and (c), x in (a).  And, through the C ABI on preallocated buffers, the four launches alone
(plain / exposure forward with maps, plain / exposure backward, the latter with its fold).

Timing: device events around a window of consecutive calls, the number of calls per window chosen per variant so that a
window lasts at least `--window-s` (0.2 s); every variant warmed up first; a pass takes `--windows` windows per variant, the
variants alternating window by window, and reports the median; two passes, and the spread of a variant is the difference of
its two medians over the smaller one.
Gate: (b) is faster than (c) by more than three times the larger spread of the two.  Target (reported): (b) <= max(1.10, 1 +
3 * spread of (a)) * (a).  Bytes needed by (a) and (b) alike: 20 B + 24 B per pixel-channel.  One JSON line per variant and
one per comparison.

    python tools/exposure_bench.py [--windows 5] [--window-s 0.2] [--launches-only]

`--launches-only`: the four launches alone (what a kernel trace of them, or a library given through GCP_LIBRARY, is run with).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from densify_bench import HBM_PEAK, median, timed  # noqa: E402
from simplegaussiansplat_tk71_amd import _lib, loss  # noqa: E402

SHAPES = [(1, 3, 1080, 1920), (8, 3, 1080, 1920)]
C1, C2 = 1e-4, 9e-4


def passes_of(variants, windows, window_s):
    """name -> (median of pass 1, median of pass 2, calls per window), ms per call."""
    calls = {}
    for k, call in variants.items():  # warm-up, then the number of calls that fills a window with a quarter to spare
        for _ in range(5):
            call()
        n = 10
        while True:
            total = timed(lambda: [call() for _ in range(n)])[0]
            if total >= 1.25 * window_s * 1e3:
                break
            n = max(2 * n, int(1.5 * window_s * 1e3 * n / max(total, 1e-3)) + 1)
        calls[k] = n
    passes = []
    for _ in range(2):
        t = {k: [] for k in variants}
        for _ in range(windows):
            for k, call in variants.items():
                total = timed(lambda: [call() for _ in range(calls[k])])[0]
                assert total >= window_s * 1e3, (k, total)
                t[k].append(total / calls[k])
        passes.append({k: median(v) for k, v in t.items()})
    return {k: (passes[0][k], passes[1][k], calls[k]) for k in variants}


def record(measurement, name, shape, p1, p2, calls, windows, moved):
    mid = 0.5 * (p1 + p2)
    return {"measurement": measurement, "variant": name, "shape": list(shape), "ms_pass_1": round(p1, 5), "ms_pass_2": round(p2, 5),
            "ms_median": round(mid, 5), "spread": round(abs(p1 - p2) / min(p1, p2), 4), "bytes_needed": moved,
            "tb_per_s": round(moved / mid / 1e9, 3), "share_of_hbm_peak": round(moved / (mid * 1e-3) / HBM_PEAK, 3),
            "calls_per_window": calls, "windows_per_pass": windows}


def measure(shape, windows, window_s, dev, launches_only=False):
    bsz, ch, h, w = shape
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(shape, device=dev, generator=g).requires_grad_(True)
    b = torch.rand(shape, device=dev, generator=g)
    E = (torch.eye(3, 4, device=dev).repeat(bsz, 1, 1) + 0.1 * torch.randn(bsz, 3, 4, device=dev, generator=g)).requires_grad_(True)

    def step(make):
        x.grad = E.grad = None
        make().backward()

    variants = {"plain": lambda: step(lambda: loss.splat_loss(x, b, 0.2)),
                "fused": lambda: step(lambda: loss.splat_loss(x, b, 0.2, exposure=E)),
                "unfused": lambda: step(lambda: loss.splat_loss(loss.apply_exposure(x, E), b, 0.2))}
    n = bsz * ch * h * w
    if launches_only:
        return launches_alone(shape, windows, window_s, dev, x, b, E)
    res = {k: record("loss forward + backward", k, shape, *v, windows, 44 * n) for k, v in passes_of(variants, windows, window_s).items()}
    # the two formulations of the compensated loss agree on what they measured
    outs = {}
    for k in ("fused", "unfused"):
        x.grad = E.grad = None
        value = loss.splat_loss(x, b, 0.2, exposure=E) if k == "fused" else loss.splat_loss(loss.apply_exposure(x, E), b, 0.2)
        value.backward()
        outs[k] = (value.detach().double(), x.grad.double(), E.grad.double())
    res["fused"]["max_abs_difference_to_unfused"] = [float((p - q).abs().max()) for p, q in zip(outs["fused"], outs["unfused"])]
    res["fused"]["max_abs_of_unfused"] = [float(q.abs().max()) for q in outs["unfused"]]
    a, f, u = res["plain"], res["fused"], res["unfused"]
    margin = 3 * max(f["spread"], u["spread"])
    gate = {"measurement": "gate", "shape": list(shape), "unfused_over_fused": round(u["ms_median"] / f["ms_median"], 4),
            "needed": round(1 + margin, 4), "larger_spread": max(f["spread"], u["spread"]), "gate_holds": bool(u["ms_median"] / f["ms_median"] > 1 + margin)}
    allowed = max(1.10, 1 + 3 * a["spread"])
    target = {"measurement": "target", "shape": list(shape), "fused_over_plain": round(f["ms_median"] / a["ms_median"], 4), "allowed": round(allowed, 4),
              "spread_of_plain": a["spread"], "target_holds": bool(f["ms_median"] / a["ms_median"] <= allowed)}
    return list(res.values()) + [gate, target] + launches_alone(shape, windows, window_s, dev, x, b, E)


def launches_alone(shape, windows, window_s, dev, x, b, E):
    """The four launches through the C ABI on preallocated buffers."""
    bsz, ch, h, w = shape
    n = bsz * ch * h * w
    lib, win = _lib.load(), loss._host_window(11, 1.5)
    xd, Ed = x.detach(), E.detach().contiguous()
    maps = [torch.empty_like(xd) for _ in range(3)]
    partial = torch.empty(lib.gcp_ssim_blocks(bsz * ch, h, w), 2, device=dev)
    partial_e = torch.empty(lib.gcp_exposure_blocks(bsz, h, w), 12, device=dev)
    grad, grad_e = torch.empty_like(xd), torch.empty_like(Ed)
    scales = torch.tensor([-0.2 / n, 0.8 / n], device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    m = [t.data_ptr() for t in maps]
    kernels = {
        "forward_plain": lambda: _lib.check(lib.gcp_ssim_l1_forward(xd.data_ptr(), b.data_ptr(), bsz * ch, h, w, win, C1, C2, *m, partial.data_ptr(),
                                                                    stream), "forward"),
        "forward_exposure": lambda: _lib.check(lib.gcp_ssim_l1_forward_exposure(xd.data_ptr(), b.data_ptr(), Ed.data_ptr(), bsz, h, w, win, C1, C2, *m,
                                                                                partial.data_ptr(), stream), "forward_exposure"),
        "backward_plain": lambda: _lib.check(lib.gcp_ssim_l1_backward(xd.data_ptr(), b.data_ptr(), *m, bsz * ch, h, w, win, scales.data_ptr(),
                                                                      grad.data_ptr(), stream), "backward"),
        "backward_exposure": lambda: _lib.check(lib.gcp_ssim_l1_backward_exposure(xd.data_ptr(), b.data_ptr(), Ed.data_ptr(), *m, bsz, h, w, win,
                                                                                  scales.data_ptr(), grad.data_ptr(), partial_e.data_ptr(),
                                                                                  grad_e.data_ptr(), stream), "backward_exposure"),
    }
    kernels["forward_exposure"]()  # the maps the backward variants read
    moved = {"forward_plain": 20 * n, "forward_exposure": 20 * n, "backward_plain": 24 * n, "backward_exposure": 24 * n}
    alone = [record("launches alone", k, shape, *v, windows, moved[k]) for k, v in passes_of(kernels, windows, window_s).items()]
    return alone


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5, help="windows per variant and pass")
    ap.add_argument("--window-s", type=float, default=0.2, help="least duration of a window")
    ap.add_argument("--launches-only", action="store_true", help="only the four launches through the C ABI")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exposure_bench measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    for shape in SHAPES:
        for line in measure(shape, a.windows, a.window_s, dev, a.launches_only):
            print(json.dumps(line), flush=True)
