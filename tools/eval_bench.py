"""Developer benchmark of the evaluation metrics (gcp_image_metrics, csrc/gcp_loss.hip: k_image_metrics + k_metrics_fold)
against the training loss's forward called without maps (gcp_ssim_l1_forward: k_ssim_l1_fwd, which this feature leaves as it
is) in the same process, at 1 x 3 x 1080 x 1920 and 8 x 3 x 1080 x 1920.  Both are called through the C ABI on preallocated
buffers, so a window holds launches only.  For information, the float32 PyTorch formulation of the three metrics on the
same GPU.

Timing: device events around a window of consecutive calls, the number of calls per window chosen per variant so that a
window lasts at least `--window-s` (0.2 s); every variant warmed up first; a pass takes `--windows` windows per variant, the
variants alternating window by window, and reports the median; two passes, and the spread of a variant is the difference of
its two medians over the smaller one.  Condition: the new call's median <= max(1.10, 1 + 3 * spread of the loss forward)
times the loss forward's median.  Bytes needed: 8 B per pixel-channel (both images read once).  One JSON line per variant
and one per comparison.

`--end-to-end`: `GS_model_with_param.evaluate` on 8 ring cameras of a cfg3-like world (synthetic.make_world: 10^6 Gaussians
of about 2 px at 1920 x 1080 — the camera-space counterpart of the 2-D scene tools/contrib_bench.py blends) against `render`
under no_grad, wall clock with a synchronise, median of `--rounds`.

    python tools/eval_bench.py [--windows 5] [--window-s 0.2] [--end-to-end] [--rounds 5]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from densify_bench import HBM_PEAK, median  # noqa: E402
from exposure_bench import passes_of  # noqa: E402
from simplegaussiansplat_tk71_amd import _lib, loss, synthetic  # noqa: E402
from simplegaussiansplat_tk71_amd import gs_model as gm  # noqa: E402

SHAPES = [(1, 3, 1080, 1920), (8, 3, 1080, 1920)]
C1, C2 = 1e-4, 9e-4


def torch_metrics(a, b, window):
    """The float32 PyTorch formulation: clamp, five reflect-padded separable blurs, the SSIM map, three per-image means."""
    a = a.clamp(0, 1)
    ch = a.shape[1]
    kx, ky = window.view(1, 1, 1, -1).expand(ch, 1, 1, -1), window.view(1, 1, -1, 1).expand(ch, 1, -1, 1)

    def blur(t):
        t = torch.nn.functional.pad(t, (5, 5, 5, 5), mode="reflect")
        return torch.nn.functional.conv2d(torch.nn.functional.conv2d(t, kx, groups=ch), ky, groups=ch)

    mu1, mu2 = blur(a), blur(b)
    s11, s22, s12 = blur(a * a) - mu1 * mu1, blur(b * b) - mu2 * mu2, blur(a * b) - mu1 * mu2
    ssim = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2) + 1e-12)
    d = a - b
    return (d * d).mean(dim=(1, 2, 3)), d.abs().mean(dim=(1, 2, 3)), ssim.mean(dim=(1, 2, 3))


def measure(shape, windows, window_s, dev):
    bsz, ch, h, w = shape
    g = torch.Generator(device=dev).manual_seed(1)
    a = -0.1 + 1.2 * torch.rand(shape, device=dev, generator=g)
    b = torch.rand(shape, device=dev, generator=g)
    lib, win = _lib.load(), loss._host_window(11, 1.5)
    blocks = lib.gcp_ssim_blocks(bsz * ch, h, w)
    partial3 = torch.empty(blocks, 3, dtype=torch.float32, device=dev)
    partial2 = torch.empty(blocks, 2, dtype=torch.float32, device=dev)
    out = torch.empty(bsz, 3, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    window = torch.tensor(list(win), dtype=torch.float32, device=dev)

    def metrics():
        _lib.check(lib.gcp_image_metrics(a.data_ptr(), b.data_ptr(), bsz, ch, h, w, win, C1, C2, _lib.METRICS_CLAMP, partial3.data_ptr(),
                                         out.data_ptr(), stream), "gcp_image_metrics")

    def loss_forward():
        _lib.check(lib.gcp_ssim_l1_forward(a.data_ptr(), b.data_ptr(), bsz * ch, h, w, win, C1, C2, None, None, None, partial2.data_ptr(),
                                           stream), "gcp_ssim_l1_forward")

    variants = {"image_metrics": metrics, "loss_forward_no_maps": loss_forward, "torch_float32": lambda: torch_metrics(a, b, window)}
    # the windows of exposure_bench: its calibration measures whole windows (ten calls alone overestimate a call by a quarter,
    # and a window sized by them fell short of `window_s`)
    moved = 8 * bsz * ch * h * w
    res = {}
    for k, (p1, p2, n_calls) in passes_of(variants, windows, window_s).items():
        res[k] = {"measurement": "per-image metrics", "variant": k, "shape": list(shape), "ms_pass_1": round(p1, 5), "ms_pass_2": round(p2, 5),
                  "ms_median": round(0.5 * (p1 + p2), 5), "spread": round(abs(p1 - p2) / min(p1, p2), 4), "bytes_needed": moved,
                  "tb_per_s": round(moved / (0.5 * (p1 + p2)) / 1e9, 3), "share_of_hbm_peak": round(moved / (0.5 * (p1 + p2) * 1e-3) / HBM_PEAK, 3),
                  "calls_per_window": n_calls, "windows_per_pass": windows}
    got = [t.cpu() for t in torch_metrics(a, b, window)]  # the two formulations agree on what they measured
    res["image_metrics"]["max_abs_difference_to_torch_float32"] = max(float((out[:, i].cpu() - got[i].double()).abs().max()) for i in range(3))
    new, old = res["image_metrics"], res["loss_forward_no_maps"]
    ratio, allowed = new["ms_median"] / old["ms_median"], max(1.10, 1 + 3 * old["spread"])
    comparison = {"measurement": "comparison", "shape": list(shape), "new": "image_metrics", "old": "loss_forward_no_maps", "new_over_old": round(ratio, 4),
                  "allowed": round(allowed, 4), "spread_of_old": old["spread"], "condition_holds": bool(ratio <= allowed),
                  "torch_float32_over_new": round(res["torch_float32"]["ms_median"] / new["ms_median"], 2)}
    return list(res.values()) + [comparison]


def end_to_end(rounds, dev, n_gauss=1_000_000, n_cam=8, width=1920, height=1080):
    mean, q, scale, opacity = synthetic.make_world(n_gauss, width, device=dev)
    model = gm.GS_model_with_param(mean, q, scale, opacity)
    P, K, wh = synthetic.ring_cameras(n_cam, width, height, device=dev)
    targets = torch.rand(n_cam, 3, height, width, device=dev, generator=torch.Generator(device=dev).manual_seed(2))

    def wall(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def render():
        with torch.no_grad():
            return model.render(P, K, wh)[0]

    t_eval, t_render, peak = [], [], {}
    for r in range(rounds + 1):  # one warm-up round
        for name, call, ts in (("evaluate", lambda: model.evaluate(P, K, wh, targets), t_eval), ("render", render, t_render)):
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            ms, out = wall(call)
            peak[name] = torch.cuda.max_memory_allocated(dev) - base
            del out
            if r:
                ts.append(ms)
    return {"measurement": "evaluate end to end", "gaussians": n_gauss, "cameras": n_cam, "width": width, "height": height, "rounds": rounds,
            "ms_evaluate_median": round(median(t_eval), 3), "ms_render_no_grad_median": round(median(t_render), 3),
            "ms_evaluate_min_max": [round(min(t_eval), 3), round(max(t_eval), 3)], "ms_render_min_max": [round(min(t_render), 3), round(max(t_render), 3)],
            "evaluate_over_render": round(median(t_eval) / median(t_render), 3), "peak_bytes_evaluate": peak["evaluate"], "peak_bytes_render": peak["render"]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5, help="windows per variant and pass")
    ap.add_argument("--window-s", type=float, default=0.2, help="least duration of a window")
    ap.add_argument("--end-to-end", action="store_true", help="also time GS_model_with_param.evaluate against render under no_grad")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    for shape in SHAPES:
        for line in measure(shape, a.windows, a.window_s, dev):
            print(json.dumps(line), flush=True)
    if a.end_to_end:
        print(json.dumps(end_to_end(a.rounds, dev)), flush=True)
