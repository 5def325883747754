"""Developer benchmark of the lens undistortion (csrc/gcp_undistort.hip) on uint8 (n, H, W, 3) photographs, at two shapes:

    100 x 427 x 640    tests/golden/colmap_scene: every image through its own OPENCV lens of the fixture's cameras.bin
    8 x 1080 x 1920    one OPENCV lens (the coefficients of the fixture's camera 1, f = 1500) for all

Each image's output camera is the one `lens.fit_pinhole` gives.  Four variants in one process, on the same bytes:

    (a) hip            gcp_undistort_u8 through the C ABI on preallocated buffers, the lens records already on the device
    (b) hip_python     lens.undistort: the same launch with the host checks, the records' upload and the output's allocation
    (c) torch          the PyTorch formulation of the same work: uint8 -> float, / 255, permute to (n, 3, H, W), the per-image
                       (n, H, W, 2) grid from the pixel centres through the distortion formulas, F.grid_sample(bilinear,
                       padding_mode="border", align_corners=False)
    (d) torch_sample   (c) with the grid computed beforehand: the conversion and grid_sample alone

Timing as tools/exposure_bench.py (`passes_of`): device events around a window of consecutive calls of at least `--window-s`,
the variants alternating window by window, `--windows` windows per pass, the median of a pass, two passes; the spread of a
variant is the difference of its two medians over the smaller.  Bytes needed by all alike: 3 B read + 12 B written per pixel.
Gate (reported, one line per shape): (a) is not slower than (c).  One JSON line per variant and comparison, and one with the
largest difference between (a) and (c) and the largest coordinate error of the kernel against float64 on a 4096 x 2731 ramp.

    python tools/undistort_bench.py [--windows 5] [--window-s 0.2]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from exposure_bench import passes_of, record  # noqa: E402
from simplegaussiansplat_tk71_amd import _lib, colmap_io, lens  # noqa: E402

SCENE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "colmap_scene", "sparse", "0")
CAMERA_1 = {"k": (-0.115, 0.068, 0.0, 0.0, 0.0, 0.0), "p": (-2.8e-4, 5.4e-3)}


def scene_lenses():
    return [lens.lens_from_colmap(c) for c in colmap_io.read_cameras(os.path.join(SCENE, "cameras.bin")).values()]


def one_lens(width, height, f):
    return lens.Lens("polynomial", f, 1.02 * f, width / 2 + 0.3, height / 2 - 0.2, width, height, **CAMERA_1)


def torch_grid(records, height, width):
    """(n, H, W, 2) normalised sampling positions for F.grid_sample(align_corners=False) from the device records (n, LENS_WORDS),
    polynomial lenses, float32 on the device."""
    r = records[:, :, None, None]
    i = torch.arange(width, dtype=torch.float32, device=records.device)[None, None, :]
    j = torch.arange(height, dtype=torch.float32, device=records.device)[None, :, None]
    x, y = (i + 0.5 - r[:, 6]) / r[:, 4], (j + 0.5 - r[:, 7]) / r[:, 5]
    r2 = x * x + y * y
    radial = (1 + r2 * (r[:, 8] + r2 * (r[:, 9] + r2 * r[:, 10]))) / (1 + r2 * (r[:, 11] + r2 * (r[:, 12] + r2 * r[:, 13])))
    xd = x * radial + 2 * r[:, 14] * x * y + r[:, 15] * (r2 + 2 * x * x)
    yd = y * radial + 2 * r[:, 15] * x * y + r[:, 14] * (r2 + 2 * y * y)
    u, v = r[:, 0] * xd + r[:, 2], r[:, 1] * yd + r[:, 3]
    return torch.stack([u * (2.0 / width) - 1, v * (2.0 / height) - 1], dim=-1)


def torch_undistort(photos, grid):
    planes = (photos.float() / 255).permute(0, 3, 1, 2)
    return torch.nn.functional.grid_sample(planes, grid, mode="bilinear", padding_mode="border", align_corners=False)


def measure(lenses, windows, window_s, dev):
    n, height, width = len(lenses), lenses[0].height, lenses[0].width
    assert all(one.kind == "polynomial" for one in lenses)
    K = torch.stack([lens.fit_pinhole(one)[0] for one in lenses])
    photos = torch.randint(0, 256, (n, height, width, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    records = lens.lens_records(lenses, K).to(dev)
    out = torch.empty(n, 3, height, width, device=dev)
    lib, stream = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
    grid = torch_grid(records, height, width)
    variants = {
        "hip": lambda: _lib.check(lib.gcp_undistort_u8(photos.data_ptr(), records.data_ptr(), n, height, width, out.data_ptr(), stream), "hip"),
        "hip_python": lambda: lens.undistort(photos, lenses, K),
        "torch": lambda: torch_undistort(photos, torch_grid(records, height, width)),
        "torch_sample": lambda: torch_undistort(photos, grid),
    }
    shape, moved = (n, height, width, 3), 15 * n * height * width
    # `passes_of` collects what a call returns over a window: nothing here, or a window would hold every output at once
    discard = {k: (lambda call=call: (call(), None)[1]) for k, call in variants.items()}
    res = {k: record("undistort u8", k, shape, *v, windows, moved) for k, v in passes_of(discard, windows, window_s).items()}
    variants["hip"]()
    difference = float((out - variants["torch"]()).abs().max())
    a, c = res["hip"], res["torch"]
    gate = {"measurement": "gate", "shape": list(shape), "torch_over_hip": round(c["ms_median"] / a["ms_median"], 4),
            "torch_sample_over_hip": round(res["torch_sample"]["ms_median"] / a["ms_median"], 4),
            "larger_spread": max(a["spread"], c["spread"]), "hip_not_slower": bool(a["ms_median"] <= c["ms_median"]),
            "max_abs_difference_hip_to_torch": difference}
    return list(res.values()) + [gate]


def coordinate_error(dev, width=4096, height=2731, f=3000.0):
    """The kernel on a float32 ramp (x + 0.5, y + 0.5) against `lens.distort` in float64: the largest coordinate error in pixels.
    The ramp's own interpolation rounds to float32 too: up to 2.4e-4 px of the figure at coordinates above 2048."""
    one = one_lens(width, height, f)
    K, scale = lens.fit_pinhole(one)
    j, i = torch.meshgrid(torch.arange(height, dtype=torch.float32), torch.arange(width, dtype=torch.float32), indexing="ij")
    ramp = torch.stack([i + 0.5, j + 0.5, torch.zeros_like(i)])[None].to(dev)
    got = lens.undistort(ramp, [one], K)[0, :2].double().cpu().numpy()
    xy = np.stack([(i.double().numpy() + 0.5 - one.cx) / (scale * one.fx), (j.double().numpy() + 0.5 - one.cy) / (scale * one.fy)], axis=-1)
    uv = lens.distort(one, xy) * np.array([one.fx, one.fy]) + np.array([one.cx, one.cy])
    uv = np.clip(uv, 0.5, np.array([width - 0.5, height - 0.5]))
    return {"measurement": "coordinate error against float64", "shape": [1, 3, height, width], "fitted_scale": scale,
            "max_error_px": [float(np.abs(got[0] - uv[..., 0]).max()), float(np.abs(got[1] - uv[..., 1]).max())]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5, help="windows per variant and pass")
    ap.add_argument("--window-s", type=float, default=0.2, help="least duration of a window")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("undistort_bench measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    for lenses in (scene_lenses(), [one_lens(1920, 1080, 1500.0)] * 8):
        for line in measure(lenses, a.windows, a.window_s, dev):
            print(json.dumps(line), flush=True)
    print(json.dumps(coordinate_error(dev)), flush=True)
