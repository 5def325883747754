"""Developer benchmark of the projection kernels (csrc/gcp_project.hip) by SH degree and direction frame: 10^6 Gaussians
(synthetic.make_world), one 1920x1080 camera.

Per case (degree 2 camera / world, degree 3 camera / world): gcp_project_forward[_sh] + gcp_project_gather (the depth
permutation is sorted once, outside the timing; the list keeps all Gaussians, so nothing is read back) and
gcp_project_backward[_sh] with random upstream gradients — device events, warm-up, median of alternating rounds.  Bytes per
Gaussian follow from the shapes of the arrays the kernels read and write; bytes/s is set against the 8 TB/s HBM peak.

--other-lib PATH: a second build of the library (e.g. the parent commit's, built into a directory of its own) runs the
degree-2 camera-frame case through the entry points both have, alternating with this checkout's in every round; it runs
twice per round, and the spread of its own medians is the margin a difference has to exceed to mean anything.

    python tools/sh_bench.py [--gaussians 1000000] [--rounds 7] [--other-lib PATH]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplegaussiansplat_tk71_amd import _lib, gs_model, raster, synthetic  # noqa: E402

HBM_PEAK = 8e12  # bytes/s


def timeit(fn, iters=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def load_other(path):
    """A second build of the library; only the entry points it exports are bound."""
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def nbytes(*tensors):
    return sum(t.numel() * t.element_size() for t in tensors)


class Case:
    """One (library, degree, frame): buffers, the two timed calls and their bytes per Gaussian."""

    def __init__(self, lib, world, degree, frame, use_sh_entry):
        self.lib, self.degree, self.frame, self.sh_entry = lib, degree, gs_model.SH_FRAMES[frame], use_sh_entry
        dev = world["mean"].device
        n = self.n = world["mean"].shape[0]
        nb = (degree + 1) ** 2
        self.params = [world[k] for k in ("mean", "variance_q", "variance_scale", "opacity")] + [world["color"][:, :nb].contiguous()]
        self.cam = [world["P"][0].contiguous(), world["K"][0].contiguous()]
        self.size = (world["width"], world["height"], gs_model._box_clamp(world["width"], world["height"], world["tile_logit"]))
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)  # noqa: E731
        i64 = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)  # noqa: E731
        self.record, self.sort_key, self.row_of, self.keep = f32(n, 16), i32(n), i32(n), torch.empty(n, dtype=torch.uint8, device=dev)
        self.lists = [i32(n, 2), i32(n, 2), i32(n, 2), i64(n), f32(n, 2, 2), f32(n, 1), f32(n, 3), i64(n)]
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        self._project()
        self.perm = raster.stable_sort_keys(self.sort_key, key_bits=31)[1]
        g = torch.Generator(device=dev).manual_seed(1)
        self.upstream = [torch.randn(s, device=dev, generator=g) for s in ((n, 2, 2), (n, 1), (n, 3))]
        self.grads = [torch.empty_like(t) for t in self.params]
        self.forward()
        torch.cuda.synchronize()
        self.kept = int(self.keep.sum())
        fwd_io = nbytes(*self.params, self.record, self.sort_key, self.keep, self.row_of)
        gather_io = nbytes(self.perm, self.record, self.keep, *self.lists, self.row_of)
        self.bytes_fwd = (fwd_io + gather_io) / n
        self.bytes_bwd = nbytes(*self.params, self.row_of, *self.upstream, *self.grads) / n

    def _project(self):
        p = [t.data_ptr() for t in self.params + self.cam]
        out = [t.data_ptr() for t in (self.record, self.sort_key, self.keep, self.row_of)]
        nb = self.params[4].shape[1]
        if self.sh_entry:
            _lib.check(self.lib.gcp_project_forward_sh(*p, self.n, self.degree, nb, self.frame, *self.size, *out, self.stream), "forward")
        else:
            _lib.check(self.lib.gcp_project_forward(*p, self.n, self.degree, nb, *self.size, *out, self.stream), "forward")

    def forward(self):
        self._project()
        _lib.check(self.lib.gcp_project_gather(self.record.data_ptr(), self.perm.data_ptr(), self.n, *(t.data_ptr() for t in self.lists),
                                               self.row_of.data_ptr(), self.keep.data_ptr(), self.stream), "gather")

    def backward(self):
        p = [t.data_ptr() for t in self.params + self.cam]
        up, out = [t.data_ptr() for t in self.upstream], [t.data_ptr() for t in self.grads]
        nb = self.params[4].shape[1]
        if self.sh_entry:
            _lib.check(self.lib.gcp_project_backward_sh(*p, self.n, self.degree, nb, self.frame, self.row_of.data_ptr(), *up, None, *out,
                                                        self.stream), "backward")
        else:
            _lib.check(self.lib.gcp_project_backward(*p, self.n, self.degree, nb, self.row_of.data_ptr(), *up, *out, self.stream), "backward")


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--other-lib", default=None, help="a second build of the library to set the degree-2 camera-frame case against")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    width, height = 1920, 1080
    mean, q, scale, opacity = synthetic.make_world(a.gaussians, width, device=dev)
    P, K, _ = synthetic.ring_cameras(1, width, height, device=dev)
    color = 0.5 * torch.randn(a.gaussians, 16, 3, generator=torch.Generator().manual_seed(2)).to(dev)
    import math

    world = {"mean": mean, "variance_q": q, "variance_scale": scale, "opacity": opacity, "color": color, "P": P, "K": K, "width": width,
             "height": height, "tile_logit": math.log(0.04 / 0.96)}
    lib = _lib.load()
    cases = {"deg2_camera": Case(lib, world, 2, "camera", False), "deg2_world": Case(lib, world, 2, "world", True),
             "deg3_camera": Case(lib, world, 3, "camera", True), "deg3_world": Case(lib, world, 3, "world", True)}
    if a.other_lib:
        other = load_other(a.other_lib)
        cases["other_deg2_camera"] = Case(other, world, 2, "camera", False)
        cases["other_deg2_camera_again"] = Case(other, world, 2, "camera", False)
        order = ["other_deg2_camera", "deg2_camera", "other_deg2_camera_again", "deg2_world", "deg3_camera", "deg3_world"]
    else:
        order = list(cases)
    times = {k: {"fwd": [], "bwd": []} for k in order}
    for _ in range(a.rounds):  # alternating: drift of the shared host hits all alike
        for k in order:
            times[k]["fwd"].append(timeit(cases[k].forward))
            times[k]["bwd"].append(timeit(cases[k].backward))
    for k in order:
        c = cases[k]
        row = {"case": k, "gaussians": c.n, "kept": c.kept, "sh_degree": c.degree, "sh_frame": c.frame}
        for leg, per in (("fwd", c.bytes_fwd), ("bwd", c.bytes_bwd)):
            ms = median(times[k][leg])
            rate = per * c.n / (ms * 1e-3)
            row.update({f"{leg}_ms": round(ms, 4), f"{leg}_rounds_ms": [round(t, 4) for t in times[k][leg]], f"{leg}_bytes_per_gaussian": per,
                        f"{leg}_TBps": round(rate / 1e12, 3), f"{leg}_of_hbm_peak": round(rate / HBM_PEAK, 3)})
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
