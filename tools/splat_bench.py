"""Developer benchmark of the projection modes (csrc/gcp_project.hip, csrc/gcp_splat.hip): 10^6 Gaussians, one 1920x1080
camera, device events; per mode the projection forward + gather, its backward, one whole training step (min / median / max
over REPEATS after 5 warm-up rounds) and the splat-pixel pairs per frame — dilation enlarges every box, so the blend's share
of a step grows with the pair count, not with the kernels.

    python tools/splat_bench.py ROOT MODE [REPEATS]

ROOT: the checkout whose package is measured ("." or another commit's tree with its library built: run one process per
tree, alternating, to set this commit against its parent); MODE: default | subpixel (centres="subpixel", cov_dilation=0.3) |
antialias (subpixel plus antialias=True).
Prints one JSON line.  Results: profiles/r10_subpixel.md, profiles/r14_antialias.md."""
import json
import statistics
import sys

root, mode = sys.argv[1], sys.argv[2]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 30
sys.path.insert(0, root)
import torch  # noqa: E402

from simplegaussiansplat_tk71_amd import gs_model as gm  # noqa: E402
from simplegaussiansplat_tk71_amd.synthetic import make_world, ring_cameras  # noqa: E402

dev = torch.device("cuda", 0)
n, width, height = 1_000_000, 1920, 1080
P, K, wh = ring_cameras(1, width, height, device=dev)
mean, q, scale, op = make_world(n, width, sigma_px=2.0, seed=0, device=dev)
if mode not in ("default", "subpixel", "antialias"):
    sys.exit(f"MODE: default, subpixel or antialias, got {mode!r}")
opts = {} if mode == "default" else {"centres": "subpixel", "cov_dilation": 0.3}
if mode == "antialias":
    opts["antialias"] = True
model = gm.GS_model_with_param(mean, q, scale, op, **opts)
with torch.no_grad():
    model.color[:, 1:] = 0.1 * torch.randn_like(model.color[:, 1:])
target = torch.rand(1, 3, height, width, device=dev)
gen = torch.Generator(device=dev).manual_seed(1)


def timed(fn, sync_before=True):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


fwd, bwd, step = [], [], []
pairs = kept = None
for it in range(reps + 5):
    t_f, (cams, _, _) = timed(lambda: model.camera_inputs(P, K, wh))
    cam = cams[0]
    outs = [cam["variance_inverse"], cam["opacity"], cam["l_d"]] + ([cam["mean"]] if cam["mean"].is_floating_point() else [])
    ups = [torch.randn(o.shape, device=dev, generator=gen) for o in outs]
    t_b, _ = timed(lambda: torch.autograd.backward(outs, ups))
    model._optimizer.zero_grad()
    pairs, kept = int(cam["boxsize"].sum()), int(cam["index"].numel())
    del cams, cam, outs, ups

    def train():
        images, _, grad_iter = model(P, K, wh, [0])
        gm.splat_loss(images, target).backward()
        model.train_step()

    t_s, _ = timed(train)
    if it >= 5:
        fwd.append(t_f), bwd.append(t_b), step.append(t_s)
med = statistics.median
print(json.dumps({"root": root, "mode": mode, "kept": kept, "pairs_per_frame": pairs, "reps": reps,
                  "project_fwd_gather_ms": [round(min(fwd), 4), round(med(fwd), 4), round(max(fwd), 4)],
                  "project_bwd_ms": [round(min(bwd), 4), round(med(bwd), 4), round(max(bwd), 4)],
                  "train_step_ms": [round(min(step), 4), round(med(step), 4), round(max(step), 4)]}))
