#!/usr/bin/env python3
"""The reference's training loop on the HIP Function: 3-D Gaussians, posed cameras, L1 + D-SSIM, Adam with
per-parameter rates, densify / prune / opacity reset on the reference's schedule.

Shape of the reference's `Control.learning` (reference: gs_control.py:98-235) with its model replaced by
simplegaussiansplat_tk71_amd.gs_model.GS_model_with_param.  Two data sources:

    python examples/train_cameras.py                         # synthetic scene (the default; runs anywhere)
    python examples/train_cameras.py --colmap DIR            # DIR/sparse/0/{cameras,images,points3D}.bin + DIR/images/
    python examples/train_cameras.py --background random     # render over a random colour per step (or "1,1,1": white)
    python examples/train_cameras.py --sh-degree 3 --sh-frame world --sh-every 100 --save-ply scene.ply
                                                             # degree-3 colour on world-space directions, one degree more
                                                             # every 100 steps, saved as a standard 3DGS .ply
    python examples/train_cameras.py --load-ply scene.ply --sh-frame world      # resume from such a file
    python examples/train_cameras.py --centres subpixel --dilation 0.3 --clamp-colour
                                                             # float splat centres at px + 0.5 (their gradient trains the
                                                             # positions), 0.3 px^2 covariance dilation, colour clamped at 0
    python examples/train_cameras.py --centres subpixel --dilation 0.3 --antialias
                                                             # the same dilation with its opacity compensation: a Gaussian
                                                             # keeps the energy it had before the dilation (Mip-Splatting's 2-D filter)
    python examples/train_cameras.py --filter-3d --centres subpixel --dilation 0.1 --antialias
                                                             # full Mip-Splatting: the 3-D smoothing filter (a per-Gaussian low-pass
                                                             # from the training cameras' sampling rates, recomputed every
                                                             # --filter-every iterations) with the 2-D filter above
    python examples/train_cameras.py --centres subpixel --densify device --densify-on screen
                                                             # split / clone / prune in one pass of HIP kernels that keeps Adam's
                                                             # moments, decided on the screen-space gradient of the centres
    python examples/train_cameras.py --densify mcmc --cap-max 4000
                                                             # the MCMC strategy: dead Gaussians relocated onto live ones, 5 % more
                                                             # rows per pass up to the cap, position noise after every step
    python examples/train_cameras.py --prune-contribution 0.01 --prune-at 300,380
                                                             # at those iterations drop every Gaussian that paints less than 1 %
                                                             # of any pixel of any training camera (--prune-on sum: less than
                                                             # that many pixels in total), keeping Adam's moments
    python examples/train_cameras.py --densify mcmc --cap-max 4000 --adam sparse
                                                             # Adam only on the rows a camera of the batch saw, all five
                                                             # tensors in one launch (--adam fused: the same launch, every row)
    python examples/train_cameras.py --distortion-reg 100 --distortion-from 300
                                                             # from iteration 300 the loss gains 100 * the mean per-pixel depth
                                                             # distortion (Mip-NeRF 360 / 2DGS): pulls each ray's weights together
    python examples/train_cameras.py --normal-reg 0.05 --normal-from 300
                                                             # from iteration 300 the loss gains 0.05 * 2DGS's normal consistency:
                                                             # the blended normals against the normals of the rendered depth
    python examples/train_cameras.py --colmap DIR --exposure --save-exposure exposure.json
                                                             # one learned 3 x 4 colour affine per training photograph, applied
                                                             # to the render inside the loss kernels (upstream 3DGS's exposure
                                                             # compensation), written as image name -> matrix
    python examples/train_cameras.py --colmap DIR --undistort
                                                             # the photographs resampled on the device, once, into the pinhole
                                                             # cameras fitted to their lenses (what `colmap image_undistorter`
                                                             # does for upstream 3DGS); K is then the fitted cameras'
    python examples/train_cameras.py --test-every 8 --eval-every 100 --eval-json eval.json
                                                             # hold out every 8th camera (sorted by name, the llffhold convention),
                                                             # report PSNR / SSIM / L1 on them every 100 iterations and at the end
    python examples/train_cameras.py --colmap DIR --init-scale knn
                                                             # the initial scales from the exact nearest neighbours of the HIP
                                                             # kernel (3dgs: upstream's rule) instead of torch.cdist + topk

The reference's own checkout cannot be trained on: its images.bin (camera poses) is missing, so the synthetic
scene renders its target images from a hidden set of Gaussians seen by a ring of cameras and then fits a
perturbed, colour-less copy of them — the same situation as starting from a COLMAP point cloud.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplegaussiansplat_tk71_amd import gs_model as gm  # noqa: E402
from simplegaussiansplat_tk71_amd.synthetic import ring_cameras  # noqa: E402

INIT_SCALES = ("cdist", "knn", "3dgs")  # --init-scale


def synthetic_scene(n_gauss, n_cam, width, height, seed, device, with_alpha=False):
    """-> (start, P, K, wh, targets) [+ the targets' alpha maps (n_cam, 1, H, W) with_alpha: to composite them over the
    background a step renders on]"""
    g = torch.Generator().manual_seed(seed)
    truth = {
        "mean": 0.6 * torch.randn(n_gauss, 3, generator=g),
        "variance_q": torch.randn(n_gauss, 4, generator=g),
        "variance_scale": torch.log(0.03 + 0.06 * torch.rand(n_gauss, 3, generator=g)),
        "opacity": torch.logit(0.3 + 0.6 * torch.rand(n_gauss, 1, generator=g)),
    }
    color = torch.zeros(n_gauss, 9, 3)
    color[:, 0, :] = torch.rand(n_gauss, 3, generator=g) / 0.28209479177387814
    color[:, 1:4, :] = 0.3 * torch.randn(n_gauss, 3, 3, generator=g)
    truth = {k: v.to(device) for k, v in truth.items()}
    P, K, wh = ring_cameras(n_cam, width, height, device=device)
    hidden = gm.GS_model_with_param(truth["mean"], truth["variance_q"], truth["variance_scale"], truth["opacity"])
    with torch.no_grad():
        hidden.color.copy_(color.to(device))
        if with_alpha:
            shots = [hidden.render(P[i:i + 1], K[i:i + 1], wh[i:i + 1]) for i in range(n_cam)]
            targets = torch.cat([s[0] for s in shots]).clamp(0, 1)
            alphas = torch.cat([s[2] for s in shots])
        else:
            targets = torch.cat([hidden(P[i:i + 1], K[i:i + 1], wh[i:i + 1], ["t"])[0] for i in range(n_cam)]).clamp(0, 1)
    start = truth["mean"] + 0.02 * torch.randn(n_gauss, 3, generator=g).to(device)  # a noisy point cloud
    return (start, P, K, wh, targets, alphas) if with_alpha else (start, P, K, wh, targets)


def load_colmap(root, device, with_names=False, undistort=False):
    """-> (xyz, P, K, wh, photographs (C, 3, H, W) in 0..1) [+ the image names with_names: what `split_cameras` sorts by]
    `undistort`: the photographs are uploaded as the bytes they decode to, one pinhole camera is fitted per image to its
    camera's lens (`gs_model.fit_pinhole`: the source's size and principal point, the widest field of view without a blank
    pixel), `gs_model.undistort` resamples them all in one HIP launch, and K is the fitted cameras' instead of the file's.
    Every photograph is treated so, whether it is trained on or held out: they are photographs through the same lenses."""
    from PIL import Image

    from simplegaussiansplat_tk71_amd import colmap_io

    xyz, P, K, wh, names, *lenses = colmap_io.load_colmap_tensors(os.path.join(root, "sparse", "0"), device=device, lenses=undistort)
    imgs = [torch.from_numpy(np.array(Image.open(os.path.join(root, "images", n)).convert("RGB"))) for n in names]
    if undistort:
        K_out = torch.stack([gm.fit_pinhole(lens)[0] for lens in lenses[0]])
        photos = gm.undistort(torch.stack(imgs).to(device), lenses[0], K_out)
        K = K_out.to(device=device, dtype=torch.float32)
    else:
        photos = (torch.stack([i.permute(2, 0, 1) for i in imgs]).float() / 255).to(device)
    return (xyz, P, K, wh, photos, list(names)) if with_names else (xyz, P, K, wh, photos)


def train(start, P, K, wh, targets, iterations=300, batch_size=3, loss_lamda=0.2, opacity_init=0.1, neighbours=3,
          densify_from_iter=500, densify_until_iter=15000, densification_interval=100, opacity_reset_interval=3000,
          reset_opacity_min=0.01, seed=0, log=print, rank=0, world=1, background=None, target_alpha=None, sh_degree=2,
          sh_frame="camera", sh_every=0, save_ply=None, load_ply=None, centres="pixel", dilation=None, clamp_colour=False,
          densify="reference", densify_on="position", antialias=False, cap_max=None, noise_lr=5e5, opacity_reg=0.01, scale_reg=0.01,
          prune_contribution=None, prune_at=(), prune_on="max", adam="tensor", test_every=0, eval_every=0, evals=None, names=None,
          screen_grad="signed", distortion_reg=0.0, distortion_from=0, filter_3d=False, filter_every=100, exposure=False,
          exposure_lr_init=0.01, exposure_lr_final=0.001, save_exposure=None, normal_reg=0.0, normal_from=7000, save_mesh=None, mesh_resolution=256,
          mesh_trunc=None, normal_depth="expected", mesh_depth="expected", init_scale="cdist", mesh_keep=None, mesh_min_faces=None,
          mesh_normals=False):
    """`world` > 1: one process per GPU under torch.distributed; every rank holds the whole scene, renders
    `batch[rank::world]` and the gradients are all-reduced (GS_model_with_param.allreduce_grads).
    `background`: None (black, the default), a fixed (r, g, b), or "random" — a new colour per step (drawn from torch's
    generator: the same on every rank); the images are then rendered over it (GS_model_with_param.render) and, where
    `target_alpha` (B, 1, H, W) is given, the targets composited over it too.
    `sh_degree` (0..3) and `sh_frame` ("camera" / "world"): the appearance model (gs_model.camera_inputs); `sh_every` N > 0:
    start at degree 0 and activate one more every N iterations.  `load_ply`: start from that scene file instead of `start`
    (its degree replaces `sh_degree`); `save_ply`: write the trained scene there (rank 0).
    `centres`, `dilation`, `clamp_colour`, `antialias`: the projection's `centres`, `cov_dilation`, `clamp_colour`, `antialias`
    (gs_model.camera_inputs); `antialias` needs a `dilation` > 0.
    `densify`: "reference" (the default: `densify_and_prune` / `reset_opacity`, which rebuild Adam without its moments, split
    samples from torch's generator) or "device" (`densify_and_prune_device` with seed + iteration and
    `reset_opacity(keep_optimizer=True)`: one pass of HIP kernels, Adam's state kept, the statistic summed over the ranks
    first) or "mcmc" (3DGS-MCMC: the loss gains opacity_reg * mean sigmoid(opacity) + scale_reg * mean exp(variance_scale),
    `add_position_noise(seed + iteration, noise_lr)` follows every optimiser step, and on the densification schedule
    `relocate_and_grow_device(seed + iteration, cap_max)` relocates the dead Gaussians and grows the scene by 5 % up to
    `cap_max` (None: no growth); no opacity reset and no statistic: every rank draws the same samples from the same
    parameters).  `densify_on`: the statistic the device path decides on, "position" or "screen" (GS_model_with_param).
    `screen_grad`: what the "screen" statistic takes the norm of, "signed" (the default) or "abs" — the per-pixel absolute
    gradients of the centre summed per component (AbsGS; gsplat's absgrad), which does not cancel over a large splat; the
    optimiser steps are those of "signed" bit for bit.  The densification threshold (the model's `grad_threshold`) is not
    tuned for this statistic here either: no full-length run on real poses exists.  As a pointer, not a default: trainers
    that switch to absolute gradients raise theirs by a factor of about four (gsplat: 2e-4 -> 8e-4).
    `prune_contribution` T with `prune_at` (iterations) and `prune_on` ("max" / "sum"): at those iterations, after the optimiser
    step, every rank measures its share of ALL cameras (`model.contribution`, `batch_size` at a time), the measurements are
    all-reduced, and `model.prune_by_contribution(stats, T, prune_on)` drops the Gaussians below T with Adam's state kept;
    works with every `densify`.
    `adam`: the optimiser step (GS_model_with_param): "tensor" (the default), "fused" (one call for all tensors, step counts
    and rates on the device) or "sparse" (the fused call restricted to the rows some camera of the batch saw on some rank,
    `grad_iter`; the other rows keep parameters and moments).  Under densify="mcmc" the two regularisers give EVERY row a
    gradient, and "sparse" does not apply it to the rows no camera saw, as the sparse Adam of other 3DGS trainers.
    `test_every` N > 0: the cameras are sorted by `names` (default: their index) and every N-th of that order, from the first,
    is held out (`gs_model.split_cameras`, the llffhold convention): it never enters a batch, the camera extent or a
    contribution pass, and the run takes exactly the steps of a run that was given the training cameras alone.  Every
    `eval_every` iterations (0: never) and always after the last step, rank r measures `test[r::world]`
    (`model.evaluate`: clamped render, per-image PSNR / SSIM / L1 in one HIP pass; over the fixed `background` if there is one,
    over black under "random" — no colour is drawn for it), `gs_model.gather_metrics` collects the ranks' shares, and rank 0
    logs the means and appends to the list `evals` a record {"iteration", "split": "test", "views", "gaussians", "psnr",
    "ssim", "l1", "per_image": {name: {"psnr", "ssim", "l1"}}}, psnr / ssim / l1 being the means of the per-image values.
    `distortion_reg` L > 0: from iteration `distortion_from` on, the step renders through `model.render(distortion=True)` (over
    black where no `background` is set) and the loss gains L * mean(distortion map) — the depth distortion loss of Mip-NeRF 360 /
    2DGS (`cuda_kernel.render`), in units of camera-space depth; the weight is not tuned here.  With L = 0 (the default) no
    step changes.
    `filter_3d`: Mip-Splatting's 3-D smoothing filter (GS_model_with_param(filter_3d=True)): `model.update_filter_3d` on ALL
    training cameras (every rank passes them all: no collective) before the first step, every `filter_every` iterations and
    right after every densify / relocate / prune pass; the saved .ply holds the filtered scales and opacities.  The held-out
    cameras never enter it.  100 iterations and the filter's variance 0.2 are the published values, not tuned here.
    `exposure`: per-camera exposure compensation (`gs_model.CameraExposure`): one 3 x 4 colour affine per TRAINING camera,
    initialised to the identity, applied to the render inside the loss kernels (`splat_loss(exposure=)`) and trained by an Adam
    group of its own on the rows of the cameras a step drew (`exposure_lr_init` -> `exposure_lr_final` over 30 000 steps: the
    published rates of upstream 3DGS, not tuned here); under `world` > 1 its gradient is summed and the drawn cameras OR-ed over
    the ranks first.  The held-out cameras have no learned exposure: they are evaluated with the identity, and every eval
    record then says "exposure": "identity".  `save_exposure`: write the matrices there as one JSON object, image name ->
    3 x 4 list (rank 0).  Scene brightness times exposure gain is not pinned (as upstream) and no regulariser is added.  With
    exposure=False (the default) no step changes.
    `normal_reg` L > 0: from iteration `normal_from` on, the step renders through `model.render(normals=True)` (over black where
    no `background` is set) and the loss gains L * `gs_model.normal_consistency(depth, alpha, normal, K)` of this rank's share —
    2DGS's normal-consistency loss, the blended per-Gaussian normals against the normals of the rendered depth surface, with
    the K of the cameras the step drew (under --undistort the fitted cameras').  2DGS trains with L = 0.05 from iteration 7000;
    that is a pointer, not a tuned value: no full-length run on real poses exists here.  With L = 0 (the default) no step
    changes.
    `save_mesh`: after the last step rank 0 fuses the depth maps of the TRAINING cameras into a TSDF volume and writes its zero
    level set there as a triangle mesh (`model.extract_mesh(P, K, wh, resolution=mesh_resolution, trunc=mesh_trunc)`,
    `ply_io.save_mesh`; `batch_size` cameras at a time; a running mean is order-dependent, so the ranks do not share the work).
    `mesh_resolution` = 256 and the default truncation of 5 voxels are pointers from 2DGS's usage, not tuned here.  With
    save_mesh=None (the default) no step and no output changes.
    `mesh_keep` / `mesh_min_faces`: with either given (the other then defaults to 50) the mesh is cleaned before it is written:
    `model.extract_mesh(keep_largest=, min_faces=)`, 2DGS's post_process_mesh rule — 50 / 50 are its values, pointers and not
    tuned here.  `mesh_normals`: the file carries `mesh.vertex_normals` of what is written (`nx ny nz`).  All three are ignored
    without save_mesh; with none of them the file is what it was.
    `normal_depth` / `mesh_depth` "median": the depth surface of the normal term / the fused depth is the median depth map
    (`model.render(median=True)` through `gs_model.median_as_depth`; `model.extract_mesh(depth="median")`) instead of the
    expected depth — 2DGS's depth_ratio = 1 for bounded scenes, a pointer and not a tuned choice.  With "expected" (the
    default) no step and no output changes.
    `init_scale`: where the initial scales come from.  "cdist" (the default): `gs_model.mean_neighbour_distance(neighbours,
    start)`, the reference's torch.cdist + topk — quadratic in the cloud, and cancelled where the cloud lies far from its origin.
    "knn": the same definition from the exact neighbours of the HIP kernel (`gs_model.neighbour_scale(start, "reference",
    neighbours)`).  "3dgs": upstream 3DGS's rule, the root of the mean of the 3 smallest squared distances (`neighbours` is
    ignored).  With "cdist" no step changes.
    Evaluation touches no gradient, statistic, optimiser state or generator.  LPIPS is not reported: it needs pretrained
    network weights.  The return value stays (model, losses)."""
    if adam not in gm.ADAM_MODES:
        raise ValueError(f"adam: 'tensor', 'fused' or 'sparse', got {adam!r}")
    if densify not in ("reference", "device", "mcmc"):
        raise ValueError(f"densify: 'reference', 'device' or 'mcmc', got {densify!r}")
    if prune_on not in ("max", "sum"):
        raise ValueError(f"prune_on: 'max' or 'sum', got {prune_on!r}")
    if init_scale not in INIT_SCALES:
        raise ValueError(f"init_scale: 'cdist', 'knn' or '3dgs', got {init_scale!r}")
    if isinstance(background, str) and background != "random":
        raise ValueError(f"background: None, (r, g, b) or 'random', got {background!r}")
    dev = start.device
    held = None
    train_names = None if names is None else [str(n) for n in names]
    if test_every:
        names = [f"{i:06d}" for i in range(P.shape[0])] if names is None else list(names)
        if len(names) != P.shape[0]:
            raise ValueError(f"names: {len(names)} entries for {P.shape[0]} cameras")
        train_idx, test_idx = gm.split_cameras(names, test_every)
        if not train_idx:
            raise ValueError(f"test_every={test_every} holds out every camera: nothing is left to train on")
        keep, out = torch.tensor(train_idx, device=dev), torch.tensor(test_idx, device=dev)
        held = {"P": P[out], "K": K[out], "wh": wh[out], "targets": targets[out], "names": [str(names[i]) for i in test_idx]}
        if isinstance(background, tuple) or isinstance(background, list):
            held["background"] = torch.as_tensor(background, dtype=torch.float32, device=dev)
            if target_alpha is not None:
                held["targets"] = held["targets"] + (1 - target_alpha[out]) * held["background"][None, :, None, None]
        P, K, wh, targets = P[keep], K[keep], wh[keep], targets[keep]
        train_names = [str(names[i]) for i in train_idx]
        target_alpha = None if target_alpha is None else target_alpha[keep]

    def evaluate_held_out():
        """One record of the held-out cameras; every rank measures its share, rank 0 reports."""
        n_test = len(held["names"])
        mine = torch.arange(n_test, device=dev)[rank::world]
        m = model.evaluate(held["P"][mine], held["K"][mine], held["wh"][mine], held["targets"][mine],
                           background=held.get("background"), batch_size=batch_size)
        if world > 1:
            m = gm.gather_metrics(m, mine, n_test)
        if rank != 0:
            return
        psnr, ssim, l1 = (t.tolist() for t in (m.psnr, m.ssim, m.l1))
        log(f"iter {iteration:5d}  test PSNR {np.mean(psnr):.3f}  SSIM {np.mean(ssim):.4f}  L1 {np.mean(l1):.5f}  ({n_test} views)")
        if evals is not None:
            evals.append({"iteration": iteration, "split": "test", "views": n_test, "gaussians": int(model.mean.shape[0]),
                          "psnr": float(np.mean(psnr)), "ssim": float(np.mean(ssim)), "l1": float(np.mean(l1)),
                          "per_image": {name: {"psnr": p, "ssim": s, "l1": e} for name, p, s, e in zip(held["names"], psnr, ssim, l1)}})
            if ce is not None:  # no exposure is learned for a held-out camera
                evals[-1]["exposure"] = "identity"

    torch.manual_seed(seed)  # densification draws samples: every rank must draw the same ones
    n = start.shape[0]
    q = torch.zeros((n, 4), device=dev)
    q[:, 3] = 1  # identity rotation, (x, y, z, w) (gs_control.py:113-114)
    if init_scale == "cdist":
        scale = torch.log(gm.mean_neighbour_distance(neighbours, start))
    else:
        scale = torch.log(gm.neighbour_scale(start, "reference" if init_scale == "knn" else "3dgs", neighbours))
    opacity = torch.full((n, 1), math.log(opacity_init / (1 - opacity_init)), device=dev)
    sh = {"sh_frame": sh_frame, "active_sh_degree": 0 if sh_every else None, "centres": centres, "cov_dilation": dilation,
          "clamp_colour": clamp_colour}
    if adam != "tensor":
        sh["adam"] = adam
    if antialias:
        sh["antialias"] = antialias
    if densify_on != "position":
        sh["densify_on"] = densify_on
    if screen_grad != "signed":
        sh["screen_grad"] = screen_grad
    if filter_3d:
        sh["filter_3d"] = True
    if load_ply is not None:
        model = gm.GS_model_with_param.from_ply(load_ply, dev, **sh)
    else:
        model = gm.GS_model_with_param(start.clone(), q, scale, opacity, L_max=sh_degree, **sh)
    ce = None
    if exposure:
        ce = gm.CameraExposure(P.shape[0], names=train_names, device=dev, lr_init=exposure_lr_init, lr_final=exposure_lr_final)
    data = gm.GS_dataset(P, K, wh, list(range(P.shape[0])))
    extent = data.get_camera_extent()
    gen = torch.Generator().manual_seed(seed)
    losses, iteration, t0 = [], 0, time.time()
    if filter_3d:
        model.update_filter_3d(P, K, wh)
    while iteration < iterations:
        order = torch.randperm(len(data), generator=gen)
        for b in range(0, len(order), batch_size):
            idx = order[b:b + batch_size].to(dev)
            mine = idx[rank::world]
            if mine.numel():
                distort = distortion_reg > 0 and iteration >= distortion_from
                with_normals = normal_reg > 0 and iteration >= normal_from
                with_median = with_normals and normal_depth == "median"
                dist = nmaps = None
                if background is None and not distort and not with_normals:
                    images, kept, grad_iter = model(P[mine], K[mine], wh[mine], mine.tolist())
                    target = targets[torch.tensor(kept, device=dev)]
                else:
                    bg = None
                    if background is not None:
                        bg = torch.rand(3, device=dev) if isinstance(background, str) else torch.as_tensor(background, dtype=torch.float32,
                                                                                                              device=dev)
                    images, *maps, kept, grad_iter = model.render(P[mine], K[mine], wh[mine], background=bg, image_sample=mine.tolist(),
                                                                  distortion=distort, **({"normals": True} if with_normals else {}),
                                                                  **({"median": True} if with_median else {}))
                    dist = maps[2] if distort else None
                    sel = torch.tensor(kept, device=dev)
                    if with_median:  # the depth surface from the median map; the blended normals as before
                        nmaps = (*gm.median_as_depth(maps[-1], maps[1]), maps[-2], K[sel])
                    elif with_normals:
                        nmaps = (maps[0], maps[1], maps[-1], K[sel])
                    target = targets[sel]
                    if bg is not None and target_alpha is not None:
                        target = target + (1 - target_alpha[sel]) * bg[None, :, None, None]
                if ce is None:
                    loss = gm.splat_loss(images, target, loss_lamda) * (mine.numel() / idx.numel())
                else:
                    loss = gm.splat_loss(images, target, loss_lamda, exposure=ce.rows(kept)) * (mine.numel() / idx.numel())
                if dist is not None:  # the geometric regulariser: the mean per-pixel depth distortion of this rank's share
                    loss = loss + distortion_reg * dist.mean() * (mine.numel() / idx.numel())
                if nmaps is not None:  # the blended normals against the normals of the rendered depth surface
                    loss = loss + normal_reg * gm.normal_consistency(*nmaps) * (mine.numel() / idx.numel())
                if densify == "mcmc":  # the regularisers that let opacities die and keep scales small; the whole term on every rank's share
                    loss = loss + (opacity_reg * torch.sigmoid(model.opacity).mean()
                                   + scale_reg * torch.exp(model.variance_scale).mean()) * (mine.numel() / idx.numel())
                loss.backward()
            else:  # more ranks than cameras in this batch
                kept = []
                loss, grad_iter = torch.zeros((), device=dev), torch.zeros(model.mean.shape[0], dtype=torch.bool, device=dev)
            if world > 1:
                grad_iter = model.allreduce_grads(grad_iter)
                loss = loss.detach().clone()  # the batch loss, for the log only
                if torch.distributed.get_backend() == "gloo":
                    host = loss.cpu()
                    torch.distributed.all_reduce(host)
                    loss = host.to(dev)
                else:
                    torch.distributed.all_reduce(loss)
            model.param_iter_update(grad_iter)
            model.train_step(visible=grad_iter)
            if ce is not None:
                drawn = ce.allreduce_grads(kept) if world > 1 else kept
                ce.set_lr(iteration)
                ce.step(drawn)
            if densify == "mcmc":
                model.add_position_noise(seed + iteration, noise_lr)
            iteration += 1
            losses.append(float(loss.detach()))
            model.set_mean_lr(iteration)
            if sh_every and iteration % sh_every == 0:
                model.oneup_sh_degree()
            if prune_contribution is not None and iteration in prune_at:
                stats = None
                share = torch.arange(len(data), device=dev)[rank::world]
                for c in range(0, share.numel(), batch_size):
                    part = share[c:c + batch_size]
                    stats = model.contribution(P[part], K[part], wh[part], stats)
                if stats is None:  # more ranks than cameras: this rank measured nothing
                    n_rows = model.mean.shape[0]
                    stats = (torch.zeros(n_rows, device=dev), torch.zeros(n_rows, device=dev), torch.zeros(n_rows, dtype=torch.int32, device=dev))
                if world > 1:
                    gm.allreduce_contribution(stats)
                n_before, n_after = model.prune_by_contribution(stats, prune_contribution, prune_on)
                log(f"iter {iteration:5d}  pruned by contribution (w_{prune_on} < {prune_contribution:g}): Gaussians {n_before} -> {n_after}")
                if filter_3d:
                    model.update_filter_3d(P, K, wh)
            if densify_from_iter <= iteration <= densify_until_iter and iteration % densification_interval == 0:
                if densify == "mcmc":
                    model.relocate_and_grow_device(seed + iteration, cap_max)
                elif densify == "device":
                    if world > 1:
                        model.allreduce_density_stats()
                    model.densify_and_prune_device(extent, seed=seed + iteration)
                else:
                    model.densify_and_prune(extent)
                if filter_3d:
                    model.update_filter_3d(P, K, wh)
            elif filter_3d and iteration % max(1, filter_every) == 0:
                model.update_filter_3d(P, K, wh)
            if opacity_reset_interval and iteration % opacity_reset_interval == 0 and densify != "mcmc":
                if densify == "device":
                    model.reset_opacity(reset_opacity_min, keep_optimizer=True)
                else:
                    model.reset_opacity(reset_opacity_min)
            if iteration % max(1, iterations // 10) == 0 or iteration == iterations:
                log(f"iter {iteration:5d}  loss {np.mean(losses[-20:]):.5f}  Gaussians {model.mean.shape[0]}")
            if held is not None and eval_every and iteration % eval_every == 0 and iteration < iterations:
                evaluate_held_out()
            if iteration >= iterations:
                break
    if held is not None:
        evaluate_held_out()  # always after the last step
    if dev.type == "cuda":
        torch.cuda.synchronize()
    log(f"{iteration} iterations in {time.time() - t0:.1f} s")
    if save_ply is not None and rank == 0:
        model.save_ply(save_ply)
    if ce is not None and save_exposure is not None and rank == 0:
        ce.save_json(save_exposure)
    if save_mesh is not None and rank == 0:
        from simplegaussiansplat_tk71_amd import ply_io

        options = {"depth": "median"} if mesh_depth == "median" else {}
        if mesh_keep is not None or mesh_min_faces is not None:
            options.update(keep_largest=mesh_keep, min_faces=mesh_min_faces)
        if mesh_normals:
            options["normals"] = True
        vertices, faces, colours, *normals = model.extract_mesh(P, K, wh, resolution=mesh_resolution, trunc=mesh_trunc, batch_size=batch_size,
                                                                **options)
        ply_io.save_mesh(save_mesh, vertices, faces, colours, *normals)
        log(f"mesh: {vertices.shape[0]} vertices, {faces.shape[0]} faces -> {save_mesh}")
    return model, losses


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--colmap", default=None, help="COLMAP root (sparse/0/*.bin + images/); default: synthetic scene")
    ap.add_argument("--undistort", action="store_true",
                    help="with --colmap: resample every photograph through its camera's lens distortion into a fitted pinhole camera "
                         "(one HIP launch) and train on those; default: the distortion terms of cameras.bin are ignored")
    ap.add_argument("--gaussians", type=int, default=3000)
    ap.add_argument("--cameras", type=int, default=12)
    ap.add_argument("--width", type=int, default=160)
    ap.add_argument("--height", type=int, default=120)
    ap.add_argument("--iterations", type=int, default=400)
    ap.add_argument("--densify-from", type=int, default=500)
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend under torchrun (nccl = RCCL; gloo to rehearse on one GPU)")
    ap.add_argument("--background", default=None, help='"random" (a colour per step) or "r,g,b"; default: black')
    ap.add_argument("--sh-degree", type=int, choices=(0, 1, 2, 3), default=2, help="SH degree of the colour")
    ap.add_argument("--sh-frame", choices=("camera", "world"), default="camera",
                    help="directions the SH basis is evaluated on; world = the convention of other 3DGS renderers")
    ap.add_argument("--sh-every", type=int, default=0, metavar="N", help="start at degree 0, one degree more every N iterations (0: off)")
    ap.add_argument("--save-ply", default=None, metavar="PATH", help="write the trained scene as a standard 3DGS .ply")
    ap.add_argument("--load-ply", default=None, metavar="PATH", help="start from a 3DGS .ply instead of the point cloud")
    ap.add_argument("--centres", choices=("pixel", "subpixel"), default="pixel",
                    help="subpixel = float splat centres at px + 0.5, trained by their own gradient; pixel = truncated (the reference's)")
    ap.add_argument("--dilation", type=float, default=None, metavar="F",
                    help="added to the diagonal of the pixel covariance (0.3: other 3DGS renderers'; default 1e-6)")
    ap.add_argument("--clamp-colour", action="store_true", help="clamp the SH colour at 0")
    ap.add_argument("--antialias", action="store_true",
                    help="scale each opacity by sqrt(det Sigma / det Sigma'), the energy the dilation adds (needs --dilation > 0)")
    ap.add_argument("--densify", choices=("reference", "device", "mcmc"), default="reference",
                    help="device = split / clone / prune in one pass of HIP kernels that keeps Adam's moments; reference = the reference's; "
                         "mcmc = relocate dead Gaussians, grow to --cap-max, position noise after every step (3DGS-MCMC)")
    ap.add_argument("--cap-max", type=int, default=None, metavar="N", help="--densify mcmc: grow by 5 %% per pass up to N Gaussians (default: no growth)")
    ap.add_argument("--noise-lr", type=float, default=5e5, help="--densify mcmc: the position noise is lr_mean * this * gate * Sigma z")
    ap.add_argument("--opacity-reg", type=float, default=0.01, help="--densify mcmc: weight of mean sigmoid(opacity) in the loss")
    ap.add_argument("--scale-reg", type=float, default=0.01, help="--densify mcmc: weight of mean exp(variance_scale) in the loss")
    ap.add_argument("--prune-contribution", type=float, default=None, metavar="T",
                    help="at the --prune-at iterations drop the Gaussians whose contribution to the training images is below T "
                         "(0.01: RadSplat's value for --prune-on max; not tuned here)")
    ap.add_argument("--prune-at", default="", metavar="I[,I...]", help="iterations at which --prune-contribution runs")
    ap.add_argument("--prune-on", choices=("max", "sum"), default="max",
                    help="max = the largest colour weight T*o*g over every pixel of every camera; sum = their sum")
    ap.add_argument("--adam", choices=("tensor", "fused", "sparse"), default="tensor",
                    help="tensor = one Adam kernel per parameter tensor; fused = one call for all of them, step counts and rates on the "
                         "device; sparse = the fused call on the rows some camera of the batch saw, the others keep parameters and moments "
                         "(under --densify mcmc the opacity and scale regularisers give every row a gradient: unseen rows are not moved by it)")
    ap.add_argument("--densify-on", choices=("position", "screen"), default="position",
                    help="statistic of --densify device: screen = gradient of the 2-D centres per view (needs --centres subpixel)")
    ap.add_argument("--screen-grad", choices=("signed", "abs"), default="signed",
                    help="with --densify-on screen: abs = per-pixel absolute gradients of the centre summed per component (AbsGS), "
                         "which do not cancel over a large splat; the threshold is not tuned for it")
    ap.add_argument("--test-every", type=int, default=0, metavar="N",
                    help="hold out every N-th camera of the name-sorted order, from the first (8: the Mip-NeRF 360 / 3DGS convention; 0: train on all)")
    ap.add_argument("--eval-every", type=int, default=0, metavar="I",
                    help="with --test-every: PSNR / SSIM / L1 on the held-out cameras every I iterations (0: only after the last step)")
    ap.add_argument("--eval-json", default=None, metavar="PATH", help="write the evaluation records (rank 0) as a JSON list")
    ap.add_argument("--distortion-reg", type=float, default=0.0, metavar="L",
                    help="weight of the mean per-pixel depth distortion (Mip-NeRF 360 / 2DGS) in the loss (0: off; not tuned here)")
    ap.add_argument("--distortion-from", type=int, default=0, metavar="I", help="with --distortion-reg: the first iteration that carries the term")
    ap.add_argument("--normal-reg", type=float, default=0.0, metavar="L",
                    help="weight of 2DGS's normal-consistency loss, the blended normals against the normals of the rendered depth "
                         "(0: off; 2DGS uses 0.05; not tuned here)")
    ap.add_argument("--normal-from", type=int, default=7000, metavar="I",
                    help="with --normal-reg: the first iteration that carries the term (7000 is 2DGS's; not tuned here)")
    ap.add_argument("--filter-3d", action="store_true",
                    help="Mip-Splatting's 3-D smoothing filter: every Gaussian low-pass filtered in world space by the highest rate a training "
                         "camera samples it at, its mass kept; full Mip-Splatting is --filter-3d --centres subpixel --dilation 0.1 --antialias")
    ap.add_argument("--filter-every", type=int, default=100, metavar="N",
                    help="with --filter-3d: recompute the filter every N iterations (and after every densify / relocate / prune pass); "
                         "100 is the published cadence, not tuned here")
    ap.add_argument("--exposure", action="store_true",
                    help="learn one 3 x 4 colour affine per training camera, applied to the render inside the loss kernels "
                         "(upstream 3DGS's exposure compensation); held-out cameras are evaluated with the identity")
    ap.add_argument("--exposure-lr-init", type=float, default=0.01, help="with --exposure: the first learning rate (upstream's, not tuned here)")
    ap.add_argument("--exposure-lr-final", type=float, default=0.001, help="with --exposure: the rate after 30 000 steps (upstream's)")
    ap.add_argument("--save-exposure", default=None, metavar="PATH", help="with --exposure: write the matrices as JSON, image name -> 3 x 4 list")
    ap.add_argument("--normal-depth", choices=("expected", "median"), default="expected",
                    help="with --normal-reg: the depth whose surface normals the blended normals are held against: the expected depth "
                         "sum w z / alpha, or the median depth, the layer at which the transmittance falls through 1/2 (2DGS's "
                         "depth_ratio = 1 for bounded scenes: a pointer, not a tuned choice)")
    ap.add_argument("--mesh-depth", choices=("expected", "median"), default="expected",
                    help="with --save-mesh: the depth map that is fused, as for --normal-depth (2DGS's depth_ratio = 1 fuses the "
                         "median depth of bounded scenes: a pointer, not a tuned choice)")
    ap.add_argument("--init-scale", choices=INIT_SCALES, default="cdist",
                    help="the initial scales: cdist = the reference's torch.cdist + topk (quadratic, cancelled far from the origin); "
                         "knn = the same definition from the exact nearest neighbours of the HIP kernel; 3dgs = upstream 3DGS's "
                         "root of the mean of the 3 smallest squared distances")
    ap.add_argument("--save-mesh", default=None, metavar="PATH",
                    help="after the last step: fuse the training cameras' depth maps into a TSDF volume and write its surface as a "
                         "triangle mesh .ply (rank 0); what --normal-reg and --distortion-reg shape the depth for")
    ap.add_argument("--mesh-resolution", type=int, default=256, metavar="N",
                    help="with --save-mesh: voxels along the scene cube's side (256: a pointer from 2DGS's usage, not tuned here)")
    ap.add_argument("--mesh-trunc", type=float, default=None, metavar="F",
                    help="with --save-mesh: the truncation distance in world units (default: 5 voxels; not tuned here)")
    ap.add_argument("--mesh-keep", type=int, default=None, metavar="N",
                    help="with --save-mesh: clean the mesh, keeping the N connected components with the most faces (ties all stay); "
                         "if only --mesh-min-faces is given, 50: 2DGS's post_process_mesh value, a pointer and not tuned here")
    ap.add_argument("--mesh-min-faces", type=int, default=None, metavar="M",
                    help="with --save-mesh: clean the mesh, dropping components of fewer than M faces; if only --mesh-keep is given, "
                         "50: 2DGS's value, a pointer and not tuned here")
    ap.add_argument("--mesh-normals", action="store_true",
                    help="with --save-mesh: write area-weighted vertex normals (nx ny nz), computed after the cleaning")
    return ap


if __name__ == "__main__":
    ap = build_parser()
    a = ap.parse_args()
    if (a.eval_every or a.eval_json) and not a.test_every:
        ap.error("--eval-every and --eval-json need --test-every N with N > 0")
    if a.undistort and not a.colmap:
        ap.error("--undistort needs --colmap DIR")
    if a.save_exposure and not a.exposure:
        ap.error("--save-exposure needs --exposure")
    if a.antialias and not (a.dilation is not None and a.dilation > 0):
        ap.error("--antialias requires --dilation F with F > 0")
    prune_at = tuple(int(v) for v in a.prune_at.split(",") if v)
    if (a.prune_contribution is None) != (not prune_at):
        ap.error("--prune-contribution T and --prune-at I[,I...] go together")
    background = a.background if a.background in (None, "random") else tuple(float(v) for v in a.background.split(","))
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)) % max(1, torch.cuda.device_count()))
    torch.cuda.set_device(device)
    if world > 1:  # python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 examples/train_cameras.py
        if a.backend == "nccl":
            torch.distributed.init_process_group("nccl", device_id=device)
        else:
            torch.distributed.init_process_group(a.backend)
    alphas, names, evals = None, None, []
    if a.colmap:
        start, P, K, wh, targets, names = load_colmap(a.colmap, device, with_names=True, undistort=a.undistort)
    elif background is not None:
        start, P, K, wh, targets, alphas = synthetic_scene(a.gaussians, a.cameras, a.width, a.height, 0, device, with_alpha=True)
    else:
        start, P, K, wh, targets = synthetic_scene(a.gaussians, a.cameras, a.width, a.height, 0, device)
    _, losses = train(start, P, K, wh, targets, iterations=a.iterations, densify_from_iter=a.densify_from, rank=rank, world=world,
                      log=print if rank == 0 else (lambda *_: None), background=background, target_alpha=alphas, sh_degree=a.sh_degree,
                      sh_frame=a.sh_frame, sh_every=a.sh_every, save_ply=a.save_ply, load_ply=a.load_ply, centres=a.centres,
                      dilation=a.dilation, clamp_colour=a.clamp_colour, densify=a.densify, densify_on=a.densify_on,
                      antialias=a.antialias, cap_max=a.cap_max, noise_lr=a.noise_lr, opacity_reg=a.opacity_reg, scale_reg=a.scale_reg,
                      prune_contribution=a.prune_contribution, prune_at=prune_at, prune_on=a.prune_on, adam=a.adam,
                      test_every=a.test_every, eval_every=a.eval_every, evals=evals, names=names,
                      screen_grad=a.screen_grad, distortion_reg=a.distortion_reg, distortion_from=a.distortion_from,
                      filter_3d=a.filter_3d, filter_every=a.filter_every, exposure=a.exposure, exposure_lr_init=a.exposure_lr_init,
                      exposure_lr_final=a.exposure_lr_final, save_exposure=a.save_exposure, normal_reg=a.normal_reg,
                      normal_from=a.normal_from, save_mesh=a.save_mesh, mesh_resolution=a.mesh_resolution, mesh_trunc=a.mesh_trunc,
                      normal_depth=a.normal_depth, mesh_depth=a.mesh_depth, init_scale=a.init_scale,
                      mesh_keep=a.mesh_keep, mesh_min_faces=a.mesh_min_faces, mesh_normals=a.mesh_normals)
    if a.eval_json and rank == 0:
        with open(a.eval_json, "w") as f:
            json.dump(evals, f, indent=1)
    if rank == 0:
        print(f"loss {np.mean(losses[:10]):.5f} -> {np.mean(losses[-10:]):.5f}")
    if world > 1:
        torch.distributed.destroy_process_group()
