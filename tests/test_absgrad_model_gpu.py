"""screen_grad="abs" through the model (GS_model_with_param): `forward` and `render` hand one [m, 2] buffer per drawn camera
to the Function, the hook on the camera's centres accumulates that buffer instead of the signed gradient, and nothing else
moves — the views, the parameters' gradients and the optimiser steps are those of screen_grad="signed" bit for bit.

Bound of the comparison with the signed statistic: per camera and component the kernel's value is within 1e-5 (1 + scale) of
the exact absolute sum (tests/test_absgrad_gpu.py), scale >= the sum itself, and the exact absolute sum is >= the exact
|signed sum|; the statistic is the norm of the two components times (W/2, H/2), so it is >= the signed one minus
sum over cameras of 1e-5 (W/2 (1 + a_x) + H/2 (1 + a_y)), with (a_x, a_y) the buffer's own values standing in for the scale
(a lower bound of it: the test asks more than the rule, never less)."""
import math

import pytest
import torch

from tests.util import TOL

pytestmark = pytest.mark.gpu
W, H = 64, 48


def small_world(device, n=300, cameras=3):
    from examples.train_cameras import synthetic_scene

    start, P, K, wh, targets = synthetic_scene(n, cameras, W, H, 0, device)
    q = torch.zeros(n, 4, device=device)
    q[:, 3] = 1
    args = (start.clone(), q, torch.full((n, 3), math.log(0.06), device=device), torch.zeros(n, 1, device=device))
    return args, P, K, wh, targets


def make_models(device, **kw):
    from simplegaussiansplat_tk71_amd import gs_model as gm

    args, P, K, wh, targets = small_world(device)
    models = [gm.GS_model_with_param(*(a.clone() for a in args), centres="subpixel", densify_on="screen", screen_grad=mode, **kw)
              for mode in ("abs", "signed")]
    return models, P, K, wh, targets


def spy_on(model):
    """Every camera `camera_inputs` returns with a differentiable centre, its gradient retained."""
    seen, inner = [], model.camera_inputs

    def spy(*a, **kw):
        out = inner(*a, **kw)
        for cam in out[0]:
            if cam is not None and cam["mean"].requires_grad:
                cam["mean"].retain_grad()
                seen.append(cam)
        return out

    model.camera_inputs = spy
    return seen


def loss_of(model, how, P, K, wh, targets, background):
    from simplegaussiansplat_tk71_amd import gs_model as gm

    if how == "forward":
        images, names, grad_iter = model(P, K, wh, list(range(P.shape[0])))
        return gm.splat_loss(images, targets), grad_iter
    images, depth, alpha, names, grad_iter = model.render(P, K, wh, background=background)
    return gm.splat_loss(images, targets) + 0.05 * depth.mean() + 0.1 * (alpha * alpha).mean(), grad_iter


@pytest.mark.parametrize("how", ["forward", "render"])
def test_statistic_is_the_accumulated_buffers_and_exceeds_the_signed_one(device, how):
    from simplegaussiansplat_tk71_amd import gs_model as gm

    (model, signed), P, K, wh, targets = make_models(device)
    assert model.screen_grad == "abs" and signed.screen_grad == "signed"
    background = torch.tensor([0.2, 0.7, 0.4], device=device)
    n = model.mean.shape[0]
    seen, seen_signed = spy_on(model), spy_on(signed)
    loss_of(model, how, P, K, wh, targets, background)[0].backward()
    loss_of(signed, how, P, K, wh, targets, background)[0].backward()
    assert len(seen) == len(seen_signed) == 3
    want_norm, want_views = torch.zeros(n, device=device), torch.zeros(n, dtype=torch.int32, device=device)
    bound = torch.zeros(n, dtype=torch.float64, device=device)
    scale = (0.5 * W, 0.5 * H)
    for cam, ref in zip(reversed(seen), reversed(seen_signed)):  # the order `backward` reaches the cameras in
        buf = cam["absgrad"]
        assert "absgrad" not in ref
        assert buf.shape == (cam["index"].numel(), 2) and buf.dtype == torch.float32 and not buf.requires_grad
        assert torch.equal(cam["mean"].grad, ref["mean"].grad)  # the signed gradient of the centres: the same bits
        slack = TOL * (1.0 + buf.double())
        assert bool((buf.double() >= cam["mean"].grad.double().abs() - slack).all()) and bool(buf.any())
        gm.accumulate_screen_grads(buf, cam["index"], scale, want_norm, want_views)
        bound.index_add_(0, cam["index"], slack[:, 0] * scale[0] + slack[:, 1] * scale[1])
    # (the bound of tests/test_densify_gpu.py for the signed statistic: the order of a Gaussian's up to three additions is autograd's)
    torch.testing.assert_close(model.screen_grads_norm, want_norm, rtol=1e-6, atol=0)
    assert torch.equal(model.screen_grads_views, want_views)
    assert torch.equal(model.screen_grads_views, signed.screen_grads_views) and int(want_views.max()) == 3
    margin = model.screen_grads_norm.double() - signed.screen_grads_norm.double()
    assert bool((margin >= -bound).all())
    hit = want_views > 0
    ratio = (model.screen_grads_norm[hit] / signed.screen_grads_norm[hit].clamp_min(1e-30)).median().item()
    print(f"{how}: {int(hit.sum())} Gaussians seen, median abs / signed statistic {ratio:.3g}, "
          f"{int((margin > bound).sum())} strictly larger")
    assert int((margin > bound).sum()) >= int(hit.sum()) // 2 and ratio > 1.2  # per-pixel terms of a splat do cancel
    for (k, p), (_, r) in zip(model.named_parameters(), signed.named_parameters()):
        assert torch.equal(p.grad, r.grad), k
    # nothing is collected without gradients
    with torch.no_grad():
        model(P, K, wh, [0, 1, 2])
    assert torch.equal(model.screen_grads_views, want_views)


def test_five_steps_take_the_parameters_and_adam_moments_of_the_signed_model(device):
    (model, signed), P, K, wh, targets = make_models(device)
    background = torch.tensor([0.2, 0.7, 0.4], device=device)
    for step in range(5):
        for m in (model, signed):
            loss, grad_iter = loss_of(m, "forward" if step % 2 == 0 else "render", P, K, wh, targets, background)
            loss.backward()
            m.param_iter_update(grad_iter)
            m.train_step()
    for (k, p), (_, r) in zip(model.named_parameters(), signed.named_parameters()):
        assert torch.equal(p.detach(), r.detach()), k
        st, rt = model._optimizer.state[p], signed._optimizer.state[r]
        assert st["step"] == rt["step"] == 5, k
        assert torch.equal(st["exp_avg"], rt["exp_avg"]) and torch.equal(st["exp_avg_sq"], rt["exp_avg_sq"]), k
    assert torch.equal(model.screen_grads_views, signed.screen_grads_views) and int(model.screen_grads_views.max()) == 15
    assert torch.equal(model.mean_grads_norm, signed.mean_grads_norm)
    assert bool((model.screen_grads_norm > signed.screen_grads_norm).any())


def test_device_densification_decides_on_the_abs_statistic_and_resizes_it(device):
    """A threshold just above the largest signed statistic: the abs model densifies Gaussians the signed one leaves alone; the
    statistic comes back zeroed at the new length and the next step collects at that length."""
    (model, signed), P, K, wh, targets = make_models(device)
    n = model.mean.shape[0]
    for m in (model, signed):
        loss_of(m, "forward", P, K, wh, targets, None)[0].backward()
    per_view = [m.screen_grads_norm / m.screen_grads_views.clamp_min(1) for m in (model, signed)]
    threshold = 1.001 * per_view[1].max().item()  # just above everything the signed statistic holds
    assert int((per_view[0] >= threshold).sum()) >= 1 and not bool((per_view[1] >= threshold).any())
    sizes = []
    for m in (model, signed):
        m.grad_threshold = threshold
        m._optimizer.zero_grad()
        before, after = m.densify_and_prune_device(1.0, seed=0)
        assert before == n and m.mean.shape[0] == after
        assert m.screen_grads_norm.shape == m.screen_grads_views.shape == (after,)
        assert not m.screen_grads_norm.any() and not m.screen_grads_views.any()
        sizes.append(after)
    grown = int((per_view[0] >= threshold).sum())
    assert grown >= 1 and sizes[0] > sizes[1]  # the hot Gaussians of the abs statistic were split or cloned
    loss_of(model, "render", P, K, wh, targets, None)[0].backward()
    assert model.screen_grads_norm.shape == (sizes[0],) and bool(model.screen_grads_norm.any()) and int(model.screen_grads_views.max()) == 3


def test_training_loop_takes_the_signed_steps_until_it_densifies_on_the_abs_statistic(device):
    """examples/train_cameras.train(screen_grad=...): one densification, at iteration 45.  Up to it both runs take the same
    steps bit for bit (45 equal losses); there the abs statistic is >= the signed one for every Gaussian, so every Gaussian the
    signed run splits or clones the abs run does too — a hot Gaussian never writes fewer rows than a kept one."""
    from examples.train_cameras import synthetic_scene, train

    start, P, K, wh, targets = synthetic_scene(600, 6, W, H, 0, device)
    runs = {}
    for mode in ("abs", "signed"):
        lines = []
        model, losses = train(start, P, K, wh, targets, iterations=60, densify_from_iter=40, densification_interval=45, opacity_reset_interval=0,
                              log=lines.append, centres="subpixel", densify="device", densify_on="screen", screen_grad=mode)
        assert model.screen_grad == mode and len(losses) == 60 and all(math.isfinite(l) for l in losses)
        assert all(st["step"] == 60 for st in model._optimizer.state.values())  # Adam was never restarted
        for t in (model.screen_grads_norm, model.screen_grads_views):
            assert t.shape[0] == model.mean.shape[0]
        runs[mode] = (model.mean.shape[0], losses)
    print({k: v[0] for k, v in runs.items()})
    assert runs["abs"][1][:45] == runs["signed"][1][:45]
    assert runs["abs"][0] >= runs["signed"][0] and runs["abs"][0] > 600
