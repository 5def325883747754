"""Per-camera exposure compensation on the GPU (csrc/gcp_loss.hip: k_ssim_l1_fwd_exposure, k_ssim_l1_bwd_exposure,
k_exposure_fold, k_image_metrics_exposure; loss.py, exposure.py): the identity against the plain kernels bit for bit, the loss
and both gradients against float64 with the float32 PyTorch formulation as the yardstick (tests/exposure_torch.py), per-image
separation through the C ABI, determinism, the fold past one stride, either gradient alone, the metrics, the masked Adam step
of `CameraExposure`, and a frozen scene whose per-camera gains it has to learn."""
import json
import math

import pytest
import torch

from simplegaussiansplat_tk71_amd import _lib, loss
from simplegaussiansplat_tk71_amd import gs_model as gm
from tests import adam_torch as at
from tests import exposure_torch as et

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
# partial tiles in both axes, two images; 3 x 3 tiles with one interior tile (edge_x / edge_y both false there); the smallest
# legal image, three images — the shapes of tests/test_loss_gpu.py, for the same reasons
TWO, NINE, SMALLEST = (2, 3, 22, 33), (1, 3, 39, 71), (3, 3, 6, 6)
FOLD = (1, 3, 257, 545)  # 17 x 18 = 306 tiles: more than the 256 threads of k_exposure_fold, whose loop is not unrolled


def _identity(bsz, device="cpu", dtype=torch.float32):
    return torch.eye(3, 4, dtype=dtype, device=device).repeat(bsz, 1, 1)


def _exposure(kind, gen):
    """One 3 x 4 matrix: 'affine' I + 0.1 randn with offset 0.05 randn; 'permute' a channel permutation with one negative
    off-diagonal entry; 'flat' all zero with offset 0.4 (y is flat: the zero-variance branch of SSIM, dL/dx exactly 0)."""
    e = torch.zeros(3, 4)
    if kind == "affine":
        e[:, :3] = torch.eye(3) + 0.1 * torch.randn(3, 3, generator=gen)
        e[:, 3] = 0.05 * torch.randn(3, generator=gen)
    elif kind == "permute":
        e[0, 2] = e[1, 0] = e[2, 1] = 1.0
        e[0, 1] = -0.25
    else:
        assert kind == "flat"
        e[:, 3] = 0.4
    return e


KINDS = ("affine", "permute", "flat")


def _case(shape, rot, seed, lowcontrast=False):
    """(x, b, E, kinds): float32 on the CPU.  Image i of the batch gets exposure kind (i + rot) % 3.  b = y64 + s (0.02 + 0.2 u),
    s = +-1, u uniform: no |y - b| lies within rounding of 0, so sign(y - b) cannot differ between precisions."""
    gen = torch.Generator().manual_seed(seed)
    bsz = shape[0]
    kinds = [KINDS[(i + rot) % 3] for i in range(bsz)]
    E = torch.stack([_exposure(k, gen) for k in kinds])
    if lowcontrast:
        x, b = 0.9 + 1e-3 * torch.rand(shape, generator=gen), 0.9 + 1e-3 * torch.rand(shape, generator=gen)
        return x, b, E, kinds
    x = torch.rand(shape, generator=gen)
    y64 = et.compensate(x.double(), E.double())
    s = 1.0 - 2.0 * torch.randint(0, 2, shape, generator=gen).double()
    b = (y64 + s * (0.02 + 0.2 * torch.rand(shape, generator=gen).double())).float()
    return x, b, E, kinds


def _float64_and_float32(x, b, E, lamda):
    """The yardsticks on the CPU, upstream gradient 3 -> per dtype (loss, dL/dx, dL/dE) as float64, and from the float64 run
    the condition scale of dL/dE: S[i, c, k] = sum_p |g_c x_k|, S[i, c, 3] = sum_p |g_c|, g = dL/dy."""
    out = {}
    for dtype in (torch.float64, torch.float32):
        xx, ee = x.detach().clone().to(dtype).requires_grad_(True), E.detach().clone().to(dtype).requires_grad_(True)
        y = et.compensate(xx, ee)
        y.retain_grad()
        value = et.loss_torch.splat_loss(y, b.to(dtype), lamda)
        (3.0 * value).backward()
        out[dtype] = (value.item(), xx.grad.double(), ee.grad.double())
        if dtype == torch.float64:
            g = y.grad
            scale = torch.cat([torch.einsum("bchw,bkhw->bck", g.abs(), xx.detach().abs()), g.abs().sum(dim=(2, 3))[..., None]], dim=2)
    return out[torch.float64], out[torch.float32], scale


def _kernel(x, b, E, lamda, device, want_x=True, want_e=True):
    xx, ee = x.detach().clone().to(device).requires_grad_(want_x), E.detach().clone().to(device).requires_grad_(want_e)
    value = gm.splat_loss(xx, b.to(device), lamda, exposure=ee)
    (3.0 * value).backward()
    return value.detach(), xx.grad, ee.grad


def _content(name, shape, gen):
    if name == "noise":
        a = torch.rand(shape, generator=gen)
        return a, (a + 0.25 * torch.randn(shape, generator=gen)).clamp(0, 1)
    assert name == "halves"  # flat 0.9 | 0.1, a +0.01 patch in the image only (tests/test_loss_gpu.py)
    h, w = shape[2:]
    b = torch.full(shape, 0.9)
    b[..., w // 2:] = 0.1
    a = b.clone()
    a[..., h // 4:h // 2, w // 4:(3 * w) // 4] += 0.01
    return a, b


# ---- 1: the identity is the plain path ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("shape", [TWO, NINE], ids=str)
@pytest.mark.parametrize("name", ["noise", "halves"])
def test_identity_exposure_is_the_plain_path_bit_for_bit(name, shape, device):
    a, b = (t.to(device) for t in _content(name, shape, torch.Generator().manual_seed(sum(shape) + len(name))))
    plain = a.clone().requires_grad_(True)
    want = gm.splat_loss(plain, b, 0.2)
    (3.0 * want).backward()
    got, grad, grad_e = _kernel(a, b, _identity(shape[0]), 0.2, device)
    assert float(plain.grad.abs().max()) > 0
    assert torch.equal(got, want.detach()) and torch.equal(grad, plain.grad)
    assert grad_e.shape == (shape[0], 3, 4) and bool(torch.isfinite(grad_e).all()) and float(grad_e.abs().max()) > 0
    render = -0.2 + 1.5 * a  # out of range on both sides: the clamp acts
    for clamp in (True, False):
        m, p = gm.image_metrics(render, b, clamp=clamp, exposure=_identity(shape[0], device)), gm.image_metrics(render, b, clamp=clamp)
        assert all(torch.equal(u, v) for u, v in zip(m, p)), clamp


# ---- 2: accuracy against float64 ----------------------------------------------------------------------------------------------

ACCURACY = [(s, lam, rot) for s in (TWO, NINE) for lam in (0.2, 0.0, 1.0) for rot in range(3)] + [(SMALLEST, 0.2, rot) for rot in range(3)]


def _check_against_float64(x, b, E, kinds, lamda, device, label):
    (l64, gx64, ge64), (l32, gx32, ge32), scale = _float64_and_float32(x, b, E, lamda)
    lk, gxk, gek = _kernel(x, b, E, lamda, device)
    lk, gxk, gek = lk.item(), gxk.cpu().double(), gek.cpu().double()
    assert bool(torch.isfinite(gxk).all()) and bool(torch.isfinite(gek).all())
    rows = {}
    for what, k, t32, t64, floor in (("loss", torch.tensor(lk, dtype=torch.float64), torch.tensor(l32, dtype=torch.float64),
                                      torch.tensor(l64, dtype=torch.float64), EPS * abs(l64)),
                                     ("dx", gxk, gx32, gx64, EPS * gx64.abs().max().item()),
                                     ("dE", gek, ge32, ge64, EPS * scale.max().item())):
        err_k, err_t = (k - t64).abs().max().item(), (t32 - t64).abs().max().item()
        rows[what] = (err_k, err_t, floor)
    print(f"exposure {label}: " + "; ".join(f"{w} err_k {a:.3e} err_t {t:.3e} floor {f:.3e} ratio {a / max(t, f, 1e-300):.3f}"
                                           for w, (a, t, f) in rows.items()))
    for what, (err_k, err_t, floor) in rows.items():
        if what == "dx" and float(gx64.abs().max()) == 0.0:  # every image of the batch is 'flat': exactness is the check
            assert err_k == 0.0
            continue
        assert max(err_t, floor) > 0, (what, "degenerate yardstick")
        assert err_k <= 4 * max(err_t, floor), (what, err_k, err_t, floor)
    for i, kind in enumerate(kinds):
        if kind == "flat":  # y is flat whatever x is: every E[c][k] of the image is 0, and so is dL/dx, exactly
            assert float(gxk[i].abs().max()) == 0.0 and float(gx64[i].abs().max()) == 0.0


@pytest.mark.parametrize("shape,lamda,rot", ACCURACY, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_loss_and_both_gradients_are_as_close_to_float64_as_float32_torch(shape, lamda, rot, device):
    """For the loss, dL/dx and dL/dE separately: err_kernel <= 4 max(err_torch32, floor), the yardstick asserted > 0.  Floor of
    the loss and of dL/dx: one float32 ulp of the largest reference value; of dL/dE: one ulp of max sum_p |g_c x_k| taken in
    float64, the condition scale of the sum."""
    x, b, E, kinds = _case(shape, rot, 1000 * sum(shape) + 10 * rot + int(10 * lamda))
    assert (et.compensate(x.double(), E.double()) - b.double()).abs().min().item() >= 0.02
    _check_against_float64(x, b, E, kinds, lamda, device, f"{shape} lambda {lamda} kinds {kinds}")


def test_low_contrast_keeps_the_badly_conditioned_denominator_in_play(device):
    """0.9 + 1e-3 rand on both sides under an 'affine' exposure: the variances are ~1e-7 and c2 = 9e-4 is the whole
    denominator.  |y - b| stays far from 0 (asserted), so the sign of the L1 term is the same in every precision."""
    x, b, E, kinds = _case(NINE, 0, 77, lowcontrast=True)
    assert kinds == ["affine"]
    assert (et.compensate(x.double(), E.double()) - b.double()).abs().min().item() >= 1e-3
    _check_against_float64(x, b, E, kinds, 0.2, device, "lowcontrast (1, 3, 39, 71) lambda 0.2")


# ---- 3: an image depends on its own exposure alone ----------------------------------------------------------------------------


def _abi(x, b, E, scales, device, want_x=True, want_e=True):
    """gcp_ssim_l1_forward_exposure + gcp_ssim_l1_backward_exposure on contiguous device tensors -> (partial, grad_img, grad_e)."""
    lib, win = _lib.load(), loss._host_window(11, 1.5)
    bsz, _, h, w = x.shape
    maps = [torch.empty_like(x) for _ in range(3)]
    partial = torch.empty(lib.gcp_ssim_blocks(3 * bsz, h, w), 2, device=device)
    grad = torch.full_like(x, float("nan")) if want_x else None
    grad_e = torch.full((bsz, 3, 4), float("nan"), device=device) if want_e else None
    partial_e = torch.empty(lib.gcp_exposure_blocks(bsz, h, w), 12, device=device) if want_e else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        _lib.check(lib.gcp_ssim_l1_forward_exposure(x.data_ptr(), b.data_ptr(), E.data_ptr(), bsz, h, w, win, 1e-4, 9e-4,
                                                    *(m.data_ptr() for m in maps), partial.data_ptr(), stream), "forward")
        status = lib.gcp_ssim_l1_backward_exposure(x.data_ptr(), b.data_ptr(), E.data_ptr(), *(m.data_ptr() for m in maps), bsz, h, w, win,
                                                   scales.data_ptr(), ptr(grad), ptr(partial_e), ptr(grad_e), stream)
    torch.cuda.synchronize(device)
    return status, partial, grad, grad_e


@pytest.mark.parametrize("shape", [(3, 3, 22, 33), (3, 3, 39, 71)], ids=str)
def test_an_image_depends_on_its_own_content_and_exposure_alone(shape, device):
    """Through the C ABI with ONE scales vector, so that no host scaling differs: grad_img and grad_exposure of image i in a
    batch of three with distinct content and exposures equal, bit for bit, those of image i submitted alone."""
    x, b, E, _ = _case(shape, 0, 5)
    x, b, E = x.to(device), b.to(device), E.to(device)
    scales = torch.tensor([-0.2 / 1000.0, 0.8 / 1000.0], device=device)
    status, partial, grad, grad_e = _abi(x, b, E, scales, device)
    assert status == 0 and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(grad_e).all())
    per_image = partial.shape[0] // shape[0]
    for i in range(shape[0]):
        s1, p1, g1, e1 = _abi(x[i:i + 1].contiguous(), b[i:i + 1].contiguous(), E[i:i + 1].contiguous(), scales, device)
        assert s1 == 0
        assert torch.equal(p1, partial[i * per_image:(i + 1) * per_image]), i
        assert torch.equal(g1[0], grad[i]) and torch.equal(e1[0], grad_e[i]), i
    assert not torch.equal(grad_e[0], grad_e[1]) and not torch.equal(grad_e[1], grad_e[2])


def test_c_abi_backward_takes_either_output_and_refuses_neither(device):
    x, b, E, _ = _case(TWO, 0, 6)
    x, b, E = x.to(device), b.to(device), E.to(device)
    scales = torch.tensor([-1e-4, 4e-4], device=device)
    status, _, grad, grad_e = _abi(x, b, E, scales, device)
    sx, _, only_x, none_e = _abi(x, b, E, scales, device, want_e=False)
    se, _, none_x, only_e = _abi(x, b, E, scales, device, want_x=False)
    assert status == sx == se == 0 and none_e is None and none_x is None
    assert torch.equal(only_x, grad) and torch.equal(only_e, grad_e)
    assert _abi(x, b, E, scales, device, want_x=False, want_e=False)[0] == 1  # GCP_ERR_INVALID_ARGUMENT: nothing to compute


# ---- 4, 6: determinism, either gradient alone ---------------------------------------------------------------------------------


@pytest.mark.parametrize("shape", [TWO, NINE], ids=str)
def test_two_calls_agree_and_either_gradient_alone_has_the_same_bits(shape, device):
    x, b, E, _ = _case(shape, 0, 9)
    first, again = _kernel(x, b, E, 0.2, device), _kernel(x, b, E, 0.2, device)
    assert all(torch.equal(u, v) for u, v in zip(first, again))  # no atomics
    value_e, none_x, only_e = _kernel(x, b, E, 0.2, device, want_x=False)
    value_x, only_x, none_e = _kernel(x, b, E, 0.2, device, want_e=False)
    assert none_x is None and none_e is None
    assert torch.equal(value_e, first[0]) and torch.equal(value_x, first[0])
    assert torch.equal(only_e, first[2]) and torch.equal(only_x, first[1])
    render = (-0.2 + 1.5 * x).to(device)
    m1, m2 = (gm.image_metrics(render, b.to(device), exposure=E.to(device)) for _ in range(2))
    assert all(torch.equal(u, v) for u, v in zip(m1, m2))
    value = gm.splat_loss(x.to(device), b.to(device), 0.2, exposure=E.to(device))  # nothing requires a gradient: no maps
    assert torch.equal(value, first[0]) and not value.requires_grad


# ---- 5: the fold past one stride ----------------------------------------------------------------------------------------------


def test_the_fold_adds_more_tiles_than_it_has_threads(device):
    """(1, 3, 257, 545): 306 tiles for the 256 threads of k_exposure_fold (its loop is not unrolled: one stride is one
    iteration).  dL/dE against float64 as above; dL/dx is printed and held to the same bound."""
    assert _lib.load().gcp_exposure_blocks(*[FOLD[0], *FOLD[2:]]) == 306
    x, b, E, kinds = _case(FOLD, 0, 11)
    assert (et.compensate(x.double(), E.double()) - b.double()).abs().min().item() >= 0.02
    _check_against_float64(x, b, E, kinds, 0.2, device, f"{FOLD} lambda 0.2")


# ---- 7: metrics ---------------------------------------------------------------------------------------------------------------


def test_the_clamp_comes_after_the_compensation(device):
    """E = 2 I on an image of 0.8 against a target of ones: y = 1.6 clamps to 1, so mse == 0 and l1 == 0 exactly; clamped before
    the compensation the image would stay 0.8 -> 1.6."""
    x, b = torch.full(TWO, 0.8, device=device), torch.ones(TWO, device=device)
    got = gm.image_metrics(x, b, clamp=True, exposure=2 * _identity(2, device))
    assert got.mse.tolist() == [0.0, 0.0] and got.l1.tolist() == [0.0, 0.0] and all(math.isinf(p) for p in got.psnr.tolist())
    free = gm.image_metrics(x, b, clamp=False, exposure=2 * _identity(2, device))
    assert all(abs(v - 0.36) < 1e-6 for v in free.mse.tolist())


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("shape", [TWO, NINE, SMALLEST], ids=str)
def test_metrics_of_a_general_exposure_against_float64(shape, clamp, device):
    """Per image and per metric |kernel - f64| <= 4 max(|torch32 - f64|, 4 * 2^-23 * mean|term64|): the bound of
    tests/test_metrics_gpu.py, the yardstick compensated with tests/exposure_torch.py and clamped after."""
    gen = torch.Generator().manual_seed(sum(shape) + clamp)
    x, b = -0.2 + 1.5 * torch.rand(shape, generator=gen), torch.rand(shape, generator=gen)
    E = torch.stack([_exposure(KINDS[i % 2], gen) for i in range(shape[0])])
    vals = {}
    for dtype in (torch.float32, torch.float64):
        y = et.compensate(x.to(dtype), E.to(dtype))
        y = y.clamp(0, 1) if clamp else y
        d = y - b.to(dtype)
        terms = (d * d, d.abs(), et.loss_torch.ssim(y, b.to(dtype), max_val=1.0, window_size=11))
        vals[dtype] = ([t.mean(dim=(1, 2, 3)).double() for t in terms], [t.abs().mean(dim=(1, 2, 3)).double() for t in terms])
    got = gm.image_metrics(x.to(device), b.to(device), clamp=clamp, exposure=E.to(device))
    worst = {}
    for field, k32, k64, size in zip(("mse", "l1", "ssim"), vals[torch.float32][0], vals[torch.float64][0], vals[torch.float64][1]):
        have = getattr(got, field).cpu()
        assert have.dtype == torch.float64 and have.shape == (shape[0],)
        err, bound = (have - k64).abs(), 4 * torch.maximum((k32 - k64).abs(), 4 * EPS * size)
        worst[field] = (err / bound.clamp_min(1e-300)).max().item()
    print(f"exposure metrics {shape} clamp={clamp}: worst error / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for field, ratio in worst.items():
        assert ratio <= 1.0, (field, ratio)


def test_evaluate_hands_every_batch_its_own_rows(device):
    """`GS_model_with_param.evaluate(exposure=)`: the identity gives the bits of exposure=None; with three different matrices and
    batch_size 2 every camera's numbers are those of the camera evaluated alone with its own matrix."""
    from simplegaussiansplat_tk71_amd import synthetic

    P, K, wh = synthetic.ring_cameras(3, 64, 48, device=device)
    mean, q, scale, op = synthetic.make_world(300, 64, sigma_px=1.5, seed=0, device=device)
    model = gm.GS_model_with_param(0.5 * mean, q, scale, op)
    gen = torch.Generator().manual_seed(4)
    with torch.no_grad():
        model.color[:, 0, :] = 0.5 + 2.0 * torch.rand(model.color.shape[0], 3, generator=gen).to(device)
    targets = torch.rand(3, 3, 48, 64, generator=gen).to(device)
    E = torch.stack([_exposure(k, gen) for k in KINDS]).to(device)
    plain = model.evaluate(P, K, wh, targets, batch_size=2)
    same = model.evaluate(P, K, wh, targets, batch_size=2, exposure=_identity(3, device))
    assert all(torch.equal(u, v) for u, v in zip(plain, same))
    got = model.evaluate(P, K, wh, targets, batch_size=2, exposure=E)
    assert got.mse.shape == (3,) and not torch.equal(got.mse, plain.mse)
    for i in range(3):
        alone = model.evaluate(P[i:i + 1], K[i:i + 1], wh[i:i + 1], targets[i:i + 1], exposure=E[i:i + 1])
        assert all(torch.equal(u[i:i + 1], v) for u, v in zip(got, alone)), i
    with pytest.raises(RuntimeError, match="one matrix per camera"):
        model.evaluate(P, K, wh, targets, exposure=E[:2])


# ---- 8: CameraExposure.step ---------------------------------------------------------------------------------------------------


def test_step_moves_the_drawn_cameras_and_keeps_the_others_bit_for_bit(device):
    """Three steps that draw cameras {0, 2} of five while EVERY row has a gradient: rows 1, 3 and 4 stay [I | 0] with zero
    moments, bit for bit; rows 0 and 2 follow float64 Adam from the state before each step within the bounds of
    tests/adam_torch.py (float32 torch.optim.Adam is held to them first), at the rate `set_lr` gave."""
    ce = gm.CameraExposure(5, device=device)
    gen = torch.Generator().manual_seed(3)
    drawn = torch.tensor([True, False, True, False, False])
    keep = drawn.reshape(5, 1).expand(5, 12)
    for step in (1, 2, 3):
        grad = 0.1 * torch.randn(5, 3, 4, generator=gen)
        st = ce.optimizer.state.get(ce.matrix, {})
        before = tuple(t.detach().cpu().reshape(5, 12).clone() for t in (ce.matrix, st.get("exp_avg", torch.zeros(5, 3, 4)),
                                                                        st.get("exp_avg_sq", torch.zeros(5, 3, 4))))
        ce.matrix.grad = grad.to(device)
        lr = ce.set_lr(step - 1)
        ce.step([0, 2])
        assert ce.matrix.grad is None
        st = ce.optimizer.state[ce.matrix]
        assert int(st["step"]) == step  # one count for all rows: the bias correction is global
        after = tuple(t.detach().cpu().reshape(5, 12) for t in (ce.matrix, st["exp_avg"], st["exp_avg_sq"]))
        want, bounds = at.reference(before[0], grad.reshape(5, 12), before[1], before[2], step, lr)
        at.worst(at.torch_step(before[0], grad.reshape(5, 12), before[1], before[2], step, lr), want, bounds, what=("float32 torch", step))
        at.worst(after, want, bounds, keep=keep, what=("kernel", step))
        assert not torch.equal(after[0][drawn], before[0][drawn])
        assert torch.equal(after[0][~drawn].view(torch.int32), _identity(5).reshape(5, 12)[~drawn].view(torch.int32))
        assert not after[1][~drawn].view(torch.int32).any() and not after[2][~drawn].view(torch.int32).any()
    mask = torch.tensor([False, True, False, False, False], device=device)  # the mask `allreduce_grads` returns
    ce.matrix.grad = torch.ones(5, 3, 4, device=device)
    ce.step(mask)
    assert not torch.equal(ce.matrix.detach()[1].cpu(), torch.eye(3, 4)) and torch.equal(ce.matrix.detach()[3:].cpu(), _identity(2))


# ---- 9: it learns -------------------------------------------------------------------------------------------------------------


def test_it_learns_per_camera_gains_of_a_frozen_scene(device, tmp_path):
    """A frozen synthetic scene (300 Gaussians, four cameras at 64 x 48); the targets are its own renders times fixed per-camera
    gains in 0.7 .. 1.3; only `CameraExposure` is trained, 200 steps of two cameras.  Gate: every camera's final loss is
    strictly below its loss at the identity.  The achieved ratio and the recovered diagonals are printed, not thresholded:
    nobody has measured them.  Then the example's `train(exposure=True)` runs 20 iterations with finite losses and its
    exposure.json reloads to the same bits."""
    from examples.train_cameras import synthetic_scene, train

    start, P, K, wh, renders = synthetic_scene(300, 4, 64, 48, 0, device)
    assert renders.shape == (4, 3, 48, 64) and float(renders.mean()) > 0.01
    gains = torch.tensor([0.7, 0.9, 1.1, 1.3], device=device)
    targets = renders * gains.view(4, 1, 1, 1)

    def per_camera(E):
        with torch.no_grad():
            return [gm.splat_loss(renders[i:i + 1], targets[i:i + 1], 0.2, exposure=E[i:i + 1]).item() for i in range(4)]

    ce = gm.CameraExposure(4, device=device)
    at_identity = per_camera(ce.matrix.detach())
    for it in range(200):
        kept = [(2 * it) % 4, (2 * it + 1) % 4] if (it // 2) % 2 == 0 else [(2 * it + 1) % 4, (2 * it + 2) % 4]
        gm.splat_loss(renders[kept], targets[kept], 0.2, exposure=ce.rows(kept)).backward()
        ce.set_lr(it)
        ce.step(kept)
    final = per_camera(ce.matrix.detach())
    diag = torch.diagonal(ce.matrix.detach()[:, :, :3], dim1=1, dim2=2).cpu()
    print("exposure learns: loss at identity " + " ".join(f"{v:.5f}" for v in at_identity) + "; after 200 steps "
          + " ".join(f"{v:.5f}" for v in final) + "; ratio " + " ".join(f"{f / max(a, 1e-300):.3f}" for f, a in zip(final, at_identity))
          + "; diagonals " + " ".join("(" + " ".join(f"{v:.3f}" for v in row) + ")" for row in diag.tolist()) + f"; gains {gains.tolist()}")
    for i in range(4):
        assert final[i] < at_identity[i], (i, final[i], at_identity[i])

    path = str(tmp_path / "exposure.json")
    _, losses = train(start, P, K, wh, targets.clamp(0, 1), iterations=20, batch_size=2, exposure=True, save_exposure=path, log=lambda *_: None)
    assert len(losses) == 20 and all(math.isfinite(v) for v in losses)
    first, second = gm.CameraExposure(4), gm.CameraExposure(4)
    first.load_json(path)
    assert not torch.equal(first.matrix.detach(), _identity(4))  # something was learned and written
    again = str(tmp_path / "again.json")
    first.save_json(again)
    second.load_json(again)
    assert torch.equal(first.matrix.detach().view(torch.int32), second.matrix.detach().view(torch.int32))
    with open(path) as f, open(again) as g:
        assert json.load(f) == json.load(g)
    # with a held-out camera: the matrices belong to the training cameras, by name, and the held-out one is measured with identity
    evals = []
    names = ["d.jpg", "a.jpg", "c.jpg", "b.jpg"]  # sorted: a (held out by test_every=4), b, c, d
    _, losses = train(start, P, K, wh, targets.clamp(0, 1), iterations=4, batch_size=2, exposure=True, save_exposure=path, log=lambda *_: None,
                      test_every=4, evals=evals, names=names)
    assert len(losses) == 4 and all(math.isfinite(v) for v in losses)
    assert len(evals) == 1 and evals[0]["exposure"] == "identity" and list(evals[0]["per_image"]) == ["a.jpg"]
    with open(path) as f:
        assert sorted(json.load(f)) == ["b.jpg", "c.jpg", "d.jpg"]
    gm.CameraExposure(3, names=["b.jpg", "c.jpg", "d.jpg"]).load_json(path)
