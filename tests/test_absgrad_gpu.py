"""The absolute screen-space gradient (raster.blend_absgrad / blend_absgrad_depth, csrc/gcp_absgrad.hip: k_absgrad_tile /
k_absgrad_reduce) against a dense float64 loop written here, against the blend backward's signed gradient, and through the
two autograd Functions (`absgrad=` of custom_autograd_grouped_cumprod / RenderDepth, eager and captured).

The dense loop (`dense_absgrad`) runs the transmittance front to back with the drop rule of tests/test_contribution_gpu.py's
dense_contribution, then goes back to front for R and m(k, p) = T o g (c - R) Λ (p - mu), and returns the signed sums, the
absolute sums and the condition scale: the same sums with the two addends of d = c - R taken in absolute value,
T o g (|c| + |R|) |Λ (p - mu)| (the form of tests/util.full_cover_scales' "common" factor).  It is validated independently of
the kernel: its signed sums equal the float64 autograd gradient, w.r.t. a float mean, of a dense float64 render.

Tolerance (tests/util.assert_parity, TOL = 1e-5): |got - want| <= 1e-5 (1 + scale).  The float32 form of the dense loop
stays within 0.02 of that bound on every scene and variant below (checked on the CPU); the worst |error| / bound the kernel
reaches per scene is printed by every parity test (profiles/r20_absgrad.md holds the figures of one run)."""
import pytest
import torch

from tests.util import TOL, assert_parity, make_scene

pytestmark = pytest.mark.gpu
KEYS = ("start", "end", "mean", "vinv", "opacity", "l_d")


# ---- the dense reference ----------------------------------------------------------------------------------------------
def dense_absgrad(sc, grad_image=None, depth=None, grad_depth=None, grad_alpha=None, background=None, dtype=torch.float64):
    """-> (signed [N, 2], absolute [N, 2], scale [N, 2]) of the loss <image, grad_image> (+ <depth_map, grad_depth> +
    <alpha, grad_alpha>, the image over `background`); every map argument may be None (zero / black)."""
    width, height = sc["width"], sc["height"]
    n = sc["start"].shape[0]
    zero = torch.zeros((), dtype=dtype)
    ys = torch.arange(height + 1, dtype=dtype)[:, None]
    xs = torch.arange(width + 1, dtype=dtype)[None, :]
    mean, v, op, l_d = sc["mean"].to(dtype), sc["vinv"].to(dtype), sc["opacity"].reshape(-1).to(dtype), sc["l_d"].to(dtype)
    g_img = torch.zeros(height + 1, width + 1, 3, dtype=dtype) if grad_image is None else grad_image.to(dtype)
    T = torch.ones(height + 1, width + 1, dtype=dtype)
    kept = []
    for i in range(n):  # front to back: the exclusive transmittance of every pair, and whether the pair is kept
        x0, y0 = max(int(sc["start"][i, 0]), 0), max(int(sc["start"][i, 1]), 0)
        x1, y1 = min(int(sc["end"][i, 0]), width), min(int(sc["end"][i, 1]), height)
        if x1 < x0 or y1 < y0:
            kept.append(None)
            continue
        dx = (xs[:, x0:x1 + 1] - mean[i, 0]).expand(y1 - y0 + 1, -1)
        dy = (ys[y0:y1 + 1, :] - mean[i, 1]).expand(-1, x1 - x0 + 1)
        a, b, c, d = v[i, 0, 0], v[i, 0, 1], v[i, 1, 0], v[i, 1, 1]
        g = torch.exp(-0.5 * ((dx * a + dy * c) * dx + (dx * b + dy * d) * dy))
        Tb = T[y0:y1 + 1, x0:x1 + 1].clone()
        incl = Tb * (1.0 - op[i] * g)
        kept.append((x0, y0, x1, y1, dx, dy, g, Tb, incl != 0))
        T[y0:y1 + 1, x0:x1 + 1] = incl
    R = torch.zeros(height + 1, width + 1, dtype=dtype)
    if depth is not None:  # the absorbing layer behind the list
        cb = g_img @ background.to(dtype) if background is not None else torch.zeros_like(R)
        ga = grad_alpha.to(dtype) if grad_alpha is not None else torch.zeros_like(R)
        R = torch.where(T != 0, cb - ga, zero)
    signed, absolute, scale = (torch.zeros(n, 2, dtype=dtype) for _ in range(3))
    for i in reversed(range(n)):
        if kept[i] is None:
            continue
        x0, y0, x1, y1, dx, dy, g, Tb, keep = kept[i]
        c = g_img[y0:y1 + 1, x0:x1 + 1] @ l_d[i]
        if depth is not None and grad_depth is not None:
            c = c + grad_depth.to(dtype)[y0:y1 + 1, x0:x1 + 1] * depth[i].to(dtype)
        Rb = R[y0:y1 + 1, x0:x1 + 1]
        dd = c - Rb
        w = torch.where(keep, Tb * op[i] * g, zero)
        lam = (v[i, 0, 0] * dx + v[i, 1, 0] * dy, v[i, 0, 1] * dx + v[i, 1, 1] * dy)  # Λ (p - mu): A dx + C dy, B dx + D dy
        for axis in range(2):
            m = w * dd * lam[axis]
            signed[i, axis], absolute[i, axis] = m.sum(), m.abs().sum()
            scale[i, axis] = (w * (c.abs() + Rb.abs()) * lam[axis].abs()).sum()
        R[y0:y1 + 1, x0:x1 + 1] = torch.where(keep, Rb + op[i] * g * dd, Rb)
    return signed, absolute, scale


def dense_render_grad(sc, grad_image=None, depth=None, grad_depth=None, grad_alpha=None, background=None):
    """float64 autograd: d/dmean of <image, grad_image> + <depth_map, grad_depth> + <alpha, grad_alpha> for a dense render
    with the pair rule above (symmetric Λ: there d g / d mu = g Λ (p - mu))."""
    dtype = torch.float64
    width, height = sc["width"], sc["height"]
    n = sc["start"].shape[0]
    ys = torch.arange(height + 1, dtype=dtype)[:, None]
    xs = torch.arange(width + 1, dtype=dtype)[None, :]
    mean = sc["mean"].to(dtype).clone().requires_grad_(True)
    v, op, l_d = sc["vinv"].to(dtype), sc["opacity"].reshape(-1).to(dtype), sc["l_d"].to(dtype)
    T = torch.ones(height + 1, width + 1, dtype=dtype)
    image = torch.zeros(height + 1, width + 1, 3, dtype=dtype)
    dmap = torch.zeros(height + 1, width + 1, dtype=dtype)
    for i in range(n):
        x0, y0 = max(int(sc["start"][i, 0]), 0), max(int(sc["start"][i, 1]), 0)
        x1, y1 = min(int(sc["end"][i, 0]), width), min(int(sc["end"][i, 1]), height)
        if x1 < x0 or y1 < y0:
            continue
        dx = xs[:, x0:x1 + 1] - mean[i, 0]
        dy = ys[y0:y1 + 1, :] - mean[i, 1]
        g = torch.exp(-0.5 * ((dx * v[i, 0, 0] + dy * v[i, 1, 0]) * dx + (dx * v[i, 0, 1] + dy * v[i, 1, 1]) * dy))
        Tb = T[y0:y1 + 1, x0:x1 + 1]
        incl = Tb * (1.0 - op[i] * g)
        w = torch.where(incl != 0, Tb * op[i] * g, torch.zeros((), dtype=dtype))
        pad = (x0, width - x1, y0, height - y1)
        image = image + torch.nn.functional.pad(w, pad)[:, :, None] * l_d[i]
        if depth is not None:
            dmap = dmap + torch.nn.functional.pad(w, pad) * depth[i].to(dtype)
        T = T + torch.nn.functional.pad(incl - Tb, pad)
    loss = torch.zeros((), dtype=dtype)
    if background is not None:
        image = image + T[:, :, None] * background.to(dtype)
    if grad_image is not None:
        loss = loss + (image * grad_image.to(dtype)).sum()
    if grad_depth is not None:
        loss = loss + (dmap * grad_depth.to(dtype)).sum()
    if grad_alpha is not None:
        loss = loss + ((1.0 - T) * grad_alpha.to(dtype)).sum()
    return torch.autograd.grad(loss, mean)[0]


# ---- scenes: the smallest that reach each branch ------------------------------------------------------------------------
def stack_scene(n_layers, opacity_lo, opacity_hi, seed, sigma=(4.0, 12.0), w=15, h=15):
    """`n_layers` wide Gaussians over one 16x16 tile: every pixel's list is n_layers deep (100: 4 chunks of 32)."""
    g = torch.Generator().manual_seed(seed)
    n = n_layers
    sx = sigma[0] + (sigma[1] - sigma[0]) * torch.rand(n, generator=g)
    vinv = torch.zeros(n, 2, 2)
    vinv[:, 0, 0] = 1.0 / (sx * sx)
    vinv[:, 1, 1] = 1.0 / (sx * sx)
    start = torch.zeros(n, 2, dtype=torch.int32)
    end = torch.tensor([[w, h]], dtype=torch.int32).repeat(n, 1)
    return {"start": start, "end": end, "mean": torch.randint(2, 14, (n, 2), generator=g).to(torch.int32), "vinv": vinv,
            "opacity": opacity_lo + (opacity_hi - opacity_lo) * torch.rand(n, 1, generator=g), "l_d": 0.1 + torch.rand(n, 3, generator=g),
            "wimg": torch.randn(h + 1, w + 1, 3, generator=g), "width": w, "height": h}


def frame_scene(seed=1, **kw):
    return make_scene(40, 191, 175, 30, seed, **kw)  # 12 x 11 tiles, the last column and row of them partial


def subpixel_scene():
    sc = frame_scene()
    sc["mean"] = sc["mean"].float() + torch.rand(40, 2, generator=torch.Generator().manual_seed(8)) - 0.5
    return sc


def wide_scene():
    """Three whole-frame boxes: 12 x 11 = 132 tile slots each, which the reduce takes with the whole wave (>= 128)."""
    sc = frame_scene(3)
    for row in (5, 17, 33):
        sc["start"][row] = torch.tensor([0, 0])
        sc["end"][row] = torch.tensor([191, 175])
        sc["vinv"][row] = 2e-4 * torch.eye(2)
        sc["opacity"][row] = 0.3
    return sc


def empty_box_scene():
    sc = frame_scene(4)
    sc["end"][10] = sc["start"][10] - 1                                             # an empty box: end < start
    sc["start"][20], sc["end"][20] = torch.tensor([200, 3]), torch.tensor([260, 9])  # wholly right of the frame
    return sc


def skewed_scene():
    """A non-symmetric Λ: B != C.  The exponent sees B + C, Λ (p - mu) sees (A dx + C dy, B dx + D dy)."""
    sc = frame_scene(5)
    skew = 0.3 * sc["vinv"][:, 0, 1].abs() + 1e-3
    sc["vinv"][:, 0, 1] += skew
    sc["vinv"][:, 1, 0] -= skew
    return sc


def none_scene():
    sc = frame_scene()
    return {k: (v[:0] if torch.is_tensor(v) and v.shape[:1] == (40,) else v) for k, v in sc.items()}


SCENES = {
    "frame": frame_scene,
    "subpixel": subpixel_scene,
    "stack": lambda: stack_scene(100, 0.02, 0.3, 9),
    # opacities near 1 and g >= 0.8 everywhere: every pixel's transmittance underflows inside the second or third chunk (the
    # front-to-back recomputation) and is an exact zero before the last one (the wave-uniform skip); the pairs behind are dropped
    "underflow": lambda: stack_scene(100, 0.9, 0.999, 10, sigma=(30.0, 60.0)),
    "one_every": lambda: frame_scene(2, opacity_one_every=5),
    "wide": wide_scene,
    "empty_box": empty_box_scene,
    "none": none_scene,
    "skewed": skewed_scene,
}
# name -> (grad_image, grad_depth, grad_alpha, background) used; "colour" is the entry point without depth
VARIANTS = {
    "colour": None,
    "grad_depth_only": (False, True, False, False),
    "grad_alpha_only": (False, False, True, False),
    "background": (True, False, False, True),
    "all_three": (True, True, True, True),
    "no_grad_image": (False, True, True, True),
}
_cache = {}


def scene_and_maps(name, variant):
    """(scene, keyword arguments of the dense loop) — built once per (scene, variant) and left unchanged."""
    key = (name, variant)
    if key not in _cache:
        sc = SCENES[name]()
        n, shape = sc["start"].shape[0], (sc["height"] + 1, sc["width"] + 1)
        g = torch.Generator().manual_seed(77)
        use = VARIANTS[variant]
        if use is None:
            maps = {"grad_image": sc["wimg"]}
        else:
            maps = {"depth": 1.0 + 4.0 * torch.rand(n, generator=g),
                    "grad_image": sc["wimg"] if use[0] else None,
                    "grad_depth": 0.3 * torch.randn(shape, generator=g) if use[1] else None,
                    "grad_alpha": torch.randn(shape, generator=g) if use[2] else None,
                    "background": torch.tensor([0.9, 0.2, 0.5]) if use[3] else None}
        _cache[key] = (sc, maps, dense_absgrad(sc, **maps))
    return _cache[key]


def hip_absgrad(sc, maps, device, capacity=None, with_backward=True):
    """-> (absgrad [N, 2], grad_mean [N, 2] of the matching backward or None, bins)"""
    from simplegaussiansplat_tk71_amd import raster

    d = [sc[k].to(device) for k in KEYS]
    bins = raster.bin_tiles(d[0], d[1], sc["width"], sc["height"], capacity=capacity)
    dev = lambda t: None if t is None else t.to(device)  # noqa: E731
    if "depth" not in maps:
        _, ckpt = raster.blend_forward(bins, *d, with_checkpoints=True)
        got = raster.blend_absgrad(bins, *d, ckpt, dev(maps["grad_image"]))
        g_mean = raster.blend_backward(bins, *d, ckpt, dev(maps["grad_image"]))[0] if with_backward else None
    else:
        z = dev(maps["depth"])
        rest = (dev(maps["grad_image"]), dev(maps["grad_depth"]), dev(maps["grad_alpha"]), dev(maps["background"]))
        ckpt = raster.blend_forward_depth(bins, *d, z, rest[3], with_checkpoints=True)[3]
        got = raster.blend_absgrad_depth(bins, *d, z, ckpt, *rest)
        g_mean = raster.blend_backward_depth(bins, *d, z, ckpt, *rest)[0] if with_backward else None
    return got, g_mean, bins


def parity(got, want, scale, what, tol=TOL):
    """tests/util.assert_parity, elementwise over [N, 2]"""
    assert got.shape == want.shape == scale.shape, what
    assert_parity(got.reshape(-1), want.reshape(-1), scale.reshape(-1), what, tol=tol)


def worst_ratio(got, want, scale):
    if got.numel() == 0:
        return 0.0
    return ((got.detach().cpu().double() - want).abs() / (TOL * (1.0 + scale))).max().item()


# ---- the reference itself -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["colour", "all_three"])
@pytest.mark.parametrize("name", ["frame", "subpixel", "stack", "one_every"])
def test_dense_loop_signed_sums_are_the_autograd_gradient_of_a_dense_render(name, variant):
    """Independent of the kernel (runs on the CPU): sum_p m(k, p) of the loop is d loss / d mean_k of a float64 render."""
    sc, maps, _ = scene_and_maps(name, variant)
    # Λ exactly symmetric (the inverse make_scene takes in float32 is so only to an ulp): there d g / d mu = g Λ (p - mu)
    sc = dict(sc, vinv=0.5 * (sc["vinv"].double() + sc["vinv"].double().transpose(1, 2)))
    signed, absolute, scale = dense_absgrad(sc, **maps)
    want = dense_render_grad(sc, **maps)
    err = (signed - want).abs().max().item()
    print(f"{name} {variant}: max |signed - autograd| {err:.3g}, max |signed| {signed.abs().max().item():.3g}")
    parity(signed, want, scale, f"{name} {variant}", tol=1e-12)
    assert bool((absolute >= signed.abs() * (1 - 1e-12)).all()) and bool((scale >= absolute * (1 - 1e-12)).all())


# ---- parity with the dense loop -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(SCENES))
def test_parity_with_the_dense_loop_and_with_the_signed_gradient(device, name, variant):
    """|absgrad - want| <= 1e-5 (1 + scale) against the float64 loop; the signed sums of the loop match the backward's
    grad_mean by the same rule (the B != C convention is grad_reduce's), and absgrad >= |grad_mean| up to the bound."""
    sc, maps, (signed, absolute, scale) = scene_and_maps(name, variant)
    n = sc["start"].shape[0]
    got, g_mean, bins = hip_absgrad(sc, maps, device)
    assert got.shape == (n, 2) and got.dtype == torch.float32 and got.is_cuda
    print(f"{name} {variant}: n {n}, entries {bins.n_tile_pairs}, worst |error| / bound: absgrad {worst_ratio(got, absolute, scale):.3g}, "
          f"grad_mean {worst_ratio(g_mean, signed, scale):.3g}")
    parity(got, absolute, scale, f"{name} {variant} absgrad")
    parity(g_mean, signed, scale, f"{name} {variant} grad_mean")
    assert bool((got.cpu().double() >= g_mean.cpu().double().abs() - TOL * (1.0 + scale)).all())
    assert bool((got >= 0).all())
    if n and not (variant == "grad_alpha_only" and name in ("stack", "underflow")):  # (there only T_N carries a gradient: ~0)
        assert float(absolute.max()) > 1e-3  # the scene is not a trivial one


def test_scenes_reach_their_branches(device):
    """What the scene names promise, checked on the bins and on a float32 transmittance: slot counts either side of the
    wave-wide reduce, an empty box that reads exactly 0, and — "underflow" — chunks a pixel underflows in (T behind the chunk
    below FLT_MIN, in front of it not 0) as well as a last chunk every pixel enters behind an exact zero."""
    sc, maps, (_, absolute, _) = scene_and_maps("wide", "colour")
    got, _, bins = hip_absgrad(sc, maps, device, with_backward=False)
    slots = (bins.tile_off[1:] - bins.tile_off[:-1]).cpu()
    assert int(slots.max()) == 132 and int((slots >= 128).sum()) == 3 and int(slots.min()) < 128
    sc, maps, _ = scene_and_maps("empty_box", "colour")
    got, _, _ = hip_absgrad(sc, maps, device, with_backward=False)
    assert not got[10].any() and not got[20].any() and int((got > 0).all(dim=1).sum()) >= 30
    sc, maps, (_, absolute, _) = scene_and_maps("underflow", "colour")
    T = torch.ones(16, 16)
    ys, xs = torch.meshgrid(torch.arange(16.0), torch.arange(16.0), indexing="ij")
    at = {}
    for i in range(100):
        if i % 32 == 0:
            at[i] = T.clone()
        dx, dy = xs - sc["mean"][i, 0], ys - sc["mean"][i, 1]
        T = T * (1.0 - sc["opacity"][i, 0] * torch.exp(-0.5 * sc["vinv"][i, 0, 0] * (dx * dx + dy * dy)))
    at[128] = T
    assert any(bool(((at[min(q + 32, 128)] < 1.17549435e-38) & (at[q] != 0)).any()) for q in (0, 32, 64))
    assert not at[96].any()
    got, _, _ = hip_absgrad(sc, maps, device, with_backward=False)
    assert not got[96:].any() and not absolute[96:].gt(1e-30).any() and bool((got[:8] > 0).all())


def test_absolute_sums_exceed_the_signed_ones_strictly_where_gradients_cancel(device):
    """grad_image has mixed signs: for most Gaussians the per-pixel terms cancel in the signed sum.  A kernel that returned
    the magnitude of the signed sum would fail here."""
    for name in ("frame", "stack"):
        sc, maps, (signed, absolute, scale) = scene_and_maps(name, "colour")
        got, g_mean, _ = hip_absgrad(sc, maps, device)
        margin = got.cpu().double() - g_mean.cpu().double().abs() - 2 * TOL * (1.0 + scale)
        assert int((margin > 0).any(dim=1).sum()) >= sc["start"].shape[0] // 2, name
        assert float((got.cpu().double() / g_mean.cpu().double().abs().clamp_min(1e-30)).median()) > 1.5, name


def test_two_calls_give_the_same_bits_with_exact_and_with_capture_safe_bins(device):
    for name, variant in (("frame", "colour"), ("wide", "all_three"), ("underflow", "colour"), ("one_every", "background")):
        sc, maps, _ = scene_and_maps(name, variant)
        a, _, bins = hip_absgrad(sc, maps, device, with_backward=False)
        b, _, _ = hip_absgrad(sc, maps, device, with_backward=False)
        assert torch.equal(a, b), name
        c, _, cap_bins = hip_absgrad(sc, maps, device, capacity=2 * bins.n_tile_pairs + 100, with_backward=False)  # ample
        assert not cap_bins.overflowed() and torch.equal(a, c), name


def test_a_capacity_that_cuts_the_list_gives_zeros_past_it(device):
    """Capture-safe binning lists whole Gaussians, front to back, while their entries fit: the listed Gaussians read what
    they read on the truncated scene, the others exactly 0."""
    sc, maps, _ = scene_and_maps("frame", "colour")
    _, _, bins = hip_absgrad(sc, maps, device, with_backward=False)
    tile_off = bins.tile_off.cpu()
    capacity = int(tile_off[25]) + 1  # cuts inside Gaussian 25
    listed = int((tile_off[1:] <= capacity).sum())
    assert 20 <= listed < 40
    got, _, cap_bins = hip_absgrad(sc, maps, device, capacity=capacity, with_backward=False)
    assert cap_bins.overflowed()
    cut = {k: (v[:listed] if torch.is_tensor(v) and v.shape[:1] == (40,) else v) for k, v in sc.items()}
    want, _, _ = hip_absgrad(cut, maps, device, with_backward=False)
    assert torch.equal(got[:listed], want) and not got[listed:].any() and int((want > 0).all(dim=1).sum()) >= 15


def test_argument_checks(device):
    from simplegaussiansplat_tk71_amd import raster

    sc, maps, _ = scene_and_maps("frame", "colour")
    d = [sc[k].to(device) for k in KEYS]
    bins = raster.bin_tiles(d[0], d[1], sc["width"], sc["height"])
    _, ckpt = raster.blend_forward(bins, *d, with_checkpoints=True)
    wimg = sc["wimg"].to(device)
    with pytest.raises(RuntimeError, match="t_ckpt: too small"):
        raster.blend_absgrad(bins, *d, ckpt[:256], wimg)
    with pytest.raises(RuntimeError, match="grad_image: expected shape"):
        raster.blend_absgrad(bins, *d, ckpt, wimg[1:])
    with pytest.raises(RuntimeError, match="absgrad: expected"):
        raster.blend_absgrad(bins, *d, ckpt, wimg, out=torch.zeros(40, 3, device=device))
    with pytest.raises(RuntimeError, match="no CPU path"):
        raster.blend_absgrad(bins, *d, ckpt, sc["wimg"])


# ---- the Functions --------------------------------------------------------------------------------------------------------
def _leaves(sc, device):
    st = {k: sc[k].to(device) for k in ("boxsize", "start", "end")}
    leaves = [sc[k].to(device).float().clone().requires_grad_(True) for k in ("mean", "vinv", "opacity", "l_d")]
    return st, leaves


def test_function_fills_the_buffer_and_leaves_the_gradients_bit_for_bit(device):
    import cuda_kernel as ck
    from simplegaussiansplat_tk71_amd import raster

    sc, maps, (_, absolute, scale) = scene_and_maps("subpixel", "colour")
    n = sc["start"].shape[0]
    st, leaves = _leaves(sc, device)
    wimg = sc["wimg"].to(device)
    batch = torch.tensor([n], device=device)

    def step(*extra):
        img = ck.custom_autograd_grouped_cumprod.apply(st["boxsize"], batch, st["start"], st["end"], *leaves, sc["width"], sc["height"], *extra)
        return (img.detach(), *torch.autograd.grad((img * wimg).sum(), leaves))

    plain = step()  # the ten arguments of the reference
    buf = ck.absgrad_buffer(st["start"])
    assert buf.shape == (n, 2) and buf.dtype == torch.float32 and not buf.any()
    with_buf = step(buf)
    with_none = step(None)
    for a, b, c in zip(plain, with_buf, with_none):
        assert torch.equal(a, b) and torch.equal(a, c)
    bins = raster.bin_tiles(st["start"], st["end"], sc["width"], sc["height"])
    args = [st["start"], st["end"], *(t.detach() for t in leaves)]
    _, ckpt = raster.blend_forward(bins, *args, with_checkpoints=True)
    assert torch.equal(buf, raster.blend_absgrad(bins, *args, ckpt, wimg)) and not buf.requires_grad
    parity(buf, absolute, scale, "Function absgrad")
    with pytest.raises(RuntimeError, match="absgrad: expected"):
        step(torch.zeros(n, 3, device=device))
    with pytest.raises(RuntimeError, match="absgrad: expected"):
        step(torch.zeros(n, 2))
    with pytest.raises(TypeError, match="at most one"):
        step(buf, buf)


def test_render_fills_the_buffer_and_leaves_the_gradients_bit_for_bit(device):
    import cuda_kernel as ck
    from simplegaussiansplat_tk71_amd import raster

    sc, maps, (_, absolute, scale) = scene_and_maps("subpixel", "all_three")
    st, leaves = _leaves(sc, device)
    z = maps["depth"].to(device).clone().requires_grad_(True)
    bg = maps["background"].to(device).clone().requires_grad_(True)
    g_i, g_d, g_a = (maps[k].to(device) for k in ("grad_image", "grad_depth", "grad_alpha"))

    def step(buf):
        img, dep, alp = ck.render(st["start"], st["end"], *leaves, z, sc["width"], sc["height"], bg, absgrad=buf)
        loss = (img * g_i).sum() + (dep * g_d).sum() + (alp * g_a).sum()
        return (img.detach(), dep.detach(), alp.detach(), *torch.autograd.grad(loss, [*leaves, z, bg]))

    plain = step(None)
    buf = ck.absgrad_buffer(st["start"])
    for a, b in zip(plain, step(buf)):
        assert torch.equal(a, b)
    assert len(plain) == 9  # three maps, the four gradients, g_z and g_bg
    bins = raster.bin_tiles(st["start"], st["end"], sc["width"], sc["height"])
    args = [st["start"], st["end"], *(t.detach() for t in leaves)]
    ckpt = raster.blend_forward_depth(bins, *args, z.detach(), bg.detach(), with_checkpoints=True)[3]
    assert torch.equal(buf, raster.blend_absgrad_depth(bins, *args, z.detach(), ckpt, g_i, g_d, g_a, bg.detach()))
    parity(buf, absolute, scale, "render absgrad")
    # only the depth map is used: the other two outputs hand their kernels no gradient at all
    buf2 = ck.absgrad_buffer(st["start"])
    dep = ck.render(st["start"], st["end"], *leaves, z, sc["width"], sc["height"], bg, absgrad=buf2)[1]
    torch.autograd.grad((dep * g_d).sum(), leaves[0])
    assert torch.equal(buf2, raster.blend_absgrad_depth(bins, *args, z.detach(), ckpt, None, g_d, None, bg.detach())) and bool(buf2.any())


def test_captured_step_fills_the_buffer_with_the_eager_bits(device):
    """Forward + backward in ONE HIP graph (GraphedStep), replayed twice on moved Gaussians: the buffer — written by a kernel
    on the capture stream — holds the bits of the eager step each time."""
    import cuda_kernel as ck

    sc, maps, _ = scene_and_maps("subpixel", "colour")
    n = sc["start"].shape[0]
    st, leaves = _leaves(sc, device)
    wimg = sc["wimg"].to(device)
    batch = torch.tensor([n], device=device)
    graph_buf, eager_buf = ck.absgrad_buffer(st["start"]), ck.absgrad_buffer(st["start"])

    def body(buf, *ls):
        img = ck.custom_autograd_grouped_cumprod.apply(st["boxsize"], batch, st["start"], st["end"], *ls, sc["width"], sc["height"], buf)
        return (img * wimg).sum(), img

    step = ck.GraphedStep(lambda *ls: body(graph_buf, *ls), leaves, capacity=16 * n + 1024)
    assert not ck.capacity_exceeded()
    for shift in (0.25, -0.4):
        with torch.no_grad():
            leaves[0].add_(shift)
            leaves[2].mul_(0.9)
            graph_buf.fill_(-1.0)
        (_, img), grads = step.replay()
        torch.cuda.synchronize()
        assert not ck.capacity_exceeded()
        loss, e_img = body(eager_buf, *leaves)
        e_grads = torch.autograd.grad(loss, leaves)
        assert torch.equal(img, e_img.detach())
        for a, b in zip(grads, e_grads):
            assert torch.equal(a, b)
        assert torch.equal(graph_buf, eager_buf) and bool((graph_buf > 0).any()) and bool((graph_buf >= 0).all())
