"""The blend's four maps and every leaf's gradient in closed dense form, with the CONDITION SCALE of every Gaussian's row: what
tests/test_blend_rows.py checks against the autograd oracles and tests/test_blend_rows_gpu.py holds the kernels to
(csrc/gcp_blend.hip k_blend_fwd_depth / k_blend_bwd_depth, csrc/gcp_distort.hip).  A helper, not a test module.

Everything is [n, P] (Gaussians in list order x pixels of the (H+1) x (W+1) frame), without autograd; the only Python loops
over layers are the recursions.  Per pixel, with m_k the box as a mask, g_k the Gaussian, a_k = m_k o_k g_k, T_k the exclusive
product of (1 - a_j), a pair kept iff it is inside the box and its inclusive product T_k (1 - a_k) is not exactly 0
(w_k = T_k a_k for a kept pair, 0 otherwise: the rule of `dense_render_depth`), T_N the product behind the list:
  render      c_k = gI . l_k + gD z_k,   R_N = gI . bg - gA where T_N != 0, else 0
  distortion  c_k = 2 G sum_j w_j |z_k - z_j|  (z non-decreasing in list order),   R_N = 0
  both        R_{k-1} = R_k + a_k (c_k - R_k) over the kept pairs,   d_k = c_k - R_k
              dL/do_k = sum_p T_k g_k d_k,   common = T_k a_k d_k,   dL/dvinv_k = -1/2 sum_p common [dx dx, dx dy; dx dy, dy dy]
              dL/dmean_k = sum_p common (dx A + dy (B + C) / 2,  dy D + dx (B + C) / 2)
  render      dL/dl_k = sum_p w_k gI,  dL/dz_k = sum_p w_k gD,  dL/dbg = sum_p T_N gI
  distortion  dL/dz_k = sum_p 2 G w_k (sum_{j<k} w_j - sum_{j>k} w_j)
The scale of a row is the same expression with every signed term replaced by its absolute value: the recursion on |c_j| and
|R_N|, |c_k| + R_k for c_k - R_k, |gI|, |gD|, |dx dy| in the pixel sums.  The distortion's c_k is a sum of one sign, so its
scale is itself: in units of the depth SPREAD, not of the depth.
dtype=torch.float32 runs the same formulation in float32 — the distortion in this PAIR form, not the kernels' prefix form
z_k A_{k-1} - B_{k-1} — and returns it as float64: what float32 can deliver."""
import torch

FLT_MIN = 1.17549435e-38


class Rows(dict):
    """leaf -> (value, scale), each float64 with the leaf's shape"""


def _back_recursion(a, keep, c, R_N):
    """R behind every entry [n, P]: R_{k-1} = R_k + a_k (c_k - R_k) over the kept pairs, from R_N behind the list"""
    out = torch.empty_like(c)
    R = R_N
    for k in range(c.shape[0] - 1, -1, -1):
        out[k] = R
        R = torch.where(keep[k], R + a[k] * (c[k] - R), R)
    return out


def _geometry_rows(Tw, keep, g, a, d, dx, dy, v, absolute):
    """the rows every c_k shares: opacity, vinv, mean; `Tw` is T_k"""
    zero = torch.zeros((), dtype=Tw.dtype)
    tg = torch.where(keep, Tw * g, zero)
    common = torch.where(keep, Tw * a, zero) * d
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    A, B, C, D = v[:, 0, 0, None], v[:, 0, 1, None], v[:, 1, 0, None], v[:, 1, 1, None]
    half = 0.5 * (B + C)
    xy = (common * f(dx * dy)).sum(1)
    sign = 0.5 if absolute else -0.5
    vinv = sign * torch.stack([(common * dx * dx).sum(1), xy, xy, (common * dy * dy).sum(1)], 1).reshape(-1, 2, 2)
    if absolute:
        mean = torch.stack([(common * ((dx * A).abs() + (dy * half).abs())).sum(1), (common * ((dy * D).abs() + (dx * half).abs())).sum(1)], 1)
    else:
        mean = torch.stack([(common * (dx * A + dy * half)).sum(1), (common * (dy * D + dx * half)).sum(1)], 1)
    return {"opacity": (tg * d).sum(1)[:, None], "vinv": vinv, "mean": mean}


def blend_rows(sc, z, bg, gI, gD, gA, gDist, dtype=torch.float64):
    """-> (render: Rows over vinv, opacity, l_d, z, bg, mean;  distortion: Rows over mean, vinv, opacity, z;
           maps: image [H+1, W+1, 3], depth, alpha, dist [H+1, W+1], depth_scale = sum w |z|, dist_scale = dist, T_N),
    everything float64 whatever `dtype` computed it.  `sc`: a scene of tests/util.make_scene's keys; z [n] non-decreasing for
    the distortion's rows to be those of the order-based form; bg float[3]; gI [H+1, W+1, 3], gD, gA, gDist [H+1, W+1]."""
    dt = dtype
    H1, W1 = sc["height"] + 1, sc["width"] + 1
    n = sc["start"].shape[0]
    ys, xs = torch.meshgrid(torch.arange(H1, dtype=dt), torch.arange(W1, dtype=dt), indexing="ij")
    xs, ys = xs.reshape(1, -1), ys.reshape(1, -1)
    mean, v = sc["mean"].to(dt), sc["vinv"].to(dt)
    o, l_d, z, bg = sc["opacity"].to(dt).reshape(n, 1), sc["l_d"].to(dt), z.to(dt), bg.to(dt)
    gI, gD, gA, G = gI.to(dt).reshape(-1, 3), gD.to(dt).reshape(1, -1), gA.to(dt).reshape(1, -1), gDist.to(dt).reshape(1, -1)
    st, en = sc["start"].to(dt), sc["end"].to(dt)
    inside = (xs >= st[:, 0:1]) & (xs <= en[:, 0:1]) & (ys >= st[:, 1:2]) & (ys <= en[:, 1:2])
    dx, dy = xs - mean[:, 0:1], ys - mean[:, 1:2]
    A, B, C, D = v[:, 0, 0, None], v[:, 0, 1, None], v[:, 1, 0, None], v[:, 1, 1, None]
    g = torch.exp(-0.5 * ((dx * A + dy * C) * dx + (dx * B + dy * D) * dy))
    zero, one = torch.zeros((), dtype=dt), torch.ones(1, xs.shape[1], dtype=dt)
    a = torch.where(inside, o * g, zero)
    T_incl = torch.cumprod(1.0 - a, 0)
    T = torch.cat([one, T_incl[:-1]])
    T_N = T_incl[-1:]
    keep = inside & (T_incl != 0)
    w = torch.where(keep, T * a, zero)

    def geometry(c, c_abs, R_N, R_N_abs):
        d = c - _back_recursion(a, keep, c, R_N)
        d_abs = c_abs + _back_recursion(a, keep, c_abs, R_N_abs)
        val = _geometry_rows(T, keep, g, a, d, dx, dy, v, False)
        sca = _geometry_rows(T, keep, g, a, d_abs, dx, dy, v, True)
        return {k: (val[k], sca[k]) for k in val}

    # the three maps of the render
    live = T_N != 0
    render = geometry(l_d @ gI.T + gD * z[:, None], l_d.abs() @ gI.abs().T + gD.abs() * z.abs()[:, None],
                      torch.where(live, (gI @ bg)[None] - gA, zero)[0], torch.where(live, (gI.abs() @ bg.abs())[None] + gA.abs(), zero)[0])
    render["l_d"] = (w @ gI, w @ gI.abs())
    render["z"] = ((w * gD).sum(1), (w * gD.abs()).sum(1))
    render["bg"] = ((T_N @ gI)[0], (T_N @ gI.abs())[0])
    # the distortion, in its pair form
    assert bool((z[1:] >= z[:-1]).all()), "the distortion's order-based form needs depths in list order"
    s = (z[:, None] - z[None, :]).abs() @ w                      # sum_j w_j |z_k - z_j|   [n, P]
    distortion = geometry(2.0 * G * s, 2.0 * G.abs() * s, zero.expand(xs.shape[1]), zero.expand(xs.shape[1]))
    front = torch.cumsum(w, 0) - w                                # sum_{j<k} w_j
    behind = torch.flip(torch.cumsum(torch.flip(w, [0]), 0), [0]) - w
    distortion["z"] = ((2.0 * G * w * (front - behind)).sum(1), (2.0 * G.abs() * w * (front + behind)).sum(1))
    dist = (w * s).sum(0)
    maps = {"image": (w.T @ l_d + T_N.T * bg[None]).reshape(H1, W1, 3), "depth": (w * z[:, None]).sum(0).reshape(H1, W1),
            "alpha": (1.0 - T_N).reshape(H1, W1), "dist": dist.reshape(H1, W1), "depth_scale": (w * z.abs()[:, None]).sum(0).reshape(H1, W1),
            "dist_scale": dist.reshape(H1, W1), "T_N": T_N.reshape(H1, W1)}
    shapes = {"opacity": sc["opacity"].shape, "z": (n,)}
    as64 = lambda name, t: t.double().reshape(shapes.get(name, t.shape))  # noqa: E731
    return (Rows({k: tuple(as64(k, t) for t in v2) for k, v2 in render.items()}),
            Rows({k: tuple(as64(k, t) for t in v2) for k, v2 in distortion.items()}), {k: t.double() for k, t in maps.items()})
