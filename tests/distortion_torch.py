"""Dense float64 oracle of the depth distortion map (cuda_kernel.render(distortion=True), csrc/gcp_distort.hip): the renderer
of tests/test_render_depth_gpu.py with the fourth map, differentiable by autograd, and the O(n^2) definition it must equal.
A helper, not a test module."""
import torch
import torch.nn.functional as F


def dense_weights(start, end, mean, vinv, opacity, width, height, dtype=torch.float64):
    """-> (w [N, H+1, W+1]: the colour weight T_k o_k g_k of every Gaussian at every pixel, 0 outside its box and for a dropped
    pair (inclusive product exactly 0), T_N [H+1, W+1]).  Differentiable in vinv, opacity (and a float mean)."""
    ys = torch.arange(height + 1, dtype=dtype)[:, None]
    xs = torch.arange(width + 1, dtype=dtype)[None, :]
    T = torch.ones(height + 1, width + 1, dtype=dtype)
    mean_t = mean.to(dtype) if mean.requires_grad else mean.to(dtype).tolist()
    ws = []
    for i in range(start.shape[0]):
        x0, y0, x1, y1 = int(start[i, 0]), int(start[i, 1]), int(end[i, 0]), int(end[i, 1])
        if x1 < x0 or y1 < y0:
            ws.append(torch.zeros(height + 1, width + 1, dtype=dtype))
            continue
        dx = xs[:, x0:x1 + 1] - mean_t[i][0]
        dy = ys[y0:y1 + 1, :] - mean_t[i][1]
        a, b, c, d = vinv[i, 0, 0], vinv[i, 0, 1], vinv[i, 1, 0], vinv[i, 1, 1]
        g = torch.exp(-0.5 * ((dx * a + dy * c) * dx + (dx * b + dy * d) * dy))
        Tb = T[y0:y1 + 1, x0:x1 + 1]
        factor = 1.0 - opacity[i, 0] * g
        keep = Tb * factor != 0
        w = torch.where(keep, Tb * opacity[i, 0] * g, torch.zeros((), dtype=dtype))
        ws.append(F.pad(w, (x0, width - x1, y0, height - y1)))
        T = T * F.pad(torch.where(keep, factor, factor.detach()), (x0, width - x1, y0, height - y1), value=1.0)
    if not ws:
        return torch.zeros(0, height + 1, width + 1, dtype=dtype), T
    return torch.stack(ws), T


def dense_render_distortion(start, end, mean, vinv, opacity, l_d, z, width, height, background=None, dtype=torch.float64):
    """-> (image, depth, alpha, dist, a_n), the first three as `dense_render_depth` of tests/test_render_depth_gpu.py, and
      dist = 2 sum_k w_k (z_k A_{k-1} - B_{k-1}),  A_k = sum_{j<=k} w_j,  B_k = sum_{j<=k} w_j z_j,  a_n = A_N
    by the recurrence, front to back in list order."""
    w, T = dense_weights(start, end, mean, vinv, opacity, width, height, dtype)
    img = torch.einsum("nhw,nc->hwc", w, l_d.to(dtype))
    dep = torch.einsum("nhw,n->hw", w, z.to(dtype))
    A = torch.zeros(height + 1, width + 1, dtype=dtype)
    B = torch.zeros(height + 1, width + 1, dtype=dtype)
    dist = torch.zeros(height + 1, width + 1, dtype=dtype)
    for wi, zi in zip(w.unbind(0), z.to(dtype).unbind(0)):  # (unbind: one backward node for all layers, not a full-size one each)
        dist = dist + 2.0 * wi * (zi * A - B)
        A = A + wi
        B = B + wi * zi
    if background is not None:
        img = img + T[:, :, None] * background[None, None, :]
    return img, dep, 1.0 - T, dist, A


def distortion_pairs(w, z):
    """The O(n^2) definition per pixel: sum_{i,j} w_i w_j |z_i - z_j|;  w [N, H+1, W+1], z [N]."""
    n = w.shape[0]
    D = (z[:, None] - z[None, :]).abs().to(w.dtype)
    flat = w.reshape(n, -1)
    return (flat * (D @ flat)).sum(0).reshape(w.shape[1:])
