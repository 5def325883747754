"""Dense float64 reference of the median depth map (cuda_kernel.render(median=True), csrc/gcp_median.hip): per pixel the exclusive
transmittance and the weight of every Gaussian, the reference's pick, and — the median being a discontinuous choice — the SET of
picks a float32 walk may legitimately make.  A helper, not a test module.

With eps = tests.util.TOL (the project's absolute bar on transmittance) and float64 T, w, per pixel:
  must = contributing pairs (w != 0) with w >= 1e-30 and T > 0.5 + eps       may = contributing pairs with T > 0.5 - eps
A pick k is admissible iff k is in `may` and k >= max(must) (no pick, -1, iff `must` is empty); the pixel is AMBIGUOUS iff
max(may) != max(must).  On every other pixel the only admissible pick is the reference's."""
import torch

from tests.util import TOL

W_MIN = 1e-30  # a float64 weight below this may underflow in float32: the pair may or may not contribute there


def dense_pairs(start, end, mean, vinv, opacity, width, height):
    """-> (w [N, H+1, W+1], T [N, H+1, W+1]) in float64: the colour weight T_k o_k g_k of every Gaussian at every pixel (0 outside
    its box and for a dropped pair: inclusive product exactly 0) and the EXCLUSIVE transmittance T_k in front of it, by the
    pair rule of tests/distortion_torch.dense_weights."""
    dtype = torch.float64
    n = start.shape[0]
    ys = torch.arange(height + 1, dtype=dtype)[:, None]
    xs = torch.arange(width + 1, dtype=dtype)[None, :]
    T = torch.ones(height + 1, width + 1, dtype=dtype)
    w_all = torch.zeros(n, height + 1, width + 1, dtype=dtype)
    T_all = torch.ones(n, height + 1, width + 1, dtype=dtype)
    mean_t, vinv, opacity = mean.to(dtype).tolist(), vinv.to(dtype), opacity.to(dtype)
    for i in range(n):
        T_all[i] = T
        x0, y0, x1, y1 = int(start[i, 0]), int(start[i, 1]), int(end[i, 0]), int(end[i, 1])
        if x1 < x0 or y1 < y0:
            continue
        dx = xs[:, x0:x1 + 1] - mean_t[i][0]
        dy = ys[y0:y1 + 1, :] - mean_t[i][1]
        a, b, c, d = vinv[i, 0, 0], vinv[i, 0, 1], vinv[i, 1, 0], vinv[i, 1, 1]
        g = torch.exp(-0.5 * ((dx * a + dy * c) * dx + (dx * b + dy * d) * dy))
        Tb = T[y0:y1 + 1, x0:x1 + 1]
        factor = 1.0 - opacity[i, 0] * g
        keep = Tb * factor != 0
        w_all[i, y0:y1 + 1, x0:x1 + 1] = torch.where(keep, Tb * opacity[i, 0] * g, torch.zeros((), dtype=dtype))
        T = T.clone()
        T[y0:y1 + 1, x0:x1 + 1] = Tb * factor
    return w_all, T_all


def _last(mask):
    """[N, ...] bool -> the largest n with mask[n], -1 where none"""
    n = mask.shape[0]
    idx = torch.arange(n).reshape(n, *([1] * (mask.dim() - 1)))
    return torch.where(mask, idx, torch.full((), -1, dtype=torch.long)).amax(0) if n else torch.full(mask.shape[1:], -1, dtype=torch.long)


class MedianReference:
    """The float64 picks of one scene (Gaussians in list order): `index` [H+1, W+1] (long, -1: no contributing pair), the
    admissible sets and the ambiguous pixels."""

    def __init__(self, sc, eps=TOL):
        self.w, self.T = dense_pairs(sc["start"], sc["end"], sc["mean"], sc["vinv"], sc["opacity"], sc["width"], sc["height"])
        contributing = self.w != 0
        self.index = _last(contributing & (self.T > 0.5))
        self.may = contributing & (self.T > 0.5 - eps)
        self.max_must = _last(contributing & (self.w >= W_MIN) & (self.T > 0.5 + eps))
        self.max_may = _last(self.may)
        self.ambiguous = self.max_may != self.max_must
        self.crossing = (self.T.amin(0) if self.T.shape[0] else torch.ones_like(self.index, dtype=torch.float64)) <= 0.5

    def ambiguous_share(self):
        return float(self.ambiguous.double().mean())

    def median(self, z):
        """z [N] -> the reference's map, float64"""
        zz = torch.cat([z.double(), torch.zeros(1, dtype=torch.float64)])  # index -1 reads the 0 at the end
        return zz[self.index]

    def check(self, index, what=""):
        """The kernel's index map (int, on the CPU) against the rule above."""
        index = index.long()
        assert index.shape == self.index.shape, what
        assert int(index.min()) >= -1 and int(index.max()) < max(self.w.shape[0], 1), what
        clear = ~self.ambiguous
        wrong = clear & (index != self.index)
        assert not bool(wrong.any()), (what, "unambiguous pixels with another pick", int(wrong.sum()), torch.nonzero(wrong)[:4].tolist())
        picked = index >= 0
        in_may = torch.zeros_like(picked)
        if self.w.shape[0]:
            in_may = torch.gather(self.may, 0, index.clamp(min=0)[None])[0] & picked
        ok = torch.where(picked, in_may & (index >= self.max_must), self.max_must < 0)
        assert bool(ok.all()), (what, "inadmissible picks", int((~ok).sum()), torch.nonzero(~ok)[:4].tolist())


def scatter_sum(index, G, n):
    """float64 sum of G over the pixels whose index is g, and of |G| (the condition scale), per Gaussian -> ([n], [n])"""
    index, G = index.reshape(-1).long(), G.reshape(-1).double()
    sel = index >= 0
    out, scale = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    out.index_add_(0, index[sel], G[sel])
    scale.index_add_(0, index[sel], G[sel].abs())
    return out, scale
