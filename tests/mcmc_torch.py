"""The torch / numpy formulation of MCMC density control (include/grouped_cumprod_hip.h, gcp_mcmc_*), which the kernels of
csrc/gcp_mcmc.hip are tested against: the integer weights, the draw of a source per slot from a numpy Philox4x32-10, the
relocated opacity and scale in float64, the row gather with Adam's moments, the position noise in float64, and the fixture
scene.  CPU tensors throughout."""
import math

import numpy as np
import torch

from tests.density_torch import philox4x32_10, rotmat

NAMES = ("mean", "variance_q", "variance_scale", "opacity", "color")
MIN_OPACITY = 0.005
MAX_COPIES = 51
NOISE_DOMAIN, DRAW_DOMAIN = 1, 2  # the Philox counter's last word; 0: the split children of density_torch.split_normals


def weight_levels(n):
    """The largest power of two <= 2^16 with n * W <= 2^31 - 1."""
    w = 1 << 16
    while w > 1 and n * w > 2 ** 31 - 1:
        w >>= 1
    return w


def weights(opacity, min_opacity=MIN_OPACITY, w_max=None):
    """-> (weight int64 (N,), dead bool (N,)); float32 arithmetic, as the kernel's."""
    o = torch.sigmoid(opacity.reshape(-1).float())
    w_max = weight_levels(o.numel()) if w_max is None else w_max
    dead = ~(o > torch.tensor(min_opacity, dtype=torch.float32))
    w = torch.floor(o * float(w_max)).long().clamp(1, w_max)
    return torch.where(dead, 0, w), dead


def _key(seed, shape):
    seed = int(seed) & (2 ** 64 - 1)
    return np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), (*shape, 2))


def draw(cum, n_out, seed):
    """cum: int (N + 1,) exclusive prefix sums of the weights -> dict src_row int32 (M,), times int32 (N,), kind uint8 (M,),
    slot bool (M,).  Counter (r, 0, 0, 2), t = (r0 T) >> 32, source = upper bound of t in cum[1:]."""
    cum = np.asarray(cum, dtype=np.int64)
    n, m, total = cum.size - 1, int(n_out), int(cum[-1])
    slot = np.ones(m, dtype=bool)
    slot[:n] = (cum[1:] == cum[:-1])[:m]
    if total == 0:
        src = (np.arange(m) % max(n, 1)).astype(np.int64)
        times = np.zeros(n, dtype=np.int64)
    else:
        r = np.nonzero(slot)[0].astype(np.uint64)  # only a slot draws: the Philox words of the other rows would be thrown away
        zero = np.zeros_like(r)
        rnd = philox4x32_10(np.stack([r, zero, zero, zero + np.uint64(DRAW_DOMAIN)], axis=-1), _key(seed, r.shape))
        t = (rnd[:, 0].astype(np.uint64) * np.uint64(total)) >> np.uint64(32)
        src = np.arange(m, dtype=np.int64)
        src[slot] = np.searchsorted(cum[1:], t.astype(np.int64), side="right")
        times = np.bincount(src[slot], minlength=n).astype(np.int64)
    kind = np.ones(m, dtype=np.uint8)
    kind[:n] = ~((src[:n] == np.arange(n)) & (times == 0))
    return {"src_row": torch.from_numpy(src.astype(np.int32)), "times": torch.from_numpy(times.astype(np.int32)),
            "kind": torch.from_numpy(kind), "slot": torch.from_numpy(slot)}


def relocated(opacity, log_scale, copies, min_opacity=MIN_OPACITY):
    """Float64 (opacity logit (n, 1), log scale (n, 3)) of sources drawn `copies` (n,) >= 1 times and of their copies:
    n = min(c + 1, 51), o' = 1 - (1 - o)^(1/n), D = sum_{i=1..n} sum_{k<i} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1)."""
    o = torch.sigmoid(opacity.reshape(-1).double())
    n = (copies.long() + 1).clamp(max=MAX_COPIES)
    o_new = 1 - (1 - o) ** (1.0 / n.double())
    denom = torch.zeros_like(o)
    for count in n.unique().tolist():  # the same sum, term by term in the same order, for all rows of one n at once (n <= 51)
        rows = n == count
        x, acc = o_new[rows], torch.zeros(int(rows.sum()), dtype=torch.float64)
        for i in range(1, count + 1):
            for k in range(i):
                acc += math.comb(i - 1, k) * (-1) ** k * x ** (k + 1) / math.sqrt(k + 1)
        denom[rows] = acc
    new_scale = log_scale.double() + torch.log(o / denom)[:, None]
    return torch.logit(o_new.clamp(min_opacity, 1 - 2.0 ** -23))[:, None], new_scale


def gather(dr, tensor, moments=False):
    """Rows of a per-Gaussian tensor after the pass; moments=True: rows that are not survivors are 0.0."""
    out = tensor[dr["src_row"].long()].clone()
    if moments:
        out[dr["kind"] != 0] = 0.0
    return out


def normals(seed, index, domain=NOISE_DOMAIN):
    """z (n, 3) float64 of counter (index, 0, 0, domain): u_k = (r_k + 0.5) 2^-32, Box-Muller as density_torch.split_normals."""
    index = np.asarray(index, dtype=np.uint64)
    zero = np.zeros_like(index)
    r = philox4x32_10(np.stack([index, zero, zero, zero + np.uint64(domain)], axis=-1), _key(seed, index.shape))
    u = (r.astype(np.float64) + 0.5) * 2.0 ** -32
    ra, rb = np.sqrt(-2 * np.log(u[..., 0])), np.sqrt(-2 * np.log(u[..., 2]))
    return np.stack([ra * np.cos(2 * np.pi * u[..., 1]), ra * np.sin(2 * np.pi * u[..., 1]), rb * np.cos(2 * np.pi * u[..., 3])], axis=-1)


def noise(variance_q, variance_scale, opacity, amount, seed, k=100.0, o0=0.005):
    """The displacement (N, 3) in float64: amount * gate * R (s^2 (.) (R^T z))."""
    n = variance_q.shape[0]
    z = torch.from_numpy(normals(seed, np.arange(n)))
    o = torch.sigmoid(opacity.reshape(-1).double())
    gate = 1 / (1 + torch.exp(-k * (o0 - o)))
    q = variance_q.double()
    rot = rotmat(q / q.norm(dim=1, keepdim=True).clamp_min(1e-8))
    s2 = torch.exp(variance_scale.double()) ** 2
    inner = s2 * torch.einsum("nji,nj->ni", rot, z)
    return amount * gate[:, None] * torch.einsum("nij,nj->ni", rot, inner)


def scene(n, n_coeff=4, seed=0, dead_share=0.2):
    """n Gaussians, about `dead_share` of them dead (logit -7: sigmoid 9.1e-4), the rest with sigmoid in [0.01, 0.99]: every
    one at least 8 % away from MIN_OPACITY.  Gaussian 0 is alive, so that a scene of one has a source."""
    g = torch.Generator().manual_seed(1000 * seed + n)
    opacity = torch.logit(0.01 + 0.98 * torch.rand(n, 1, generator=g))
    dead = torch.rand(n, generator=g) < dead_share
    dead[0] = False
    opacity[dead] = -7.0
    return {"mean": torch.randn(n, 3, generator=g), "variance_q": torch.randn(n, 4, generator=g),
            "variance_scale": torch.log(0.03 + 0.3 * torch.rand(n, 3, generator=g)), "opacity": opacity,
            "color": torch.randn(n, n_coeff, 3, generator=g)}
