"""The torch / numpy formulation of density control on the device (include/grouped_cumprod_hip.h, gcp_densify_*), which
the kernels of csrc/gcp_densify.hip are tested against: the plan (one action per Gaussian from the state before the pass,
prune test on the output rows), the row gather with Adam's moments, the split samples from a numpy Philox4x32-10, and the
fixture scene that reaches every branch of the plan.  CPU tensors throughout."""
import numpy as np
import torch

KEEP, CLONE, SPLIT = 0, 1, 2          # action
SURVIVOR, FRESH, CHILD = 0, 1, 2      # kind
NAMES = ("mean", "variance_q", "variance_scale", "opacity", "color")

# the fixture's thresholds: all exactly representable in float32 where a case sits ON them
HYPER = {"grad_threshold": 0.5, "dense_extent": 0.1, "prune_extent": 1.0, "min_opacity": 0.005}
BRANCHES = ("keep", "clone", "split", "split_children_pruned_by_scale", "prune_by_opacity", "prune_by_scale", "hot_without_views",
            "exactly_at_threshold", "clone_pruned_by_opacity", "split_parent_over_prune_extent_children_under")


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11).  counter (..., 4), key (..., 2), anything that converts to uint32 -> (..., 4) uint32."""
    c = [np.asarray(counter, dtype=np.uint64)[..., k] & 0xFFFFFFFF for k in range(4)]
    key = np.asarray(key, dtype=np.uint64)
    k0, k1 = key[..., 0] & 0xFFFFFFFF, key[..., 1] & 0xFFFFFFFF
    m0, m1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]  # 32 x 32 bits: fits uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack(c, axis=-1).astype(np.uint32)


def split_normals(seed, parent, child):
    """z (n, 3) float64 of the children (parent[i], child[i]): key (seed_lo, seed_hi), counter (parent, child, 0, 0),
    u_k = (r_k + 0.5) 2^-32, Box-Muller."""
    parent, child = np.asarray(parent, dtype=np.uint64), np.asarray(child, dtype=np.uint64)
    zero = np.zeros_like(parent)
    seed = int(seed) & (2 ** 64 - 1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), (*parent.shape, 2))
    r = philox4x32_10(np.stack([parent, child, zero, zero], axis=-1), key)
    u = (r.astype(np.float64) + 0.5) * 2.0 ** -32
    ra, rb = np.sqrt(-2 * np.log(u[..., 0])), np.sqrt(-2 * np.log(u[..., 2]))
    return np.stack([ra * np.cos(2 * np.pi * u[..., 1]), ra * np.sin(2 * np.pi * u[..., 1]), rb * np.cos(2 * np.pi * u[..., 3])], axis=-1)


def plan(norm, views, log_scale, opacity, grad_threshold, dense_extent, prune_extent, min_opacity, n_split=2):
    """-> dict: count, action, offset (N + 1), M, src_row (M), kind (M), child (M).  float32 arithmetic, as the kernel's."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    n = norm.numel()
    g = norm / views.clamp_min(1).to(torch.float32)
    hot = (views > 0) & (g >= f32(grad_threshold))
    s = torch.exp(log_scale).reshape(n, 3).max(dim=1).values if n else torch.zeros(0)
    split = hot & (s > f32(dense_extent))
    clone = hot & ~split
    out_s = torch.where(split, s / (f32(0.8) * n_split), s)
    pruned = (torch.sigmoid(opacity.reshape(-1)) < f32(min_opacity)) | (out_s > f32(prune_extent))
    action = torch.where(split, SPLIT, torch.where(clone, CLONE, KEEP)).to(torch.uint8)
    count = torch.where(pruned, 0, torch.where(split, n_split, torch.where(clone, 2, 1))).to(torch.int32)
    offset = torch.cat([torch.zeros(1, dtype=torch.int64), count.long().cumsum(0)]).to(torch.int32)
    src_row = torch.repeat_interleave(torch.arange(n), count.long())
    child = torch.arange(src_row.numel()) - offset[src_row].long()
    kind = torch.where(split[src_row], CHILD, torch.where(clone[src_row] & (child > 0), FRESH, SURVIVOR)).to(torch.uint8)
    return {"count": count, "action": action, "offset": offset, "M": int(offset[-1]), "src_row": src_row.to(torch.int32), "kind": kind,
            "child": child, "pruned": pruned, "hot": hot, "g": g}


def gather(pl, tensor, moments=False):
    """Rows of a per-Gaussian tensor after the pass; moments=True: rows that are not survivors are 0.0."""
    out = tensor[pl["src_row"].long()].clone()
    if moments:
        out[pl["kind"] != SURVIVOR] = 0.0
    return out


def split_children(pl, mean, variance_q, variance_scale, seed, n_split=2):
    """-> (rows (n,) of the split children, mean (n, 3), log scale (n, 3)) in float64 from the numpy Philox draws."""
    rows = torch.nonzero(pl["kind"] == CHILD).reshape(-1)
    parent = pl["src_row"].long()[rows]
    z = torch.from_numpy(split_normals(seed, parent.numpy(), pl["child"][rows].numpy()))
    sigma = torch.exp(variance_scale.double()[parent])
    q = variance_q.double()[parent]
    q = q / q.norm(dim=1, keepdim=True).clamp_min(1e-8)
    return rows, mean.double()[parent] + torch.einsum("nij,nj->ni", rotmat(q), sigma * z), torch.log(sigma / (0.8 * n_split))


def rotmat(q):
    """(N, 4) unit quaternions (x, y, z, w) -> (N, 3, 3), as gs_model.qvec_to_rotmat_batch."""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    r0 = torch.stack([1 - 2 * (y**2 + z**2), 2 * (x * y - w * z), 2 * (x * z + w * y)], dim=1)
    r1 = torch.stack([2 * (x * y + w * z), 1 - 2 * (x**2 + z**2), 2 * (y * z - w * x)], dim=1)
    r2 = torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x**2 + y**2)], dim=1)
    return torch.stack([r0, r1, r2], dim=1)


def scene(n, n_coeff=9, seed=0):
    """A scene of n Gaussians with its statistic, every Gaussian in one of BRANCHES (`branch`, by index into it) under HYPER
    with n_split = 2, each decision with a margin of >= 8 % except the case that sits exactly on the gradient threshold."""
    g = torch.Generator().manual_seed(1000 * seed + n)
    rand = lambda *shape: torch.rand(*shape, generator=g)  # noqa: E731
    branch = torch.randint(0, len(BRANCHES), (n,), generator=g)
    is_ = lambda *names: torch.isin(branch, torch.tensor([BRANCHES.index(k) for k in names]))  # noqa: E731
    views = torch.randint(1, 6, (n,), generator=g).to(torch.int32)
    hot = is_("clone", "split", "split_children_pruned_by_scale", "clone_pruned_by_opacity", "split_parent_over_prune_extent_children_under")
    norm = views.float() * torch.where(hot, 1.0 + rand(n), 0.1 * rand(n))
    views[is_("hot_without_views")] = 0
    norm[is_("hot_without_views")] = 5.0
    views[is_("exactly_at_threshold")] = 4
    norm[is_("exactly_at_threshold")] = 2.0  # g = 0.5 = the threshold: hot (>=), small: a clone
    largest = torch.full((n,), 0.05)
    largest[is_("split")] = 0.3
    largest[is_("split_children_pruned_by_scale")] = 2.0   # children 1.25 > 1.0
    largest[is_("prune_by_scale")] = 1.5
    largest[is_("split_parent_over_prune_extent_children_under")] = 1.2  # children 0.75
    largest = largest * (0.92 + 0.16 * rand(n))
    scale = largest[:, None] * (0.3 + 0.6 * rand(n, 3))
    scale[torch.arange(n), torch.randint(0, 3, (n,), generator=g)] = largest
    opacity = torch.logit(0.1 + 0.8 * rand(n, 1))
    opacity[is_("prune_by_opacity", "clone_pruned_by_opacity")] = -7.0  # sigmoid = 9.1e-4
    return {"mean": torch.randn(n, 3, generator=g), "variance_q": torch.randn(n, 4, generator=g), "variance_scale": torch.log(scale),
            "opacity": opacity, "color": torch.randn(n, n_coeff, 3, generator=g), "norm": norm, "views": views, "branch": branch}
