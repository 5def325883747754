"""Exact k nearest neighbours inside a point cloud on the kernels of csrc/gcp_knn.hip (`nearest_neighbours`) and the initial
scale of every Gaussian from them (`neighbour_scale`): the reference's `kyori2` computed exactly, or upstream 3DGS's rule.
`gs_model.mean_neighbour_distance` — torch.cdist + topk in batches, quadratic, and cancelled where the cloud lies far from its
origin — stays what it was and stays the default of the training example.  GPU float32 tensors only: there is no CPU path."""
import torch

from . import _lib

MAX_K = 16  # of gcp_knn
RULES = ("reference", "3dgs")


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def nearest_neighbours(points, k):
    """(dist2 float32 (N, k), index int32 (N, k)): per point its k nearest OTHER points of `points` (N, 3), 1 <= k <= 16.
    dist2 = (dx dx + dy dy) + dz dz in float32 of the float32 differences; a row is ascending by (dist2, index), so equal
    distances come lower index first and the result is the same bits whatever the order of the points; "other" is by index:
    a duplicate at distance 0 is a neighbour, the point itself is not.  With N <= k the missing entries are index -1,
    dist2 +inf.  Exact, not approximate (gcp_knn: Morton order, two levels of boxes, float32-exact pruning).
    Non-finite coordinates raise ValueError: that check is one device->host read; the C entry point itself reads nothing
    back and can be captured."""
    if not points.is_cuda:
        raise RuntimeError("nearest_neighbours is a HIP kernel: tensors must live on the GPU (no CPU path)")
    if points.dtype != torch.float32:
        raise RuntimeError("nearest_neighbours expects float32 points")
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f"nearest_neighbours expects points (N, 3), got {tuple(points.shape)}")
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k: 1..{MAX_K}, got {k}")
    n, dev = points.shape[0], points.device
    xyz = points.detach().contiguous()
    if not bool(torch.isfinite(xyz).all()):
        raise ValueError("nearest_neighbours: non-finite coordinates")
    dist2 = torch.empty((n, k), dtype=torch.float32, device=dev)
    index = torch.empty((n, k), dtype=torch.int32, device=dev)
    if n == 0:
        return dist2, index
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = torch.empty(lib.gcp_knn_workspace_bytes(n), dtype=torch.uint8, device=dev)
        _lib.check(lib.gcp_knn(xyz.data_ptr(), n, k, index.data_ptr(), dist2.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), "gcp_knn")
    return dist2, index


def neighbour_scale(points, rule="reference", neighbours=3):
    """Linear initial scales (N, 3), the same value on the three axes, from the exact neighbours of `nearest_neighbours`.
    rule="reference": the reference's `kyori2` (what `mean_neighbour_distance(neighbours, points)` states), computed exactly —
        the mean distance to the `neighbours` nearest points, SELF INCLUDED with distance 0:
        sum_{j < neighbours - 1} sqrt(dist2_j) / neighbours.  neighbours >= 2 and neighbours - 1 <= 16.
    rule="3dgs": upstream 3DGS's — sqrt(clamp_min(mean of the 3 smallest dist2, 1e-7)); `neighbours` is ignored.
    A cloud with fewer other points than that uses the neighbours it has (the reference's mean then divides by the cloud's
    size, as its topk does); a cloud of one point has none and raises ValueError."""
    if rule not in RULES:
        raise ValueError(f'rule: "reference" or "3dgs", got {rule!r}')
    if rule == "reference":
        neighbours = int(neighbours)
        if not 2 <= neighbours <= MAX_K + 1:
            raise ValueError(f"neighbours: 2..{MAX_K + 1} (self and up to {MAX_K} others), got {neighbours}")
        k = neighbours - 1
    else:
        k = 3
    dist2, index = nearest_neighbours(points, k)
    n = points.shape[0]
    if n == 1:
        raise ValueError("neighbour_scale: a cloud of one point has no neighbours")
    if n == 0:
        return dist2.new_empty((0, 3))
    have = min(k, n - 1)  # columns that are not padding: the same for every row
    d2 = dist2[:, :have]
    if rule == "reference":
        d = torch.sqrt(d2)
        total = d[:, 0]
        for j in range(1, have):
            total = total + d[:, j]
        scale = total / float(have + 1)
    else:
        total = d2[:, 0]
        for j in range(1, have):
            total = total + d2[:, j]
        scale = torch.sqrt(torch.clamp_min(total / float(have), 1e-7))
    return scale[:, None].repeat(1, 3)
