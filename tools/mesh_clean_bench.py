"""Developer benchmark of the mesh cleaning and the vertex normals (csrc/gcp_meshclean.hip, simplegaussiansplat_tk71_amd/mesh.py);
no effect on bench.py.

Per volume size (256^3 and 512^3), on the fused colour volume of tools/mesh_bench.py's scene (a sphere of radius 0.8 seen by 8 ring
cameras at 1080 x 1920), in ONE run, alternating within every round:

  extract          `TSDFVolume.extract` of the fused volume — the yardstick: cleaning a mesh should not cost more than making it
  components       `mesh.face_components`
  clean            `mesh.clean_mesh` with colours, keep_largest = 50, min_faces = 50 (components + select + compact)
  normals          `mesh.vertex_normals`
  torch_labels     the labels in plain PyTorch on the same GPU: iterated scatter_reduce(amin) over the face edges + pointer
                   jumping, to convergence (the convergence tests are host reads, as a PyTorch user would write them)
  torch_normals    the normals in plain PyTorch: cross products, three index_add_, normalise (float atomics: not reproducible)

The labels and normals of the two formulations are compared.  Times are device events around the call followed by a synchronise;
medians, minima and maxima over the rounds after the warm-up rounds.  `least_bytes` is what a stage must move at the very least,
counted from the shapes (every array read or written once per pass that touches it; the union-find's walks and the gathers' cache
misses come on top); `gb_per_s` is that over the median time.

    python tools/mesh_clean_bench.py [--rounds 7] [--warmup 2] [--sizes 256,512]

One JSON line."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_bench as mb  # noqa: E402
from simplegaussiansplat_tk71_amd import mesh, synthetic  # noqa: E402


def torch_labels(faces, n_vertices):
    """label[v] = the smallest vertex index of v's component, by min-propagation over the face edges + pointer jumping."""
    f = faces.long()
    src = torch.cat([f[:, 0], f[:, 1], f[:, 0], f[:, 2], f[:, 1], f[:, 2]])
    dst = torch.cat([f[:, 1], f[:, 0], f[:, 2], f[:, 0], f[:, 2], f[:, 1]])
    label = torch.arange(n_vertices, device=faces.device)
    rounds = 0
    while True:
        new = label.scatter_reduce(0, dst, label[src], "amin", include_self=True)
        while True:
            jumped = new[new]
            if torch.equal(jumped, new):
                break
            new = jumped
        rounds += 1
        if torch.equal(new, label):
            return label, rounds
        label = new


def torch_normals(vertices, faces):
    f = faces.long()
    a, b, c = vertices[f[:, 0]], vertices[f[:, 1]], vertices[f[:, 2]]
    cross = torch.linalg.cross(b - a, c - a)
    total = torch.zeros_like(vertices)
    for j in range(3):
        total.index_add_(0, f[:, j], cross)
    length = total.norm(dim=1, keepdim=True)
    return torch.where(length > 0, total / length, torch.zeros_like(total))


def normals_against_float64(vertices, faces, candidates):
    """Per candidate (V, 3) float32: the largest |n - n_hat|_inf over the float32 bound of tests/mesh_clean_ref.py::normal_bound
    (sqrt(3) (d + 3) / 2 eps32 kappa + 4 eps32), over the vertices whose float64 sum is not zero; and how the mesh is conditioned."""
    eps = torch.finfo(torch.float32).eps
    f, v = faces.long(), vertices.double()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cross, weight = torch.linalg.cross(b - a, c - a), (b - a).norm(dim=1) * (c - a).norm(dim=1)
    total, scale = torch.zeros_like(v), torch.zeros(v.shape[0], dtype=v.dtype, device=v.device)
    valence = torch.zeros(v.shape[0], dtype=torch.int64, device=v.device)
    for j in range(3):
        total.index_add_(0, f[:, j], cross)
        scale.index_add_(0, f[:, j], weight)
        valence.index_add_(0, f[:, j], torch.ones_like(f[:, j]))
    length = total.norm(dim=1)
    live = length > 0
    n_hat = total[live] / length[live, None]
    kappa = scale[live] / length[live]
    bound = math.sqrt(3.0) * (valence[live] + 3) / 2 * eps * kappa + 4 * eps
    out = {"vertices_with_a_zero_float64_sum": int((~live).sum()), "kappa_median": float(kappa.median()), "kappa_max": float(kappa.max()),
           "vertices_with_kappa_above_1e3": int((kappa > 1e3).sum()), "valence_max": int(valence.max())}
    for name, n in candidates.items():
        err = (n.double()[live] - n_hat).abs().max(dim=1).values
        out[name] = {"max_error": float(err.max()), "max_error_over_bound": float((err / bound).max()),
                     "nonzero_rows_at_a_zero_sum": int((n[~live].abs().max(dim=1).values > 0).sum()) if int((~live).sum()) else 0}
    return out


def least_bytes(n_v, n_f, kept_v, kept_f):
    sort_passes = lambda bits: math.ceil(bits / 8)  # noqa: E731  (8-bit digits; keys and payload, read and written per pass)
    components = 8 * n_v + (12 * n_f + 12 * n_f) + 8 * n_v + (12 * n_f + 4 * n_f)  # init, hook, flatten, count
    select = (sort_passes(max(1, n_f.bit_length())) * 16 * n_v + (12 * n_f + 4 * n_f + 8 * n_v + 4 * n_v + 4 * n_f)  # sort, flags
              + 8 * n_v + 8 * n_f)                                                                                   # two scans
    compact = 2 * (12 * n_v + 8 * n_v / 3 + 12 * kept_v) + (12 * n_f + 8 * n_f + 12 * n_f + 12 * kept_f)  # vertices + colours; faces
    normals = (24 * n_f + sort_passes(max(1, n_v.bit_length())) * 16 * 3 * n_f + 12 * n_f + 4 * n_v      # keys, sort, run starts
               + 3 * n_f * (4 + 12 + 36) + 8 * n_v + 12 * n_v)                                            # per corner: id, face, 3 positions
    return {"components": components, "clean": components + select + compact, "normals": normals}


def bench_size(n, dev, rounds, warmup, maps, P, K):
    depth, alpha, image = maps
    voxel = 2 * mb.HALF / (n - 1)
    vol = mesh.TSDFVolume((-mb.HALF,) * 3, voxel, (n, n, n), 5 * voxel, dev, colour=True)
    vol.integrate(depth, alpha, P, K, image=image, alpha_min=0.5, depth_max=mb.DEPTH_MAX)
    vertices, faces, colours = vol.extract()
    n_v, n_f = vertices.shape[0], faces.shape[0]
    calls = {"extract": lambda: vol.extract(),
             "components": lambda: mesh.face_components(faces, n_v),
             "clean": lambda: mesh.clean_mesh(vertices, faces, colours),
             "normals": lambda: (mesh.vertex_normals(vertices, faces),),
             "torch_labels": lambda: torch_labels(faces, n_v),
             "torch_normals": lambda: (torch_normals(vertices, faces),)}
    times, first, last = mb.alternate(calls, rounds, warmup)
    label, size = last["components"]
    kept = last["clean"]
    counts = size[size > 0].sort(descending=True).values
    t_label, t_rounds = last["torch_labels"]
    normal_gap = (last["normals"][0] - last["torch_normals"][0]).abs().max()
    bytes_ = least_bytes(n_v, n_f, kept[0].shape[0], kept[1].shape[0])
    ms = {k: mb.stats(v) for k, v in times.items()}
    out = {"vertices": n_v, "faces": n_f, "components": int(counts.numel()), "largest_counts": counts[:5].tolist(),
           "kept_vertices": int(kept[0].shape[0]), "kept_faces": int(kept[1].shape[0]), "ms": ms,
           "least_bytes": {k: int(v) for k, v in bytes_.items()},
           "gb_per_s": {k: round(v / (ms[k]["median"] * 1e-3) / 1e9, 1) for k, v in bytes_.items()},
           "over_extract": {k: round(ms[k]["median"] / ms["extract"]["median"], 3) for k in ("components", "clean", "normals")},
           "torch_over_hip": {"labels": round(ms["torch_labels"]["median"] / ms["components"]["median"], 1),
                              "normals": round(ms["torch_normals"]["median"] / ms["normals"]["median"], 1)},
           "torch_label_rounds": t_rounds, "labels_equal_torch": bool(torch.equal(label.long(), t_label)),
           "normals_max_abs_difference_from_torch": float(normal_gap),
           "normals_against_float64": normals_against_float64(vertices, faces, {"hip": last["normals"][0], "torch": last["torch_normals"][0]}),
           "bit_equal_first_and_last_round": all(torch.equal(a, b) for k in ("components", "clean", "normals")
                                                 for a, b in zip(first[k], last[k]) if a is not None)}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="256,512")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_clean_bench measures on the GPU: no device visible")
    dev = torch.device("cuda", 0)
    P, K, _ = synthetic.ring_cameras(mb.CAMERAS, mb.WIDTH, mb.HEIGHT, radius=3.2, device=dev)
    maps = mb.sphere_maps(P, K, dev)
    out = {"rounds": a.rounds, "warmup": a.warmup, "cameras": mb.CAMERAS, "height": mb.HEIGHT, "width": mb.WIDTH,
           "sizes": {str(n): bench_size(int(n), dev, a.rounds, a.warmup, maps, P, K) for n in a.sizes.split(",")}}
    print(json.dumps(out), flush=True)
