"""What csrc/gcp_tsdf.hip is tested against, in plain torch and numpy (no GPU, no library):
  * `integrate`: the TSDF update rule of include/grouped_cumprod_hip.h in float64, statement by statement, with the mask of the
    lattice points at which a float64 decision of any camera is marginal and the condition scale of the comparison;
  * `counts`: the exact number of vertices and triangles of the marching-tetrahedra surface from a sign array and a cell
    validity array alone;
  * `extract`: a slow per-tetrahedron extractor for grids of a few hundred cells, the winding decided geometrically;
  * `topology`: V - E + F and how often every edge is used, from a face list.
Volumes are (nz, ny, nx) arrays, x fastest; point (i, j, k) sits at origin + voxel (i, j, k)."""
import itertools
from collections import Counter

import numpy as np
import torch

KINDS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))  # (dx, dy, dz): +x +y +z +xy +xz +yz +xyz
PERMS = tuple(itertools.permutations(range(3)))  # axis 0 = x: the order of the tetrahedra in a cell


def lattice(dims, origin, voxel, dtype=torch.float64):
    """-> (nz, ny, nx, 3) world coordinates."""
    nx, ny, nz = dims
    k, j, i = torch.meshgrid(torch.arange(nz), torch.arange(ny), torch.arange(nx), indexing="ij")
    ijk = torch.stack([i, j, k], dim=-1).to(dtype)
    return torch.as_tensor(origin, dtype=dtype) + float(voxel) * ijk


# ---- integration ---------------------------------------------------------------------------------------------------------------
def integrate(state, dims, origin, voxel, trunc, depth, alpha, P, K, image=None, alpha_min=0.5, depth_max=0.0):
    """state = (tsdf, weight, rgb or None) float64 (nz, ny, nx) / (3, nz, ny, nx) -> (the new state, marginal bool (nz, ny, nx),
    scale float64 (nz, ny, nx) = max over the updating cameras of max(1, (|d| + |z|) / trunc)).  Inputs are taken to float64 as
    they are (the float32 world coordinates of the kernel are not imitated: origin + voxel i in float64)."""
    tsdf, weight, rgb = (None if t is None else t.double().clone() for t in state)
    xw = lattice(dims, torch.as_tensor(origin, dtype=torch.float32).double(), float(np.float32(voxel)))
    trunc = float(np.float32(trunc))
    marginal = torch.zeros(tsdf.shape, dtype=torch.bool)
    scale = torch.ones(tsdf.shape, dtype=torch.float64)
    b, _, h, w = depth.shape
    for c in range(b):
        Pc, Kc = P[c].double(), K[c].double()
        p = xw @ Pc[:, :3].T + Pc[:, 3]
        z = p[..., 2]
        marginal |= z.abs() < 1e-5
        live = z > 0
        zs = torch.where(live, z, torch.ones_like(z))
        u = Kc[0, 0] * p[..., 0] / zs + Kc[0, 2]
        v = Kc[1, 1] * p[..., 1] / zs + Kc[1, 2]
        near_int = ((u - u.round()).abs() < 1e-4) | ((v - v.round()).abs() < 1e-4)  # frame edges are integers too
        in_frame = (u >= 0) & (u < w) & (v >= 0) & (v < h)
        almost_in = (u > -1) & (u < w + 1) & (v > -1) & (v < h + 1)
        marginal |= live & near_int & almost_in
        live = live & in_frame
        x = u.floor().clamp(0, w - 1).long()
        y = v.floor().clamp(0, h - 1).long()
        a, D = alpha[c, 0].double()[y, x], depth[c, 0].double()[y, x]
        live = live & (a >= float(np.float32(alpha_min))) & (D > 0)  # a NaN compares false
        d = torch.where(live, D / torch.where(live, a, torch.ones_like(a)), torch.zeros_like(D))
        if depth_max > 0:
            marginal |= live & ((d - float(np.float32(depth_max))).abs() < 1e-5)
            live = live & ~(d > float(np.float32(depth_max)))
        s = d - z
        marginal |= live & ((s + trunc).abs() < 1e-5)
        live = live & ~(s < -trunc)
        tau = torch.clamp(s / trunc, max=1.0)
        w1 = weight + 1
        tsdf = torch.where(live, (tsdf * weight + tau) / w1, tsdf)
        if rgb is not None:
            col = image[c].double()[:, y, x]
            rgb = torch.where(live, (rgb * weight + col) / w1, rgb)
        weight = torch.where(live, w1, weight)
        scale = torch.where(live, torch.maximum(scale, (d.abs() + z.abs()) / trunc), scale)
    return (tsdf, weight, rgb), marginal, scale


# ---- exact counts --------------------------------------------------------------------------------------------------------------
def cell_validity(weight):
    """(nz, ny, nx) weights -> bool (nz-1, ny-1, nx-1): all 8 corners > 0."""
    ok = np.asarray(weight) > 0
    out = np.ones(tuple(n - 1 for n in ok.shape), dtype=bool)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        out &= ok[dz:ok.shape[0] - 1 + dz, dy:ok.shape[1] - 1 + dy, dx:ok.shape[2] - 1 + dx]
    return out


def edge_has_valid_cell(valid, kind):
    """bool over the owners (nz - dz, ny - dy, nx - dx) of the edges of `kind`: some valid cell contains the edge."""
    dx, dy, dz = kind
    nz, ny, nx = (n + 1 for n in valid.shape)
    padded = np.zeros((nz + 1, ny + 1, nx + 1), dtype=bool)  # cell (k, j, i) at [k + 1, j + 1, i + 1]; zeros around
    padded[1:nz, 1:ny, 1:nx] = valid
    out = np.zeros((nz, ny, nx), dtype=bool)
    for bz, by, bx in itertools.product(range(2 - dz), range(2 - dy), range(2 - dx)):
        out |= padded[1 - bz:1 - bz + nz, 1 - by:1 - by + ny, 1 - bx:1 - bx + nx]
    return out[:nz - dz, :ny - dy, :nx - dx]


def counts(inside, valid=None):
    """inside bool (nz, ny, nx), valid bool (nz-1, ny-1, nx-1) or None (all) -> (V, F): the sign-change owned edges next to a
    valid cell, and the triangles, per-tetrahedron cases summed over the valid cells."""
    inside = np.asarray(inside, dtype=bool)
    nz, ny, nx = inside.shape
    if valid is None:
        valid = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
    n_vert = 0
    for kind in KINDS:
        dx, dy, dz = kind
        change = inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]
        n_vert += int((change & edge_has_valid_cell(valid, kind)).sum())
    corner = lambda o: inside[o[2]:nz - 1 + o[2], o[1]:ny - 1 + o[1], o[0]:nx - 1 + o[0]].astype(np.int64)  # noqa: E731
    n_face = 0
    for perm in PERMS:
        o, m = [0, 0, 0], corner((0, 0, 0))
        for axis in perm:
            o[axis] = 1
            m = m + corner(o)
        n_face += int((np.where(m == 2, 2, np.where((m == 1) | (m == 3), 1, 0)) * valid).sum())
    return n_vert, n_face


# ---- the slow extractor --------------------------------------------------------------------------------------------------------
def extract(f, valid=None, origin=(0.0, 0.0, 0.0), voxel=1.0, iso=0.0):
    """f float (nz, ny, nx) -> (vertices float64 (V, 3), faces int64 (F, 3), keys: [(owner (i, j, k), kind index)] per vertex),
    cell by cell and tetrahedron by tetrahedron.  A triangle is turned so that its normal has a positive component along
    (mean of the outside corners) - (mean of the inside corners): inside a tetrahedron f is linear, its gradient g has
    g . (o - a) = f_o - f_a > 0 for every outside o and inside a, and the cut is a plane with normal parallel to g."""
    f = np.asarray(f, dtype=np.float64)
    nz, ny, nx = f.shape
    origin = np.asarray(origin, dtype=np.float64)
    ids, keys, verts, faces = {}, [], [], []

    def pos(c):
        return origin + voxel * np.asarray(c, dtype=np.float64)

    def vid(a, b):  # corners as (i, j, k); the lower one owns the edge
        lo, hi = (a, b) if a <= b else (b, a)  # comparable: chain members
        assert all(l <= h for l, h in zip(lo, hi))
        key = (lo, KINDS.index(tuple(h - l for l, h in zip(lo, hi))))
        if key not in ids:
            fl, fh = f[lo[2], lo[1], lo[0]], f[hi[2], hi[1], hi[0]]
            t = (iso - fl) / (fh - fl)
            ids[key] = len(verts)
            keys.append(key)
            verts.append(pos(lo) + t * (pos(hi) - pos(lo)))
        return ids[key]

    def emit(tri, towards):
        a, b, c = (verts[q] for q in tri)
        if np.dot(np.cross(b - a, c - a), towards) < 0:
            tri = [tri[0], tri[2], tri[1]]
        faces.append(tri)

    for k, j, i in itertools.product(range(nz - 1), range(ny - 1), range(nx - 1)):
        if valid is not None and not valid[k, j, i]:
            continue
        for perm in PERMS:
            chain = [(i, j, k)]
            for axis in perm:
                q = list(chain[-1])
                q[axis] += 1
                chain.append(tuple(q))
            ins = [c for c in chain if f[c[2], c[1], c[0]] < iso]
            outs = [c for c in chain if not f[c[2], c[1], c[0]] < iso]
            if not ins or not outs:
                continue
            towards = np.mean([pos(c) for c in outs], axis=0) - np.mean([pos(c) for c in ins], axis=0)
            if len(ins) == 1:
                emit([vid(ins[0], o) for o in outs], towards)
            elif len(ins) == 3:
                emit([vid(outs[0], c) for c in ins], towards)
            else:
                (a, b), (o0, o1) = ins, outs
                q = [vid(a, o0), vid(a, o1), vid(b, o1), vid(b, o0)]
                emit([q[0], q[1], q[2]], towards)
                emit([q[0], q[2], q[3]], towards)
    return np.asarray(verts, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3), keys


# ---- topology ------------------------------------------------------------------------------------------------------------------
def topology(n_vert, faces):
    """-> (V - E + F, Counter of undirected edge uses -> number of edges, the largest count of one DIRECTED edge)."""
    faces = np.asarray(faces).reshape(-1, 3)
    directed = Counter()
    for a, b in ((0, 1), (1, 2), (2, 0)):
        directed.update(zip(faces[:, a].tolist(), faces[:, b].tolist()))
    undirected = Counter()
    for (a, b), n in directed.items():
        undirected[(min(a, b), max(a, b))] += n
    return n_vert - len(undirected) + faces.shape[0], Counter(undirected.values()), max(directed.values(), default=0)


def canonical_faces(faces):
    """The faces as a sorted list of triples rotated so that the smallest index comes first (the winding is kept)."""
    out = []
    for tri in np.asarray(faces).reshape(-1, 3).tolist():
        r = tri.index(min(tri))
        out.append(tuple(tri[r:] + tri[:r]))
    return sorted(out)


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = (v[np.asarray(faces)[:, n]] for n in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# ---- analytic fields (float32 (nz, ny, nx) arrays; no lattice value is exactly 0) ----------------------------------------------
def grid_xyz(dims):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return i.astype(np.float64), j.astype(np.float64), k.astype(np.float64)


def sphere_field(dims, centre, radius):
    x, y, z = grid_xyz(dims)
    return (np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius).astype(np.float32)


def torus_field(dims, centre, major, minor):
    x, y, z = grid_xyz(dims)
    x, y, z = x - centre[0], y - centre[1], z - centre[2]
    return (np.sqrt((np.sqrt(x * x + y * y) - major) ** 2 + z * z) - minor).astype(np.float32)


def plane_field(dims, normal, offset):
    x, y, z = grid_xyz(dims)
    return (normal[0] * x + normal[1] * y + normal[2] * z - offset).astype(np.float32)


SPHERE = dict(dims=(19, 14, 11), centre=(9.13, 6.57, 5.21), radius=4.3)
TORUS = dict(dims=(23, 23, 9), centre=(11.13, 10.57, 4.21), major=7.2, minor=2.6)
PLANE = dict(dims=(19, 14, 11), normal=(0.3, 0.5, 1.0), offset=9.21)
