"""Exact k nearest neighbours (csrc/gcp_knn.hip, simplegaussiansplat_tk71_amd/knn.py): the oracle and the worlds its tests run
on.  A helper, not a test.

The oracle is numpy float32 brute force with the expression the header pins, d2 = (dx dx + dy dy) + dz dz — numpy rounds
every float32 operation once and fuses nothing, as the library compiled with -ffp-contract=off does, so the kernel is held to
it BIT FOR BIT — and a stable order by (d2, index).  Per row only the candidates at or below the k-th value (np.partition) are
sorted, which keeps the 10 409-point fixture cloud to seconds.  Results are cached per (world, n, k) and must not be modified.

The float64 statements of the two scale rules (`scale_f64`) and their float32 restatement on the host (`scale_f32`) serve the
tolerance of `neighbour_scale`: the margin of tests/filter3d_torch.py over what the float32 restatement misses float64 by."""
import functools
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "colmap_scene", "sparse", "0", "points3D.bin")
WORLDS = ("uniform", "lattice", "clusters", "identical", "line", "plane", "offset", "fixture")
DEGENERATE = ("identical", "line", "plane")
EPS32 = float(np.finfo(np.float32).eps)


def fixture_cloud():
    from simplegaussiansplat_tk71_amd import colmap_io

    return np.ascontiguousarray(colmap_io.read_points3d(FIXTURE)["xyz"].astype(np.float32))


@functools.lru_cache(maxsize=None)
def world(name, n):
    """float32 (n, 3), read-only; seeded by the name and the size alone.  `fixture` ignores n (pass None)."""
    if name == "fixture":
        pts = fixture_cloud()
    else:
        rng = np.random.default_rng([WORLDS.index(name), 0 if n is None else n])
        if name == "uniform":  # the baseline
            pts = rng.random((n, 3))
        elif name == "lattice":  # small integers with repeats: every distance exact, many ties and duplicates
            pts = rng.integers(0, 7, (n, 3)).astype(np.float64)
        elif name == "clusters":  # two clusters 1e-3 wide, 1e3 apart, a handful of outliers at 1e6: a cluster shares one Morton key
            pts = 1e-3 * rng.random((n, 3))
            pts[n // 2:, 0] += 1e3
            far = min(5, n // 4)
            pts[:far] = 1e6 * rng.choice([-1.0, 1.0], (far, 3)) * (1.0 + rng.random((far, 3)))
            pts = pts[rng.permutation(n)]
        elif name == "identical":  # one point repeated: zero extent on every axis
            pts = np.tile(np.array([[1.5, -2.25, 3.0]]), (n, 1))
        elif name == "line":  # zero extent on two axes
            pts = np.stack([rng.random(n), np.full(n, 0.75), np.full(n, -4.0)], axis=1)
        elif name == "plane":  # zero extent on one axis
            pts = np.stack([rng.random(n), rng.random(n), np.full(n, 2.5)], axis=1)
        elif name == "offset":  # `uniform` at a spacing of 1e-2, shifted by 1e4: a few ulps between neighbours
            pts = 1e4 + 1e-2 * max(n, 1) ** (1.0 / 3.0) * rng.random((n, 3))
        else:
            raise KeyError(name)
        pts = np.ascontiguousarray(pts.astype(np.float32))
    pts.setflags(write=False)
    return pts


def d2_rows(pts, rows):
    """float32 (len(rows), n): the pinned expression for the given query rows against the whole cloud."""
    q = pts[rows]
    dx = q[:, None, 0] - pts[None, :, 0]
    dy = q[:, None, 1] - pts[None, :, 1]
    dz = q[:, None, 2] - pts[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def knn_bruteforce(pts, k, rows=None):
    """(dist2 float32 (m, k), index int32 (m, k)) for the query rows (default: all): ascending by (d2, index), self excluded by
    index, padded with +inf / -1."""
    pts = np.asarray(pts, dtype=np.float32)
    n = pts.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    dist2 = np.full((rows.size, k), np.inf, dtype=np.float32)
    index = np.full((rows.size, k), -1, dtype=np.int32)
    kk = min(k, n - 1)
    if kk <= 0 or rows.size == 0:
        return dist2, index
    batch = max(1, (1 << 22) // n)
    for b0 in range(0, rows.size, batch):
        r = rows[b0:b0 + batch]
        d2 = d2_rows(pts, r)
        kth = np.partition(d2, kk, axis=1)[:, kk]  # self is a 0, the least value there is: position kk of the whole row = the kk-th other
        for t, i in enumerate(r):
            row = d2[t]
            cand = np.nonzero(row <= kth[t])[0]  # ascending index
            cand = cand[cand != i]
            order = np.argsort(row[cand], kind="stable")[:kk]  # stable: equal distances stay in index order
            dist2[b0 + t, :kk] = row[cand[order]]
            index[b0 + t, :kk] = cand[order]
    return dist2, index


@functools.lru_cache(maxsize=None)
def oracle(name, n, k):
    """The oracle's (dist2, index) of world(name, n), read-only and shared between the tests."""
    d, i = knn_bruteforce(world(name, n), k)
    d.setflags(write=False)
    i.setflags(write=False)
    return d, i


def boundary_ties(name, n, k):
    """Rows whose k-th and (k+1)-th neighbours are at the same distance: where only the index rule decides who is listed."""
    d, _ = oracle(name, n, k + 1)
    return int((np.isfinite(d[:, k]) & (d[:, k - 1] == d[:, k])).sum())


def neighbour_d2_f64(pts, index):
    """float64 squared distances (n, k) from every point to the listed neighbours (index >= 0 everywhere)."""
    p = np.asarray(pts, dtype=np.float64)
    diff = p[:, None, :] - p[index]
    return (diff * diff).sum(axis=2)


def scale_f64(pts, index, rule, neighbours=3):
    """The scale rule stated in float64 on the given neighbours (columns already cut to those the rule uses)."""
    d2 = neighbour_d2_f64(pts, index)
    if rule == "reference":
        return np.sqrt(d2).sum(axis=1) / neighbours
    return np.sqrt(np.maximum(d2.mean(axis=1), 1e-7))


def scale_f32(dist2, rule, neighbours=3):
    """The same statements in float32 on the host, from the oracle's float32 dist2 (columns already cut), summed left to right."""
    d2 = np.asarray(dist2, dtype=np.float32)
    terms = np.sqrt(d2) if rule == "reference" else d2
    total = terms[:, 0].copy()
    for j in range(1, terms.shape[1]):
        total = total + terms[:, j]
    if rule == "reference":
        return total / np.float32(neighbours)
    return np.sqrt(np.maximum(total / np.float32(terms.shape[1]), np.float32(1e-7)))
