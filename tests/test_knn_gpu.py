"""Exact k nearest neighbours on the GPU (csrc/gcp_knn.hip): every word of `index` and `dist2` against the float32 brute-force
oracle of tests/knn_ref.py — EXACTLY, so there is no tolerance — at the sizes where leaves, groups and blocks begin and end, on
worlds with ties, duplicates, degenerate extents and a cloud far from its origin; the same bits under a permutation of the
points, on another stream and over a differently painted workspace; no write outside outputs and workspace; the two scale
rules against their float64 statements; the training example on top.  The outputs start at NaN / a sentinel: an unwritten
word fails.  tests/test_knn.py holds what needs no GPU, the worlds' tie counts among it."""
import json
import os

import numpy as np
import pytest
import torch

from tests import filter3d_torch as ft
from tests import knn_ref as kr
from tests.guarded_alloc import Arena, guarded, same_bits

pytestmark = pytest.mark.gpu

K = 3
# where the structure can break: nothing, one point, fewer points than k, one leaf and its edges, one group (64 leaves = 4096
# points) and its edges, a third group with a 3-point last leaf.  The kernels have no grid cap: every launch covers its items.
SIZES = (0, 1, 2, K, K + 1, 63, 64, 65, 4095, 4096, 4097, 8195)
SENTINEL = -77


def raw_knn(points, k, paint=0xA5, stream=None):
    """gcp_knn through ctypes on buffers of the test's own: outputs preset to NaN / SENTINEL, the workspace painted."""
    from simplegaussiansplat_tk71_amd import _lib

    lib = _lib.load()
    dev = points.device
    n = points.shape[0]
    dist2 = torch.full((n, k), float("nan"), dtype=torch.float32, device=dev)
    index = torch.full((n, k), SENTINEL, dtype=torch.int32, device=dev)
    ws = torch.full((lib.gcp_knn_workspace_bytes(n),), paint, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(s):
        _lib.check(lib.gcp_knn(points.data_ptr(), n, k, index.data_ptr(), dist2.data_ptr(), ws.data_ptr(), ws.numel(), s.cuda_stream), "gcp_knn")
    s.synchronize()
    return dist2, index


def assert_exact(got, want, what):
    (d, i), (wd, wi) = got, want
    d, i = d.cpu().numpy(), i.cpu().numpy()
    assert d.shape == wd.shape and i.shape == wi.shape, what
    bad = np.nonzero((i != wi).any(axis=1) | (d.view(np.uint32) != wd.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, (what, "rows that differ:", bad.size, "first", int(bad[0]), i[bad[0]].tolist(), wi[bad[0]].tolist(),
                           d[bad[0]].tolist(), wd[bad[0]].tolist())


CASES = ([("uniform", n, K) for n in SIZES] + [("lattice", n, K) for n in SIZES]
         + [(name, n, K) for name in kr.DEGENERATE for n in (200, 4097)]
         + [("clusters", 8195, K), ("offset", 8195, K), ("fixture", None, K)])


@pytest.mark.parametrize("name,n,k", CASES, ids=[f"{name}-{n}" for name, n, _ in CASES])
def test_exact_parity_with_the_oracle(device, name, n, k):
    pts = torch.tensor(kr.world(name, n)).to(device)
    assert_exact(raw_knn(pts, k), kr.oracle(name, n, k), (name, n, k))


@pytest.mark.parametrize("k", range(1, 17))
def test_every_k(device, k):
    pts = torch.tensor(kr.world("lattice", 200)).to(device)
    assert_exact(raw_knn(pts, k), kr.oracle("lattice", 200, k), k)


@pytest.mark.parametrize("n,k", [(1, 1), (1, 16), (2, 2), (2, 5), (5, 5), (5, 8), (9, 16), (16, 16), (17, 16)])
def test_rows_with_fewer_than_k_others_are_padded(device, n, k):
    pts = torch.tensor(kr.world("lattice", n)).to(device)
    d, i = raw_knn(pts, k)
    assert_exact((d, i), kr.oracle("lattice", n, k), (n, k))
    have = min(k, n - 1)
    assert bool((i[:, have:] == -1).all()) and bool(torch.isposinf(d[:, have:]).all()) and bool((i[:, :have] >= 0).all())


@pytest.mark.parametrize("name", ("uniform", "lattice"))
def test_a_permutation_of_the_points_permutes_the_rows(device, name):
    """dist2 of points[perm], un-permuted, has the bits of dist2 of points: nothing depends on where a point sits in memory (the
    indices may differ only among equal distances, where the rule is by the caller's numbering)."""
    n = 4097
    host = torch.tensor(kr.world(name, n))
    d0, _ = raw_knn(host.to(device), 4)
    for perm in (torch.arange(n - 1, -1, -1), torch.randperm(n, generator=torch.Generator().manual_seed(5))):
        d1, i1 = raw_knn(host[perm].contiguous().to(device), 4)
        back = torch.empty_like(d1)
        back[perm.to(device)] = d1
        assert same_bits(back, d0), name
        assert bool((i1 >= 0).all()) and bool((i1 < n).all())


def test_runs_streams_and_workspace_contents_do_not_change_a_bit(device):
    pts = torch.tensor(kr.world("fixture", None)).to(device)
    d0, i0 = raw_knn(pts, 5)
    side = torch.cuda.Stream(device)
    torch.cuda.synchronize(device)
    for d1, i1 in (raw_knn(pts, 5), raw_knn(pts, 5, paint=0x00), raw_knn(pts, 5, paint=0xFF), raw_knn(pts, 5, stream=side)):
        assert same_bits(d1, d0) and same_bits(i1, i0)


@pytest.mark.parametrize("offset_bytes", (0, 4))
@pytest.mark.parametrize("name,n,k", [("lattice", 4097, 3), ("clusters", 8195, 3), ("uniform", 65, 16), ("lattice", 2, 5)])
def test_guarded_no_write_outside_outputs_and_workspace(device, monkeypatch, name, n, k, offset_bytes):
    from simplegaussiansplat_tk71_amd import knn

    arena = Arena(offset_bytes=offset_bytes)
    guarded(monkeypatch, arena, knn)
    pts = arena.copy(torch.tensor(kr.world(name, n)).to(device))
    d, i = knn.nearest_neighbours(pts, k)
    torch.cuda.synchronize(device)
    assert arena.check() == []
    assert len(arena.blocks) == 4 and arena.unwritten(d) == 0 and arena.unwritten(i) == 0  # points, dist2, index, workspace
    assert_exact((d, i), kr.oracle(name, n, k), (name, n, k, offset_bytes))


@pytest.mark.parametrize("name,n", [("fixture", None), ("offset", 8195)])
def test_neighbour_scale_against_float64(device, name, n):
    """Both rules against their float64 statement on the oracle's neighbours; a row may miss it by filter3d_torch.MARGIN times
    what the float32 restatement of the same formula misses it by, relative to the value (a sum of non-negative terms is its own
    condition scale).  On `offset` the cdist route is printed beside it: that one is not held to anything."""
    from simplegaussiansplat_tk71_amd import gs_model as gm

    host = kr.world(name, n)
    pts = torch.tensor(host).to(device)
    d32, i32 = kr.oracle(name, n, K)
    for rule, cols, neighbours in (("reference", 2, 3), ("3dgs", 3, 3), ("reference", 3, 4)):
        want = torch.from_numpy(kr.scale_f64(host, i32[:, :cols].astype(np.int64), rule, neighbours))
        yard = torch.from_numpy(kr.scale_f32(d32[:, :cols], rule, neighbours))
        got = gm.neighbour_scale(pts, rule, neighbours).cpu()
        assert got.shape == (host.shape[0], 3) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        assert torch.equal(got[:, 0], got[:, 1]) and torch.equal(got[:, 0], got[:, 2])
        scale = want.abs()
        err, allowed = ft.worst(got[:, 0], want, scale), ft.MARGIN * ft.worst(yard, want, scale)
        print(f"{name} {rule} neighbours={neighbours}: kernel route {err / ft.EPS32:.3f} eps32, float32 restatement "
              f"{allowed / ft.MARGIN / ft.EPS32:.3f} eps32, allowed {allowed / ft.EPS32:.3f}")
        if rule == "reference" and name == "offset":
            cd = gm.mean_neighbour_distance(neighbours, pts).cpu()[:, 0].double()
            rel = ((cd - want).abs() / want)[want > 0]
            print(f"{name} mean_neighbour_distance({neighbours}) against float64: max relative error {float(rel.max()):.3g}, "
                  f"median {float(rel.median()):.3g}; the kernel route: max {err:.3g}")
        assert err <= allowed, (name, rule, err, allowed)


def test_neighbour_scale_refuses_what_it_cannot_answer(device):
    from simplegaussiansplat_tk71_amd import gs_model as gm

    pts = torch.tensor(kr.world("uniform", 65)).to(device)
    for bad in (float("nan"), float("inf"), -float("inf")):
        broken = pts.clone()
        broken[17, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            gm.nearest_neighbours(broken, 3)
        with pytest.raises(ValueError, match="non-finite"):
            gm.neighbour_scale(broken, "3dgs")
    for rule in ("reference", "3dgs"):
        with pytest.raises(ValueError, match="one point"):
            gm.neighbour_scale(pts[:1], rule)
    with pytest.raises(ValueError, match="k: 1..16"):
        gm.nearest_neighbours(pts, 17)
    with pytest.raises(RuntimeError, match="float32"):
        gm.nearest_neighbours(pts.double(), 3)
    # fewer others than the rule asks for: the neighbours there are.  Two points at distance 5: (0 + 5) / 2 and sqrt(25)
    two = torch.tensor([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]], device=device)
    assert gm.neighbour_scale(two, "reference", 3).cpu().tolist() == [[2.5] * 3] * 2
    assert gm.neighbour_scale(two, "3dgs").cpu().tolist() == [[5.0] * 3] * 2
    d, i = gm.nearest_neighbours(pts[:0], 3)
    assert d.shape == (0, 3) and i.shape == (0, 3) and gm.neighbour_scale(pts[:0]).shape == (0, 3)


def test_example_trains_from_either_kernel_rule_and_cdist_keeps_its_golden_losses(device):
    from examples.train_cameras import synthetic_scene, train

    start, P, K_, wh, targets = synthetic_scene(600, 6, 64, 48, 0, device)
    for init in ("knn", "3dgs"):
        _, losses = train(start, P, K_, wh, targets, iterations=4, densify_from_iter=10, log=lambda *_: None, init_scale=init)
        assert len(losses) == 4 and all(np.isfinite(v) for v in losses), (init, losses)
    with open(os.path.join(os.path.dirname(__file__), "golden", "default_loop_losses.json")) as f:
        want = json.load(f)
    model, losses = train(start, P, K_, wh, targets, iterations=30, densify_from_iter=10, densification_interval=10,
                          opacity_reset_interval=20, log=lambda *_: None, init_scale="cdist")
    assert losses == want["losses"] and model.mean.shape[0] == want["gaussians"]
