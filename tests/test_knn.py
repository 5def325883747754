"""Exact k nearest neighbours (gcp_knn, csrc/gcp_knn.hip) without a GPU: the entry points are bound, exported and declared with
the ABI version unchanged, the workspace size is monotone and aligned, argument validation returns before any HIP call, the
Python layers refuse CPU tensors, the example takes its flag, the kernels compile without scratch, the oracle of
tests/knn_ref.py agrees with float64 brute force wherever float64 can tell, and the worlds really hold rows tied at the k
boundary, so the index rule cannot go untested."""
import ctypes
import inspect
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import knn_ref as kr

N = None  # a NULL pointer
NAMES = ("gcp_knn_workspace_bytes", "gcp_knn")
OK, INVALID, WORKSPACE = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from simplegaussiansplat_tk71_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def host():
    """Host memory standing in for device arrays: every call that gets it must return before anything would read it."""
    buf = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(buf) + 63) & ~63
    return buf, [base + 256 * k for k in range(8)]


def test_abi_version_is_unchanged_and_the_entry_points_are_bound_exported_and_declared(lib):
    from simplegaussiansplat_tk71_amd import _build, _lib, gs_model, knn

    assert lib.gcp_abi_version() == _lib.ABI_VERSION == 4
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert any(s.endswith("gcp_knn.hip") for s in _build.SRCS)  # the source hash covers it
    with open(_build.INCLUDE + "/grouped_cumprod_hip.h") as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
    # the definition is pinned there: the expression, the order, self by index, the padding, the precondition
    for phrase in ("(dx * dx + dy * dy) + dz * dz", "lexicographic", "by INDEX", "index = -1, dist2 = +inf", "FINITE coordinates"):
        assert phrase in header, phrase
    for name in ("nearest_neighbours", "neighbour_scale"):
        assert name in gs_model.__all__ and getattr(gs_model, name) is getattr(knn, name)
    assert inspect.signature(knn.neighbour_scale).parameters["rule"].default == "reference"
    assert inspect.signature(knn.neighbour_scale).parameters["neighbours"].default == 3


def test_workspace_size_is_monotone_and_aligned(lib):
    last = 0
    for n in (-5, 0, 1, 63, 64, 65, 4096, 4097, 10 ** 6 + 7, 2 ** 31 - 2):
        b = lib.gcp_knn_workspace_bytes(n)
        assert b % 256 == 0 and b > 0 and b >= last and b >= 28 * max(n, 0), n  # the sorted points, two key arrays, the permutation
        last = b
    assert lib.gcp_knn_workspace_bytes(10 ** 6) < 64 * 10 ** 6


def test_validation_returns_before_any_hip_call(lib, host):
    p = host[1]
    # xyz | index dist2 | ws
    def knn(n=4, k=3, ptrs=None, ws_bytes=1 << 20):
        a = list(p[:4]) if ptrs is None else ptrs
        return lib.gcp_knn(a[0], n, k, a[1], a[2], a[3], ws_bytes, None)

    assert knn(n=0) == OK and knn(n=0, ptrs=[N] * 4, ws_bytes=0) == OK  # no points: a no-op
    assert knn(n=-1) == INVALID and knn(n=-1, ptrs=[N] * 4) == INVALID and knn(n=2 ** 31 - 1) == INVALID
    for k in (-1, 0, 17, 2 ** 31 - 1):
        assert knn(k=k) == INVALID and knn(n=0, k=k) == INVALID, k
    for missing in range(4):
        a = list(p[:4])
        a[missing] = N
        assert knn(ptrs=a) == INVALID, missing
    need = lib.gcp_knn_workspace_bytes(4)
    assert knn(ws_bytes=need - 1) == WORKSPACE and knn(ws_bytes=0) == WORKSPACE
    assert knn(n=1000, ws_bytes=lib.gcp_knn_workspace_bytes(1000) - 256) == WORKSPACE


def test_python_layers_reject_cpu_tensors_and_bad_arguments():
    from simplegaussiansplat_tk71_amd import gs_model as gm

    pts = torch.rand(10, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gm.nearest_neighbours(pts, 3)
    for rule in ("reference", "3dgs"):
        with pytest.raises(RuntimeError, match="no CPU path"):
            gm.neighbour_scale(pts, rule)
    with pytest.raises(ValueError, match="rule"):
        gm.neighbour_scale(pts, "mean")
    for neighbours in (1, 18):
        with pytest.raises(ValueError, match="neighbours"):
            gm.neighbour_scale(pts, "reference", neighbours)
    assert gm.mean_neighbour_distance(3, pts).shape == (10, 3)  # the cdist route keeps its CPU path


def test_example_takes_the_flag():
    from examples import train_cameras as tc

    assert tc.build_parser().parse_args([]).init_scale == "cdist"
    for choice in ("cdist", "knn", "3dgs"):
        assert tc.build_parser().parse_args(["--init-scale", choice]).init_scale == choice
    with pytest.raises(SystemExit):
        tc.build_parser().parse_args(["--init-scale", "grid"])
    assert inspect.signature(tc.train).parameters["init_scale"].default == "cdist"
    z = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="init_scale"):
        tc.train(z, None, None, None, None, init_scale="grid")


def test_knn_kernels_use_no_scratch(tmp_path):
    """Zero scratch and zero spills in every kernel of the file: the best list of k_knn_search<16> is 32 registers that must
    never be indexed at run time."""
    from simplegaussiansplat_tk71_amd import _build

    src = [s for s in _build.SRCS if s.endswith("gcp_knn.hip")][0]
    out = tmp_path / "knn.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    res = subprocess.run([_build.find_hipcc(), *flags, "-I", _build.INCLUDE, "-S", "--cuda-device-only", "-o", str(out), src],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", out.read_text())
    report = {name: (int(scratch), int(vgpr), int(spills)) for name, scratch, vgpr, spills in kernels}
    print(report)
    assert len(report) == 10 and all("k_knn_" in k for k in report)  # six stages + the search at capacity 2, 4, 8, 16
    assert sum("k_knn_search" in k for k in report) == 4
    for name, (scratch, vgpr, spills) in report.items():
        assert scratch == 0 and spills == 0 and vgpr <= 128, (name, scratch, vgpr, spills)


def test_oracle_against_float64_brute_force_on_uniform():
    """Wherever the float64 gap between the k-th and the (k+1)-th neighbour exceeds what float32 rounding can move a squared
    distance by (each difference, square and sum rounds once: below 4 eps32 relative), the oracle lists the float64 set."""
    n, k = 1500, 5
    pts = kr.world("uniform", n)
    d32, i32 = kr.oracle("uniform", n, k)
    p = pts.astype(np.float64)
    diff = p[:, None, :] - p[None, :, :]
    d64 = (diff * diff).sum(axis=2)
    np.fill_diagonal(d64, np.inf)
    order = np.argsort(d64, axis=1, kind="stable")
    ranked = np.take_along_axis(d64, order, axis=1)
    clear = ranked[:, k] - ranked[:, k - 1] > 8 * kr.EPS32 * ranked[:, k]
    print("rows with a clear float64 gap:", int(clear.sum()), "of", n)
    assert clear.sum() > 0.99 * n
    assert (np.sort(i32[clear], axis=1) == np.sort(order[clear, :k], axis=1)).all()
    assert (i32 != np.arange(n)[:, None]).all() and (i32 >= 0).all()  # never self, never padding
    assert (np.diff(d32, axis=1) >= 0).all()
    rel = np.abs(d32.astype(np.float64) - np.take_along_axis(d64, i32.astype(np.int64), axis=1)) / np.take_along_axis(d64, i32.astype(np.int64), axis=1)
    print("oracle dist2 against float64: worst relative error", rel.max() / kr.EPS32, "eps32")
    assert rel.max() <= 4 * kr.EPS32


def test_oracle_orders_ties_by_index_and_pads():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0], [-1, 0, 0]], dtype=np.float32)
    d, i = kr.knn_bruteforce(pts, 3)
    assert i.tolist() == [[2, 1, 3], [0, 2, 3], [0, 1, 3], [0, 2, 1], [0, 2, 3]]
    assert d.tolist() == [[0, 1, 1], [1, 1, 2], [0, 1, 1], [1, 1, 2], [1, 1, 2]]
    d, i = kr.knn_bruteforce(pts[:2], 3)
    assert i.tolist() == [[1, -1, -1], [0, -1, -1]] and d[:, 0].tolist() == [1, 1] and np.isinf(d[:, 1:]).all()
    d, i = kr.knn_bruteforce(pts[:1], 2)
    assert i.tolist() == [[-1, -1]] and np.isinf(d).all()


@pytest.mark.parametrize("name,n,k", [("lattice", 4097, 3), ("lattice", 200, 8), ("fixture", None, 3)])
def test_worlds_hold_rows_tied_at_the_k_boundary(name, n, k):
    ties = kr.boundary_ties(name, n, k)
    d, _ = kr.oracle(name, n, k)
    print(name, n, "rows tied at the boundary of k =", k, ":", ties, "; rows with a neighbour at distance 0:", int((d[:, 0] == 0).sum()))
    assert ties > 0 and (d[:, 0] == 0).sum() > 0
