"""Mesh extraction (csrc/gcp_tsdf.hip, simplegaussiansplat_tk71_amd/mesh.py) without a GPU: the four entry points bound, exported
and declared and refusing before any HIP call, mesh files round-tripping through ply_io, the options defaulting to off, the
reference of tests/mesh_ref.py against the closed surfaces it is used on — and the input conditions of tests/test_tsdf_gpu.py,
built here exactly as that file builds them: at most 1 % of the lattice points of any case are left out of its comparison."""
import ctypes
import inspect
import re

import numpy as np
import pytest
import torch

from tests import mesh_cases as mc
from tests import mesh_ref as mr

NAMES = ("gcp_tsdf_integrate", "gcp_mesh_workspace_bytes", "gcp_mesh_count", "gcp_mesh_write")
OK, INVALID, WORKSPACE = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from simplegaussiansplat_tk71_amd import _lib

    return _lib.load()


def test_the_source_and_its_entry_points_are_built_bound_and_declared(lib):
    from simplegaussiansplat_tk71_amd import _build, _lib

    assert any(s.endswith("gcp_tsdf.hip") for s in _build.SRCS)
    with open(_build.INCLUDE + "/grouped_cumprod_hip.h") as f:
        header = f.read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.gcp_abi_version() == _lib.ABI_VERSION == 4


def _buffers(n=16):
    buf = ctypes.create_string_buffer(256 * (n + 2))
    base = (ctypes.addressof(buf) + 255) & ~255
    return buf, [base + 256 * k for k in range(n)]


def test_integrate_validates_before_any_hip_call(lib):
    """Host memory stands in for device arrays: every call that gets it must return before anything would read it."""
    keep, p = _buffers()

    def call(dims=(4, 3, 2), voxel=0.1, trunc=0.5, b=2, h=5, w=7, a=p, origin=(0.0, 0.0, 0.0)):
        return lib.gcp_tsdf_integrate(a[0], a[1], a[2], *dims, *origin, voxel, trunc, a[3], a[4], a[5], a[6], a[7], b, h, w, 0.5, 0.0, None)

    assert call(b=0) == OK  # a no-op, whatever the pointers
    assert call(b=0, a=[None] * 8) == OK
    assert call(b=-1) == INVALID
    for dims in ((1, 3, 2), (4, 1, 2), (4, 3, 1), (0, 3, 2), (-4, 3, 2), (2048, 1024, 1024), (65536, 32768, 2)):
        assert call(dims=dims) == INVALID and call(dims=dims, b=0) == INVALID, dims
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(voxel=bad) == INVALID and call(trunc=bad) == INVALID and call(voxel=bad, b=0) == INVALID
    assert call(origin=(float("nan"), 0.0, 0.0)) == INVALID
    assert call(h=0) == INVALID and call(w=0) == INVALID and call(h=2 ** 16, w=2 ** 16) == INVALID
    for missing in (0, 1, 3, 4, 6, 7):  # rgb (2) is optional; image (5) only with rgb
        a = list(p)
        a[missing] = None
        assert call(a=a) == INVALID, missing
    a = list(p)
    a[5] = None
    assert call(a=a) == INVALID  # rgb without image
    del keep


def test_extraction_validates_before_any_hip_call(lib):
    keep, p = _buffers()
    totals = (ctypes.c_int64 * 2)(7, 7)
    assert lib.gcp_mesh_workspace_bytes(4, 3, 2) >= 4 * 3 * 2 * 18 and lib.gcp_mesh_workspace_bytes(4, 3, 2) % 256 == 0
    assert lib.gcp_mesh_workspace_bytes(1, 3, 2) == 0 and lib.gcp_mesh_workspace_bytes(2048, 1024, 1024) == 0
    big = 1 << 40

    def count(dims=(4, 3, 2), iso=0.0, f=p[0], w=p[1], ws=p[2], ws_bytes=big, out=totals):
        return lib.gcp_mesh_count(f, w, *dims, iso, ws, ws_bytes, out, None)

    def write(dims=(4, 3, 2), voxel=1.0, iso=0.0, f=p[0], rgb=p[1], ws=p[2], ws_bytes=big, nv=3, nf=1, v=p[3], fa=p[4], col=p[5]):
        return lib.gcp_mesh_write(f, rgb, *dims, 0.0, 0.0, 0.0, voxel, iso, ws, ws_bytes, nv, nf, v, fa, col, None)

    for dims in ((1, 3, 2), (4, 1, 2), (4, 3, 1), (2048, 1024, 1024)):
        assert count(dims=dims) == INVALID and write(dims=dims) == INVALID, dims
    assert count(iso=float("nan")) == INVALID and write(iso=float("nan")) == INVALID
    assert count(f=None) == INVALID and count(ws=None) == INVALID and count(out=None) == INVALID
    assert count(ws_bytes=16) == WORKSPACE and write(ws_bytes=16) == WORKSPACE
    assert count(ws=p[2] + 8) == WORKSPACE and write(ws=p[2] + 8) == WORKSPACE
    assert write(voxel=0.0) == INVALID and write(voxel=float("nan")) == INVALID
    assert write(f=None) == INVALID and write(ws=None) == INVALID
    assert write(nv=-1) == INVALID and write(nf=-1) == INVALID and write(nv=2 ** 31) == INVALID and write(nf=2 ** 31) == INVALID
    assert write(v=None) == INVALID and write(fa=None) == INVALID and write(rgb=None) == INVALID  # colours without rgb
    assert write(nv=0, nf=0, v=None, fa=None, col=None) == OK  # nothing to write: nothing is launched
    del keep


def test_python_refuses_before_the_library():
    from simplegaussiansplat_tk71_amd import gs_model as gm
    from simplegaussiansplat_tk71_amd import mesh

    for name in ("TSDFVolume", "extract_surface"):
        assert name in gm.__all__ and getattr(gm, name) is getattr(mesh, name)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), 0.5, "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.extract_surface(torch.zeros(4, 4, 4))
    for dims in ((1, 4, 4), (2048, 1024, 1024)):
        with pytest.raises(RuntimeError, match="dims"):
            mesh.TSDFVolume((0, 0, 0), 0.1, dims, 0.5, "cuda")
    for voxel, trunc in ((0.0, 0.5), (0.1, 0.0), (-1.0, 0.5)):
        with pytest.raises(RuntimeError, match="positive"):
            mesh.TSDFVolume((0, 0, 0), voxel, (4, 4, 4), trunc, "cuda")
    assert "not capturable" in mesh.extract_surface.__doc__.lower()


def test_options_default_to_off():
    import cuda_kernel as ck
    from examples import train_cameras as tc
    from simplegaussiansplat_tk71_amd import gs_model as gm

    a = tc.build_parser().parse_args([])
    assert a.save_mesh is None and a.mesh_resolution == 256 and a.mesh_trunc is None
    a = tc.build_parser().parse_args(["--save-mesh", "m.ply", "--mesh-resolution", "64", "--mesh-trunc", "0.1"])
    assert a.save_mesh == "m.ply" and a.mesh_resolution == 64 and a.mesh_trunc == 0.1
    sig = inspect.signature(tc.train).parameters
    assert sig["save_mesh"].default is None and sig["mesh_resolution"].default == 256 and sig["mesh_trunc"].default is None
    sig = inspect.signature(gm.GS_model_with_param.extract_mesh).parameters
    assert [sig[k].default for k in ("resolution", "bounds", "trunc", "alpha_min", "depth_max", "batch_size", "colour")] == [
        256, None, None, 0.5, None, 4, True]
    assert "not tuned" in gm.GS_model_with_param.extract_mesh.__doc__
    assert "paint_maps" in ck.__all__


# ---- mesh files ----------------------------------------------------------------------------------------------------------------
def _mesh(n_face=2):
    v = torch.tensor([[0.0, 0.5, 1.0], [1.25, 0.0, -2.0], [3.0, 1.0, 0.125], [0.0, 0.0, 7.0]])
    f = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)[:n_face]
    c = torch.tensor([[0.0, 1.0, 0.2], [51 / 255, 102 / 255, 1.0], [1.5, -0.5, 0.5], [0.25, 0.75, 1 / 3]])
    return v, f, c


@pytest.mark.parametrize("coloured", [False, True])
@pytest.mark.parametrize("n_face", [2, 0])
def test_mesh_files_round_trip(tmp_path, coloured, n_face):
    from simplegaussiansplat_tk71_amd import ply_io

    v, f, c = _mesh(n_face)
    path = tmp_path / "m.ply"
    ply_io.save_mesh(path, v, f, c if coloured else None)
    v2, f2, c2 = ply_io.load_mesh(path)
    assert torch.equal(v2, v) and v2.dtype == torch.float32
    assert torch.equal(f2, f) and f2.dtype == torch.int32 and f2.shape == (n_face, 3)
    if coloured:
        assert torch.equal(c2, torch.round(c.clamp(0, 1) * 255) / 255)
    else:
        assert c2 is None
    data = path.read_bytes()
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
              + ("property uchar red\nproperty uchar green\nproperty uchar blue\n" if coloured else "")
              + f"element face {n_face}\nproperty list uchar int vertex_indices\nend_header\n").encode()
    assert data.startswith(header)
    assert len(data) == len(header) + 4 * (12 + (3 if coloured else 0)) + n_face * 13
    body = data[len(header):]
    assert np.frombuffer(body[:12], dtype="<f4").tolist() == [0.0, 0.5, 1.0]
    if coloured:
        assert list(body[12:15]) == [0, 255, 51]
    if n_face:
        at = 4 * (12 + (3 if coloured else 0))
        assert body[at] == 3 and np.frombuffer(body[at + 1:at + 13], dtype="<i4").tolist() == [0, 1, 2]


def test_mesh_files_refuse_what_they_do_not_hold(tmp_path):
    from simplegaussiansplat_tk71_amd import ply_io

    v, f, c = _mesh()
    with pytest.raises(ValueError, match="index"):
        ply_io.save_mesh(tmp_path / "m.ply", v, f + 3)
    with pytest.raises(ValueError, match="expected"):
        ply_io.save_mesh(tmp_path / "m.ply", v[:, :2], f)
    ply_io.save_mesh(tmp_path / "empty.ply", torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32))
    v0, f0, c0 = ply_io.load_mesh(tmp_path / "empty.ply")
    assert v0.shape == (0, 3) and f0.shape == (0, 3) and c0 is None
    (tmp_path / "bad.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nelement face 0\nend_header\n")
    with pytest.raises(ValueError, match="layout"):
        ply_io.load_mesh(tmp_path / "bad.ply")


# ---- the reference itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,field,chi,n_vert,boundary", [
    ("sphere", lambda: mr.sphere_field(**mr.SPHERE), 2, 1036, 0),
    ("torus", lambda: mr.torus_field(**mr.TORUS), 0, 3230, 0),
    ("plane", lambda: mr.plane_field(**mr.PLANE), 1, 1599, 162)])
def test_the_reference_extractor_and_the_counters_agree(name, field, chi, n_vert, boundary):
    f = field()
    assert not (f == 0).any()
    v, faces, keys = mr.extract(f)
    assert mr.counts(f < 0) == (len(v), len(faces)) and len(v) == n_vert
    got_chi, uses, directed = mr.topology(len(v), faces)
    assert got_chi == chi and directed == 1 and uses.get(1, 0) == boundary and set(uses) <= {1, 2}
    assert len(set(keys)) == len(keys) and set(faces.reshape(-1).tolist()) == set(range(len(v)))
    if boundary == 0:
        assert mr.signed_volume(v, faces) > 0


def test_the_counters_follow_cell_validity():
    f = mr.sphere_field(**mr.SPHERE)
    weight = mc.slab_weight(f.shape)
    valid = mr.cell_validity(weight)
    assert valid.any() and not valid.all()
    v, faces, _ = mr.extract(f, valid)
    assert mr.counts(f < 0, valid) == (len(v), len(faces)) and 0 < len(v) < 1036


# ---- the input conditions of tests/test_tsdf_gpu.py ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", mc.TSDF_CASES, ids=lambda c: c["id"])
def test_tsdf_cases_leave_out_at_most_one_percent(case):
    inputs = mc.tsdf_inputs(case)
    state, marginal, scale = mc.tsdf_reference(case, inputs)
    left_out = marginal.double().mean().item()
    assert left_out <= 0.01, left_out
    weight = state[1]
    assert weight.max() >= 2 and (weight == 0).any()  # the case exercises both updated and untouched points
    if case.get("expect_behind"):
        assert inputs["behind"] > 0 and inputs["grazing"] > 0
