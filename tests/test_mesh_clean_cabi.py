"""Mesh cleaning and vertex normals (csrc/gcp_meshclean.hip, simplegaussiansplat_tk71_amd/mesh.py) without a GPU: the seven entry
points bound, exported and declared and refusing before any HIP call, the workspace functions, the Python wrappers refusing CPU
tensors, the options defaulting to off, mesh files with normals — and the fixtures of tests/test_mesh_clean_gpu.py, checked here
against the slow extractor and scipy exactly as that file asserts them."""
import ctypes
import inspect
import re

import numpy as np
import pytest
import torch

from tests import mesh_clean_ref as cr
from tests import mesh_ref as mr

NAMES = ("gcp_mesh_components_workspace_bytes", "gcp_mesh_components", "gcp_mesh_clean_workspace_bytes", "gcp_mesh_select",
         "gcp_mesh_compact", "gcp_mesh_vertex_normals_workspace_bytes", "gcp_mesh_vertex_normals")
OK, INVALID, WORKSPACE = 0, 1, 2
TOO_MANY = (2 ** 31 - 1) // 3 + 1  # 3 n past int32
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    from simplegaussiansplat_tk71_amd import _lib

    return _lib.load()


def _buffers(n=16):
    buf = ctypes.create_string_buffer(256 * (n + 2))
    base = (ctypes.addressof(buf) + 255) & ~255
    return buf, [base + 256 * k for k in range(n)]


def test_the_source_and_its_entry_points_are_built_bound_and_declared(lib):
    from simplegaussiansplat_tk71_amd import _build, _lib

    assert any(s.endswith("gcp_meshclean.hip") for s in _build.SRCS)
    with open(_build.INCLUDE + "/grouped_cumprod_hip.h") as f:
        header = f.read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.gcp_abi_version() == _lib.ABI_VERSION == 4
    assert "shared-EDGE" in header or "shared EDGE" in header  # how Open3D's rule differs is stated
    assert header.index("gcp_mesh_write(") < header.index("gcp_mesh_components(") < header.index("gcp_knn(")  # after the mesh block


def test_workspace_sizes(lib):
    for fn in (lib.gcp_mesh_components_workspace_bytes, lib.gcp_mesh_clean_workspace_bytes, lib.gcp_mesh_vertex_normals_workspace_bytes):
        assert fn(-1, 5) == 0 and fn(5, -1) == 0 and fn(TOO_MANY, 5) == 0 and fn(5, TOO_MANY) == 0
        assert fn(1560, 3096) % 256 == 0
        assert fn(TOO_MANY - 1, TOO_MANY - 1) > 0
    assert lib.gcp_mesh_components_workspace_bytes(1560, 3096) >= 4
    # label, size, the sorted sizes and their permutation, keep flags and offsets of both kinds
    assert lib.gcp_mesh_clean_workspace_bytes(1560, 3096) >= 4 * (6 * 1560 + 2 * 3096)
    # corner keys, sorted keys, the permutation, the run starts
    assert lib.gcp_mesh_vertex_normals_workspace_bytes(1560, 3096) >= 4 * (9 * 3096 + 1561)
    assert lib.gcp_mesh_clean_workspace_bytes(0, 0) > 0  # the totals


def test_components_validate_before_any_hip_call(lib):
    """Host memory stands in for device arrays: every call that gets it must return before anything would read it."""
    keep, p = _buffers()

    def call(nf=5, nv=7, faces=p[0], label=p[1], size=p[2], status=p[3], ws=p[4], ws_bytes=BIG):
        return lib.gcp_mesh_components(faces, nf, nv, label, size, status, ws, ws_bytes, None)

    assert call(nv=0) == OK and call(nv=0, nf=0, faces=None, label=None, size=None, status=None, ws=None, ws_bytes=0) == OK
    assert call(nf=-1) == INVALID and call(nv=-1) == INVALID and call(nf=TOO_MANY) == INVALID and call(nv=TOO_MANY) == INVALID
    assert call(faces=None) == INVALID and call(label=None) == INVALID and call(size=None) == INVALID and call(ws=None) == INVALID
    assert call(ws_bytes=16) == WORKSPACE and call(ws=p[4] + 8) == WORKSPACE
    del keep


def test_select_and_compact_validate_before_any_hip_call(lib):
    keep, p = _buffers()
    totals = (ctypes.c_int64 * 2)(7, 7)

    def select(nf=5, nv=7, k=50, m=50, faces=p[0], ws=p[1], ws_bytes=BIG, out=totals):
        return lib.gcp_mesh_select(faces, nf, nv, k, m, ws, ws_bytes, out, None)

    def compact(nf=5, nv=7, nv_out=3, nf_out=1, faces=p[0], v=p[2], c=p[3], n=p[4], ws=p[1], ws_bytes=BIG, v_out=p[5], f_out=p[6], c_out=p[7],
                n_out=p[8]):
        return lib.gcp_mesh_compact(faces, nf, nv, v, c, n, ws, ws_bytes, nv_out, nf_out, v_out, f_out, c_out, n_out, None)

    assert select(nf=0) == OK and (totals[0], totals[1]) == (0, 0)  # nothing kept, nothing launched
    totals[0] = totals[1] = 7
    assert select(nv=0, faces=None, ws=None, ws_bytes=0) == OK and (totals[0], totals[1]) == (0, 0)
    for bad in (dict(nf=-1), dict(nv=-1), dict(nf=TOO_MANY), dict(nv=TOO_MANY), dict(k=0), dict(k=-3), dict(m=0), dict(m=-1), dict(out=None),
                dict(faces=None), dict(ws=None)):
        assert select(**bad) == INVALID, bad
    assert select(k=0, nf=0) == INVALID and select(m=0, nv=0) == INVALID  # also with nothing to do
    assert select(ws_bytes=16) == WORKSPACE and select(ws=p[1] + 8) == WORKSPACE
    assert compact(nv_out=0, nf_out=0, faces=None, v=None, ws=None, v_out=None, f_out=None, c_out=None, n_out=None) == OK
    for bad in (dict(nf=-1), dict(nv=-1), dict(nf=TOO_MANY), dict(nv=TOO_MANY), dict(nv_out=-1), dict(nf_out=-1), dict(nv_out=8), dict(nf_out=6),
                dict(faces=None), dict(v=None), dict(ws=None), dict(v_out=None), dict(f_out=None), dict(c=None), dict(n=None)):
        assert compact(**bad) == INVALID, bad  # the last two: colours_out without colours, normals_out without normals
    assert compact(c=None, c_out=None, n=None, n_out=None, ws_bytes=16) == WORKSPACE and compact(ws=p[1] + 8) == WORKSPACE
    del keep


def test_normals_validate_before_any_hip_call(lib):
    keep, p = _buffers()

    def call(nv=7, nf=5, v=p[0], faces=p[1], out=p[2], ws=p[3], ws_bytes=BIG):
        return lib.gcp_mesh_vertex_normals(v, faces, nv, nf, out, ws, ws_bytes, None)

    assert call(nv=0) == OK and call(nv=0, v=None, faces=None, out=None, ws=None, ws_bytes=0) == OK
    for bad in (dict(nf=-1), dict(nv=-1), dict(nf=TOO_MANY), dict(nv=TOO_MANY), dict(v=None), dict(faces=None), dict(out=None), dict(ws=None)):
        assert call(**bad) == INVALID, bad
    assert call(ws_bytes=16) == WORKSPACE and call(ws=p[3] + 8) == WORKSPACE
    del keep


def test_python_refuses_before_the_library():
    from simplegaussiansplat_tk71_amd import gs_model as gm
    from simplegaussiansplat_tk71_amd import mesh

    for name in ("face_components", "vertex_normals", "clean_mesh"):
        assert name in gm.__all__ and name in mesh.__all__ and getattr(gm, name) is getattr(mesh, name)
    v, f = torch.zeros(4, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.face_components(f, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.vertex_normals(v, f)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.clean_mesh(v, f)
    with pytest.raises(RuntimeError, match=r"faces \(F, 3\)"):
        mesh.clean_mesh(v, f.reshape(-1))
    assert "not capturable" in mesh.clean_mesh.__doc__.lower() and "one host read" in mesh.clean_mesh.__doc__.lower()
    assert "capturable" in mesh.face_components.__doc__ and "capturable" in mesh.vertex_normals.__doc__


def test_options_default_to_off():
    from examples import train_cameras as tc
    from simplegaussiansplat_tk71_amd import gs_model as gm
    from simplegaussiansplat_tk71_amd import mesh, ply_io

    a = tc.build_parser().parse_args([])
    assert a.mesh_keep is None and a.mesh_min_faces is None and a.mesh_normals is False
    a = tc.build_parser().parse_args(["--save-mesh", "m.ply", "--mesh-keep", "1", "--mesh-min-faces", "20", "--mesh-normals"])
    assert a.mesh_keep == 1 and a.mesh_min_faces == 20 and a.mesh_normals is True
    help_text = " ".join(tc.build_parser().format_help().split())  # argparse wraps lines
    for option in ("--mesh-keep N", "--mesh-min-faces M"):
        about = help_text[help_text.rindex(option):][:400]  # the option's own entry, not the usage line
        assert "2DGS" in about and "not tuned" in about, option
    sig = inspect.signature(tc.train).parameters
    assert sig["mesh_keep"].default is None and sig["mesh_min_faces"].default is None and sig["mesh_normals"].default is False
    sig = inspect.signature(gm.GS_model_with_param.extract_mesh).parameters
    assert [sig[k].default for k in ("keep_largest", "min_faces", "normals")] == [None, None, False]
    assert "no mesh cleaning" not in gm.GS_model_with_param.extract_mesh.__doc__
    sig = inspect.signature(mesh.clean_mesh).parameters
    assert [sig[k].default for k in ("colours", "normals", "keep_largest", "min_faces")] == [None, None, 50, 50]
    assert inspect.signature(ply_io.save_mesh).parameters["normals"].default is None
    assert inspect.signature(ply_io.load_mesh).parameters["with_normals"].default is False


# ---- mesh files ----------------------------------------------------------------------------------------------------------------
def _mesh():
    v = torch.tensor([[0.0, 0.5, 1.0], [1.25, 0.0, -2.0], [3.0, 1.0, 0.125], [0.0, 0.0, 7.0]])
    f = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    c = torch.tensor([[0.0, 1.0, 0.2], [51 / 255, 102 / 255, 1.0], [1.5, -0.5, 0.5], [0.25, 0.75, 1 / 3]])
    n = torch.tensor([[0.0, 0.0, 1.0], [0.6, 0.0, -0.8], [0.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    return v, f, c, n


@pytest.mark.parametrize("coloured", [False, True])
def test_mesh_files_round_trip_with_normals(tmp_path, coloured):
    from simplegaussiansplat_tk71_amd import ply_io

    v, f, c, n = _mesh()
    path = tmp_path / "m.ply"
    ply_io.save_mesh(path, v, f, c if coloured else None, n)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
              "property float nx\nproperty float ny\nproperty float nz\n"
              + ("property uchar red\nproperty uchar green\nproperty uchar blue\n" if coloured else "")
              + "element face 2\nproperty list uchar int vertex_indices\nend_header\n").encode()
    data = path.read_bytes()
    assert data.startswith(header) and len(data) == len(header) + 4 * (24 + (3 if coloured else 0)) + 2 * 13
    assert np.frombuffer(data[len(header) + 12:len(header) + 24], dtype="<f4").tolist() == [0.0, 0.0, 1.0]
    v2, f2, c2, n2 = ply_io.load_mesh(path, with_normals=True)
    assert torch.equal(v2, v) and torch.equal(f2, f) and torch.equal(n2, n) and n2.dtype == torch.float32
    assert (c2 is None) if not coloured else torch.equal(c2, torch.round(c.clamp(0, 1) * 255) / 255)
    default = ply_io.load_mesh(path)  # the 3-tuple, stored normals ignored
    assert len(default) == 3 and torch.equal(default[0], v) and torch.equal(default[1], f)
    with pytest.raises(ValueError, match="normals"):
        ply_io.save_mesh(path, v, f, None, n[:3])


@pytest.mark.parametrize("coloured", [False, True])
def test_mesh_files_without_normals_are_what_they_were(tmp_path, coloured):
    from simplegaussiansplat_tk71_amd import ply_io

    v, f, c, _ = _mesh()
    path = tmp_path / "m.ply"
    ply_io.save_mesh(path, v, f, c if coloured else None)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
              + ("property uchar red\nproperty uchar green\nproperty uchar blue\n" if coloured else "")
              + "element face 2\nproperty list uchar int vertex_indices\nend_header\n").encode()
    rows = b"".join(np.asarray(v[i], dtype="<f4").tobytes()
                    + (bytes(int(x) for x in torch.round(c[i].clamp(0, 1) * 255).tolist()) if coloured else b"") for i in range(4))
    tris = b"".join(b"\x03" + np.asarray(f[i], dtype="<i4").tobytes() for i in range(2))
    assert path.read_bytes() == header + rows + tris  # byte for byte the layout from before normals existed
    loaded = ply_io.load_mesh(path, with_normals=True)
    assert len(loaded) == 4 and loaded[3] is None and torch.equal(loaded[0], v)


# ---- the reference and the fixtures of tests/test_mesh_clean_gpu.py ------------------------------------------------------------
def test_the_blobs_are_what_the_gpu_test_takes_them_for():
    f = cr.blobs_field()
    assert not (f == 0).any()
    v, faces, _ = mr.extract(f)
    label, size = cr.components(faces, len(v))
    assert (len(v), len(faces), tuple(sorted(size[size > 0].tolist(), reverse=True))) == cr.BLOB_COUNTS
    assert np.array_equal(size, np.bincount(label[faces[:, 0]], minlength=len(v))) and (label <= np.arange(len(v))).all()
    for (k, m), kept in (((1, 1), 1), ((2, 1), 3), ((4, 50), 4), ((50, 50), 5), ((50, 1), 6)):
        kv, kf = cr.clean(v, faces, k, m)
        assert cr.euler_per_shell(len(kv), kf) == [2] * kept, (k, m)
        assert np.array_equal(np.unique(kf), np.arange(len(kv)))
    kv, kf = cr.clean(v, faces, 50, 1)
    assert np.array_equal(kv, v) and np.array_equal(kf, faces)


def test_the_strips_are_what_the_gpu_test_takes_them_for():
    v, faces = cr.strips_mesh()
    label, size = cr.components(faces, len(v))
    assert len(v) == 20011 + 17 + 2 + 13
    assert (label == np.arange(len(v))).sum() == 7 + 1 + 1 + 13  # strips, the two fans as one, the pair, the unreferenced
    counts = sorted(size[size > 0].tolist(), reverse=True)
    assert len(counts) == 9 and len(set(counts[:7])) == 7 and 14 in counts and 1 in counts and sum(counts) == len(faces)
    kv, kf = cr.clean(v, faces, 3, 1)
    assert len(kf) == sum(counts[:3]) and np.array_equal(np.unique(kf), np.arange(len(kv)))


def test_the_normal_reference_on_a_closed_form():
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    faces = np.asarray([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])  # a tetrahedron, outward
    n, kappa, valence = cr.vertex_normals(v, faces)
    assert np.allclose(n[0], -np.ones(3) / np.sqrt(3)) and valence.tolist() == [3, 3, 3, 3]
    assert np.isclose(kappa[0], np.sqrt(3.0))  # three unit right triangles: sum |b - a| |c - a| = 3, |S| = |(-1, -1, -1)|
    assert np.isclose(cr.normal_bound(kappa, valence)[0], (np.sqrt(3.0) * 6 / 2 * np.sqrt(3.0) + 4) * cr.EPS32)
