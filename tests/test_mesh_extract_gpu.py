"""Marching tetrahedra (csrc/gcp_tsdf.hip: k_mesh_cells / _edges / _vertices / _faces, mesh.extract_surface) on the GPU, on the
analytic float32 fields of tests/mesh_ref.py (no lattice value is exactly 0): exact vertex and face counts, every edge in two
faces once in each direction, the Euler characteristic, every vertex on its lattice edge within a few ulp of the float64
interpolation, the enclosed volume, the face set of the slow reference extractor, cell validity, iso != 0, colours, and the same
bits on every run.  The grids are a few thousand points: more than one block of 256, rows that are no multiple of a wave."""
import numpy as np
import pytest
import torch

from tests import mesh_cases as mc
from tests import mesh_ref as mr

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
ORIGIN, VOXEL = (-1.37, 0.61, 2.03), 0.173


def run(device, f, weight=None, rgb=None, origin=ORIGIN, voxel=VOXEL, iso=0.0):
    from simplegaussiansplat_tk71_amd.mesh import extract_surface

    as_dev = lambda a: None if a is None else torch.as_tensor(np.asarray(a), dtype=torch.float32).to(device)  # noqa: E731
    v, faces, colours = extract_surface(as_dev(f), as_dev(weight), as_dev(rgb), origin=origin, voxel=voxel, iso=iso)
    assert v.dtype == torch.float32 and faces.dtype == torch.int32 and v.shape[1:] == (3,) and faces.shape[1:] == (3,)
    return v.cpu().numpy(), faces.cpu().numpy(), None if colours is None else colours.cpu().numpy()


def edge_interpolation(f, keys_ijk, kinds, origin, voxel, iso, values=None):
    """float64: the point (or the value of `values` (C, nz, ny, nx)) at t = (iso - f_p) / (f_q - f_p) on the edge from owner p."""
    f = np.asarray(f, dtype=np.float64)
    d = np.asarray(mr.KINDS)[kinds]
    p, q = keys_ijk, keys_ijk + d
    fp, fq = f[p[:, 2], p[:, 1], p[:, 0]], f[q[:, 2], q[:, 1], q[:, 0]]
    t = (iso - fp) / (fq - fp)
    if values is None:
        o, vx = np.asarray(np.float32(origin), dtype=np.float64), float(np.float32(voxel))
        xp, xq = o + vx * p, o + vx * q
    else:
        values = np.asarray(values, dtype=np.float64)
        xp, xq = values[:, p[:, 2], p[:, 1], p[:, 0]].T, values[:, q[:, 2], q[:, 1], q[:, 0]].T
    return xp + t[:, None] * (xq - xp), (fp < iso) != (fq < iso)


def owned_edges(f, valid, iso):
    """The (owner (i, j, k), kind) of every vertex, in output order: by owner index (x fastest), then kind."""
    inside = np.asarray(f) < iso
    nz, ny, nx = inside.shape
    rows = []
    for n, kind in enumerate(mr.KINDS):
        dx, dy, dz = kind
        change = (inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]) & mr.edge_has_valid_cell(valid, kind)
        k, j, i = np.nonzero(change)
        rows.append(np.stack([(k * ny + j) * nx + i, np.full_like(i, n), i, j, k], axis=1))
    rows = np.concatenate(rows)
    rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
    return rows[:, 2:5], rows[:, 1]


def check_mesh(f, v, faces, valid=None, origin=ORIGIN, voxel=VOXEL, iso=0.0):
    """What holds for every output: exact counts, indices in range, every vertex referenced, every vertex on its edge."""
    nz, ny, nx = f.shape
    if valid is None:
        valid = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
    assert (len(v), len(faces)) == mr.counts(np.asarray(f) < iso, valid)
    if len(faces):
        assert faces.min() >= 0 and faces.max() < len(v)
    assert np.array_equal(np.unique(faces), np.arange(len(v)))  # no unreferenced vertex
    ijk, kinds = owned_edges(f, valid, iso)
    want, crosses = edge_interpolation(f, ijk, kinds, origin, voxel, iso)
    assert crosses.all() and len(want) == len(v)
    bound = 8 * EPS32 * (np.abs(want).max() + voxel * np.sqrt(3.0))
    err = np.abs(v.astype(np.float64) - want).max() if len(v) else 0.0
    print(f"vertices {len(v)}, faces {len(faces)}, position error {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert len(np.unique(np.round(want / (voxel * 1e-6)).astype(np.int64), axis=0)) == len(v) or len(v) == 0  # no duplicated vertex
    return ijk, kinds


CLOSED = [
    ("sphere", lambda: mr.sphere_field(**mr.SPHERE), 2),
    ("torus", lambda: mr.torus_field(**mr.TORUS), 0),
    ("two_spheres", lambda: np.minimum(mr.sphere_field((19, 14, 11), (4.63, 6.57, 5.21), 3.1), mr.sphere_field((19, 14, 11), (13.41, 7.13, 5.33), 3.3)), 4),
]


@pytest.mark.parametrize("name,field,chi", CLOSED, ids=[c[0] for c in CLOSED])
def test_closed_surfaces(device, name, field, chi):
    f = field()
    assert not (f == 0).any()
    v, faces, colours = run(device, f)
    assert colours is None
    check_mesh(f, v, faces)
    got_chi, uses, directed = mr.topology(len(v), faces)
    assert set(uses) == {2} and directed == 1  # every undirected edge in exactly 2 faces, once in each direction
    assert got_chi == chi
    volume = mr.signed_volume(v, faces) / VOXEL ** 3
    assert volume > 0
    if name == "sphere":
        centre, r = np.asarray(mr.SPHERE["centre"]), mr.SPHERE["radius"]
        o, vx = np.asarray(np.float32(ORIGIN), dtype=np.float64), float(np.float32(VOXEL))
        delta = np.abs(np.linalg.norm((v.astype(np.float64) - o) / vx - centre, axis=1) - r).max()
        # delta: the largest vertex distance from the sphere, in float64 (0.088 lattice units here: the field is not linear
        # along an edge); the volume lies between those of the balls of radius r -+ delta
        print(f"sphere: volume {volume:.3f} lattice units, delta {delta:.4f}")
        assert 4 / 3 * np.pi * (r - delta) ** 3 <= volume <= 4 / 3 * np.pi * (r + delta) ** 3


def test_the_same_faces_as_the_slow_extractor(device):
    f = mr.sphere_field((6, 5, 4), (2.63, 2.17, 1.41), 1.7)
    v, faces, _ = run(device, f)
    check_mesh(f, v, faces)
    want_v, want_faces, _ = mr.extract(f, origin=np.asarray(np.float32(ORIGIN), dtype=np.float64), voxel=float(np.float32(VOXEL)))
    assert len(want_v) == len(v) and len(want_faces) == len(faces)
    # match vertices by position (float32 against float64: within the bound of check_mesh, far below the vertex spacing)
    dist = np.linalg.norm(v.astype(np.float64)[:, None, :] - want_v[None, :, :], axis=2)
    match = dist.argmin(axis=1)
    assert dist.min(axis=1).max() < 1e-5 * VOXEL and len(set(match.tolist())) == len(v)
    assert mr.canonical_faces(match[faces]) == mr.canonical_faces(want_faces)


def test_plane_through_the_box(device):
    f = mr.plane_field(**mr.PLANE)
    v, faces, _ = run(device, f)
    ijk, kinds = check_mesh(f, v, faces)
    assert len(v) == 1599
    chi, uses, directed = mr.topology(len(v), faces)
    assert chi == 1 and directed == 1 and set(uses) == {1, 2} and uses[1] == 162
    # boundary edges (used once) lie on the faces of the volume: both end vertices sit on edges inside one face of the box
    nz, ny, nx = f.shape
    upper = np.asarray([nx - 1, ny - 1, nz - 1])
    d = np.asarray(mr.KINDS)[kinds]
    on_low = (ijk == 0) & (d == 0)            # per vertex and axis: its lattice edge lies in the plane coordinate = 0
    on_high = (ijk == upper) & (d == 0)
    count = {}
    for tri in faces.tolist():
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            count[(min(a, b), max(a, b))] = count.get((min(a, b), max(a, b)), 0) + 1
    for (a, b), n in count.items():
        if n == 1:
            assert ((on_low[a] & on_low[b]) | (on_high[a] & on_high[b])).any(), (a, b)


def test_unobserved_slab(device):
    f = mr.sphere_field(**mr.SPHERE)
    weight = mc.slab_weight(f.shape)
    valid = mr.cell_validity(weight)
    v, faces, _ = run(device, f, weight=weight)
    ijk, kinds = check_mesh(f, v, faces, valid=valid)  # the counts with that validity; every vertex next to a valid cell
    assert 0 < len(v) < 1036
    # no face has a vertex on an edge of invalid cells only: check_mesh's owned_edges lists exactly the edges with a valid cell
    for n, kind in enumerate(mr.KINDS):
        has = mr.edge_has_valid_cell(valid, kind)
        sel = kinds == n
        assert has[ijk[sel, 2], ijk[sel, 1], ijk[sel, 0]].all()
    chi, uses, directed = mr.topology(len(v), faces)
    assert directed == 1 and set(uses) == {1, 2}  # cut open along the slab
    all_zero = np.zeros_like(weight)
    v0, f0, _ = run(device, f, weight=all_zero)
    assert v0.shape == (0, 3) and f0.shape == (0, 3)


def test_smallest_volume_and_empty_volume(device):
    f = np.full((2, 2, 2), 0.75, dtype=np.float32)
    f[0, 0, 0] = -0.25  # one inside corner: the 7 owned edges of point 0 are cut, 6 tetrahedra give one triangle each
    v, faces, _ = run(device, f, origin=(0.0, 0.0, 0.0), voxel=1.0)
    check_mesh(f, v, faces, origin=(0.0, 0.0, 0.0), voxel=1.0)
    assert len(v) == 7 and len(faces) == 6
    want = 0.25 * np.asarray([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1]], dtype=np.float64)
    assert np.allclose(v, want, rtol=0, atol=4 * EPS32)  # ordered by edge kind
    a, b, c = (v[faces[:, n]].astype(np.float64) for n in range(3))
    normals = np.cross(b - a, c - a)
    assert (normals @ np.ones(3) > 0).all()  # away from the inside corner, towards increasing f
    v, faces, colours = run(device, np.full((3, 4, 5), 1.0, dtype=np.float32), rgb=np.zeros((3, 3, 4, 5), dtype=np.float32))
    assert v.shape == (0, 3) and faces.shape == (0, 3) and colours.shape == (0, 3)
    v, faces, _ = run(device, np.full((3, 4, 5), -1.0, dtype=np.float32))
    assert v.shape == (0, 3) and faces.shape == (0, 3)


def test_other_level_and_colours(device):
    f = mr.sphere_field(**mr.SPHERE)
    iso = 0.381966
    assert not (f == np.float32(iso)).any()
    x, y, z = mr.grid_xyz(mr.SPHERE["dims"])
    rgb = np.stack([0.05 * x, 0.07 * y, 0.02 * x + 0.03 * y + 0.04 * z]).astype(np.float32)  # linear fields, in [0, 1.3]
    v, faces, colours = run(device, f, rgb=rgb, iso=iso)
    ijk, kinds = check_mesh(f, v, faces, iso=np.float64(np.float32(iso)))
    chi, uses, directed = mr.topology(len(v), faces)
    assert chi == 2 and set(uses) == {2} and directed == 1
    assert len(v) > 1036  # the larger sphere
    want, _ = edge_interpolation(f, ijk, kinds, ORIGIN, VOXEL, np.float64(np.float32(iso)), values=rgb)
    bound = 8 * EPS32 * (np.abs(rgb).max() + np.abs(rgb[:, 1:, 1:, 1:] - rgb[:, :-1, :-1, :-1]).max())  # colour range + edge length
    err = np.abs(colours.astype(np.float64) - want).max()
    print(f"colour error {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_two_runs_give_the_same_bits(device):
    from simplegaussiansplat_tk71_amd.mesh import extract_surface

    f = torch.as_tensor(mr.torus_field(**mr.TORUS)).to(device)
    rgb = torch.rand(3, *f.shape, device=device)
    first = extract_surface(f, rgb=rgb, origin=ORIGIN, voxel=VOXEL)
    second = extract_surface(f, rgb=rgb, origin=ORIGIN, voxel=VOXEL)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
