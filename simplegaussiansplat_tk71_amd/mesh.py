"""A triangle mesh out of rendered depth maps, on the HIP library (csrc/gcp_tsdf.hip): `TSDFVolume` fuses depth / alpha
(/ colour) maps into a truncated signed distance volume, `extract_surface` takes the level set of any such volume out as an
indexed mesh by marching tetrahedra.  The float64 statements both are tested against: tests/mesh_ref.py.  GPU tensors only.
`face_components`, `clean_mesh` and `vertex_normals` (csrc/gcp_meshclean.hip) finish the mesh: connected components, 2DGS's
keep-the-largest-clusters rule with an order-preserving compaction, area-weighted vertex normals; their integer / float64
statements: tests/mesh_clean_ref.py.
`GS_model_with_param.extract_mesh` drives them from a trained model; `ply_io.save_mesh` writes the result."""
import ctypes

import torch

from . import _lib

__all__ = ["TSDFVolume", "clean_mesh", "extract_surface", "face_components", "vertex_normals"]


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _dims(dims):
    try:
        nx, ny, nz = (int(d) for d in dims)
    except (TypeError, ValueError):
        raise RuntimeError(f"dims: (nx, ny, nz) expected, got {dims!r}") from None
    if min(nx, ny, nz) < 2 or nx * ny * nz >= 2 ** 31:
        raise RuntimeError(f"dims: every dimension >= 2 and fewer than 2^31 lattice points expected, got {(nx, ny, nz)}")
    return nx, ny, nz


def _origin(origin):
    if torch.is_tensor(origin):
        origin = origin.detach().cpu().tolist()
    origin = tuple(float(o) for o in origin)
    if len(origin) != 3:
        raise RuntimeError("origin: three coordinates expected")
    return origin


def extract_surface(tsdf, weight=None, rgb=None, origin=(0.0, 0.0, 0.0), voxel=1.0, iso=0.0):
    """The level set `tsdf = iso` as an indexed triangle mesh -> (vertices float32 (V, 3), faces int32 (F, 3), colours float32
    (V, 3) or None), by marching tetrahedra (csrc/gcp_tsdf.hip; include/grouped_cumprod_hip.h pins every rule).
    tsdf (nz, ny, nx) float32 on the GPU, x fastest: point (i, j, k) sits at origin + voxel (i, j, k).  weight (nz, ny, nx) or
    None: a cell counts only when all 8 corners have weight > 0 (None: every cell).  rgb (3, nz, ny, nx) or None: interpolated
    like the positions.  A corner is inside when tsdf < iso; faces are counter-clockwise seen from where tsdf grows — out of the
    surface, towards the cameras that saw it.  Every cell is cut into the 6 Kuhn tetrahedra: watertight by construction, no
    case table.  Vertices are ordered by (owner point, edge kind), faces by (cell, tetrahedron, triangle): two calls give the
    same bits.  No vertex is duplicated or unreferenced; zero-area triangles are kept (the topology stays a manifold).
    An all-outside or all-invalid volume gives (0, 3) tensors.
    Count, two prefix sums, ONE host read of the two totals to size the outputs, write: extraction is a one-off and it is
    NOT capturable.  A mesh whose 3 V or 3 F does not fit int32 is refused."""
    if not (torch.is_tensor(tsdf) and tsdf.dim() == 3):
        raise RuntimeError("extract_surface expects tsdf (nz, ny, nx)")
    if not tsdf.is_cuda:
        raise RuntimeError("extract_surface is a HIP kernel: tensors must live on the GPU (no CPU path)")
    nz, ny, nx = tsdf.shape
    _dims((nx, ny, nz))
    if weight is not None and (tuple(weight.shape) != (nz, ny, nx) or weight.device != tsdf.device):
        raise RuntimeError(f"weight: expected {(nz, ny, nx)} on {tsdf.device}, or None")
    if rgb is not None and (tuple(rgb.shape) != (3, nz, ny, nx) or rgb.device != tsdf.device):
        raise RuntimeError(f"rgb: expected {(3, nz, ny, nx)} on {tsdf.device}, or None")
    if not float(voxel) > 0.0:
        raise RuntimeError("voxel: a positive number expected")
    ox, oy, oz = _origin(origin)
    f = tsdf.detach().contiguous().float()
    w = None if weight is None else weight.detach().contiguous().float()
    c = None if rgb is None else rgb.detach().contiguous().float()
    dev = f.device
    lib = _lib.load()
    totals = (ctypes.c_int64 * 2)()
    with torch.cuda.device(dev):
        ws = torch.empty(lib.gcp_mesh_workspace_bytes(nx, ny, nz), dtype=torch.uint8, device=dev)
        _lib.check(lib.gcp_mesh_count(f.data_ptr(), None if w is None else w.data_ptr(), nx, ny, nz, float(iso), ws.data_ptr(), ws.numel(),
                                      totals, _stream(dev)), "gcp_mesh_count")
        n_vert, n_face = int(totals[0]), int(totals[1])
        vertices = torch.empty(n_vert, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(n_face, 3, dtype=torch.int32, device=dev)
        colours = None if c is None else torch.empty(n_vert, 3, dtype=torch.float32, device=dev)
        _lib.check(lib.gcp_mesh_write(f.data_ptr(), None if c is None else c.data_ptr(), nx, ny, nz, ox, oy, oz, float(voxel), float(iso),
                                      ws.data_ptr(), ws.numel(), n_vert, n_face, vertices.data_ptr() if n_vert else None,
                                      faces.data_ptr() if n_face else None, None if (c is None or not n_vert) else colours.data_ptr(),
                                      _stream(dev)), "gcp_mesh_write")
    return vertices, faces, colours


# ---- cleaning and normals (csrc/gcp_meshclean.hip) -----------------------------------------------------------------------------
def _faces(faces, what):
    if not (torch.is_tensor(faces) and faces.dim() == 2 and faces.shape[1] == 3):
        raise RuntimeError(f"{what} expects faces (F, 3)")
    if not faces.is_cuda:
        raise RuntimeError(f"{what} is a HIP kernel: tensors must live on the GPU (no CPU path)")
    if faces.dtype != torch.int32:
        raise RuntimeError(f"{what}: faces must be int32 (what extract_surface returns), got {faces.dtype}")
    return faces.detach().contiguous()


def _rows(t, n, device, name, what):
    if t is None:
        return None
    if not (torch.is_tensor(t) and tuple(t.shape) == (n, 3) and t.device == device):
        raise RuntimeError(f"{what}: {name} ({n}, 3) on {device} expected, or None")
    return t.detach().contiguous().float()


def _mesh_sizes(n_vertices, n_faces, what):
    if n_vertices < 0 or 3 * n_vertices >= 2 ** 31 or 3 * n_faces >= 2 ** 31:
        raise RuntimeError(f"{what}: 3 V and 3 F must fit int32, got V = {n_vertices}, F = {n_faces}")


def face_components(faces, n_vertices):
    """The connected components of an indexed triangle list -> (label int32 (V,), size int32 (V,)), on the HIP library
    (csrc/gcp_meshclean.hip; include/grouped_cumprod_hip.h pins every rule).  faces (F, 3) int32 on the GPU over `n_vertices`
    vertices: any triangle list — unreferenced vertices, repeated faces, faces naming a vertex twice, ids in any order.
    The rule: two vertices belong together when a face names both (shared VERTEX; Open3D's cluster_connected_triangles joins
    over a shared edge — the same thing on a manifold such as `extract_surface`'s).  label[v]: the smallest vertex index of v's
    component; size: at a component's label the number of its faces, 0 in every other row.
    The order: none to choose — both outputs are functions of the mesh alone, the same bits on every run (a lock-free union-find
    that always hooks the larger root under the smaller; integer atomics for the counts).
    A face with an index outside [0, V) is never addressed through; here it is ignored.  No host read: capturable."""
    f = _faces(faces, "face_components")
    n_vertices, n_faces, dev = int(n_vertices), f.shape[0], f.device
    _mesh_sizes(n_vertices, n_faces, "face_components")
    lib = _lib.load()
    with torch.cuda.device(dev):
        label = torch.empty(n_vertices, dtype=torch.int32, device=dev)
        size = torch.empty(n_vertices, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.gcp_mesh_components_workspace_bytes(n_vertices, n_faces), dtype=torch.uint8, device=dev)
        _lib.check(lib.gcp_mesh_components(f.data_ptr() if n_faces else None, n_faces, n_vertices, label.data_ptr() if n_vertices else None,
                                           size.data_ptr() if n_vertices else None, None, ws.data_ptr(), ws.numel(), _stream(dev)),
                   "gcp_mesh_components")
    return label, size


def vertex_normals(vertices, faces):
    """Area-weighted vertex normals -> (V, 3) float32: Open3D's compute_vertex_normals on the HIP library
    (csrc/gcp_meshclean.hip).  vertices (V, 3) float32, faces (F, 3) int32, on the GPU.
    The rule: n_v = normalise(sum of (b - a) x (c - a) over the corners that name v, (a, b, c) the corner's face) — cross
    products are not normalised, so large faces weigh more and zero-area faces nothing; a zero or non-finite sum gives
    (0, 0, 0), never a NaN.  `extract_surface`'s faces are counter-clockwise seen from where the field grows: these normals point
    out of the surface, towards the cameras.
    The order: the corners are stably sorted by vertex and each vertex adds its faces in ascending corner index 3 f + j, in
    float32, nothing fused, no atomics: the same bits on every run.  A face with an index outside [0, V) is left out.
    No host read: capturable."""
    f = _faces(faces, "vertex_normals")
    if not (torch.is_tensor(vertices) and vertices.dim() == 2 and vertices.shape[1] == 3 and vertices.device == f.device):
        raise RuntimeError(f"vertex_normals expects vertices (V, 3) on {f.device}")
    v = vertices.detach().contiguous().float()
    n_vertices, n_faces, dev = v.shape[0], f.shape[0], f.device
    _mesh_sizes(n_vertices, n_faces, "vertex_normals")
    lib = _lib.load()
    with torch.cuda.device(dev):
        normals = torch.empty(n_vertices, 3, dtype=torch.float32, device=dev)
        ws = torch.empty(lib.gcp_mesh_vertex_normals_workspace_bytes(n_vertices, n_faces), dtype=torch.uint8, device=dev)
        _lib.check(lib.gcp_mesh_vertex_normals(v.data_ptr() if n_vertices else None, f.data_ptr() if n_faces else None, n_vertices, n_faces,
                                               normals.data_ptr() if n_vertices else None, ws.data_ptr() if ws.numel() else None, ws.numel(),
                                               _stream(dev)), "gcp_mesh_vertex_normals")
    return normals


def clean_mesh(vertices, faces, colours=None, normals=None, keep_largest=50, min_faces=50):
    """Drop the small connected components of a mesh -> (vertices, faces, colours or None, normals or None): what 2DGS, GOF,
    RaDe-GS and PGSR do with Open3D's post_process_mesh(cluster_to_keep=50) after the fusion, on the HIP library
    (csrc/gcp_meshclean.hip).  vertices (V, 3) float32, faces (F, 3) int32, colours / normals (V, 3) float32 or None, on the GPU.
    The rule, 2DGS's: with c_k the `keep_largest`-th largest face count of the components of `face_components` (the smallest
    count if there are fewer) and T = max(c_k, min_faces), a component stays iff it has at least T faces.  Ties at the threshold
    all stay: no tie-break, a function of the mesh alone.  A vertex no kept face names is dropped — unreferenced input vertices
    too.  50 / 50 are 2DGS's values: pointers, not tuned here.
    The order: vertices and faces keep their input order (`extract_surface`'s: by (owner, kind) and by (cell, tetrahedron,
    triangle)); kept rows are bit copies, faces are renumbered; with everything kept the outputs equal the inputs bit for bit.
    Components, a sort of the counts, keep flags, two prefix sums, ONE host read of the two totals (and a status word) to size
    the outputs, write: NOT capturable.  A face index outside [0, V) is never addressed through and raises from that read."""
    f = _faces(faces, "clean_mesh")
    if not (torch.is_tensor(vertices) and vertices.dim() == 2 and vertices.shape[1] == 3 and vertices.device == f.device):
        raise RuntimeError(f"clean_mesh expects vertices (V, 3) on {f.device}")
    keep_largest, min_faces = int(keep_largest), int(min_faces)
    if keep_largest < 1 or min_faces < 1:
        raise RuntimeError(f"clean_mesh: keep_largest >= 1 and min_faces >= 1 expected, got {keep_largest} and {min_faces}")
    v = vertices.detach().contiguous().float()
    n_vertices, n_faces, dev = v.shape[0], f.shape[0], f.device
    _mesh_sizes(n_vertices, n_faces, "clean_mesh")
    c = _rows(colours, n_vertices, dev, "colours", "clean_mesh")
    n = _rows(normals, n_vertices, dev, "normals", "clean_mesh")
    lib = _lib.load()
    totals = (ctypes.c_int64 * 2)()
    ptr = lambda t, rows: t.data_ptr() if (t is not None and rows) else None  # noqa: E731
    with torch.cuda.device(dev):
        ws = torch.empty(lib.gcp_mesh_clean_workspace_bytes(n_vertices, n_faces), dtype=torch.uint8, device=dev)
        _lib.check(lib.gcp_mesh_select(ptr(f, n_faces), n_faces, n_vertices, keep_largest, min_faces, ws.data_ptr(), ws.numel(), totals,
                                       _stream(dev)), "gcp_mesh_select")
        kept_v, kept_f = int(totals[0]), int(totals[1])
        v_out = torch.empty(kept_v, 3, dtype=torch.float32, device=dev)
        f_out = torch.empty(kept_f, 3, dtype=torch.int32, device=dev)
        c_out = None if c is None else torch.empty(kept_v, 3, dtype=torch.float32, device=dev)
        n_out = None if n is None else torch.empty(kept_v, 3, dtype=torch.float32, device=dev)
        _lib.check(lib.gcp_mesh_compact(ptr(f, n_faces), n_faces, n_vertices, ptr(v, n_vertices), ptr(c, n_vertices), ptr(n, n_vertices),
                                        ws.data_ptr(), ws.numel(), kept_v, kept_f, ptr(v_out, kept_v), ptr(f_out, kept_f), ptr(c_out, kept_v),
                                        ptr(n_out, kept_v), _stream(dev)), "gcp_mesh_compact")
    return v_out, f_out, c_out, n_out


class TSDFVolume:
    """A dense truncated signed distance volume on the GPU: `dims = (nx, ny, nz)` lattice points, x fastest, point (i, j, k) at
    origin + voxel (i, j, k) in world coordinates.  State, float32: `.tsdf` (nz, ny, nx), `.weight` (nz, ny, nx) and, with
    colour=True, `.rgb` (3, nz, ny, nx), else None.  A fresh (or `reset()`) volume has tsdf = 1, weight = 0, rgb = 0.
    `trunc`: the truncation distance, in world units.  Fewer than 2^31 points, every dimension >= 2, voxel > 0, trunc > 0."""

    def __init__(self, origin, voxel, dims, trunc, device, colour=True):
        self.nx, self.ny, self.nz = _dims(dims)
        self.origin = _origin(origin)
        self.voxel, self.trunc = float(voxel), float(trunc)
        if not (self.voxel > 0.0 and self.trunc > 0.0):
            raise RuntimeError("voxel and trunc: positive numbers expected")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TSDFVolume is integrated by a HIP kernel: it must live on the GPU (no CPU path)")
        shape = (self.nz, self.ny, self.nx)
        self.tsdf = torch.ones(shape, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.rgb = torch.zeros((3, *shape), dtype=torch.float32, device=self.device) if colour else None

    def reset(self):
        """Back to the fresh state, in place."""
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        if self.rgb is not None:
            self.rgb.zero_()
        return self

    @torch.no_grad()
    def integrate(self, depth, alpha, P, K, image=None, alpha_min=0.5, depth_max=0.0):
        """Fuse B cameras' maps into the volume, in place, in one launch.  depth, alpha (B, 1, H, W): what `render` and
        `cuda_kernel.paint_maps` return after the [1:, 1:] crop — depth NOT divided by alpha; image (B, 3, H, W): required by a
        colour volume, ignored otherwise; P (B, 3, 4) world->camera, K (B, 3, 3), on the volume's device (the kernel reads them).
        Per lattice point, for the cameras in order: p = R x_w + t, z = p.z > 0; (u, v) = (fx p.x / z + cx, fy p.y / z + cy)
        inside [0, W) x [0, H) — pixel centres at +0.5 in K's coordinates, nearest pixel (x, y) = floor; a = alpha, D = depth
        there with a >= alpha_min and D > 0 (a NaN skips); d = D / a, not beyond depth_max if that is > 0; s = d - z >= -trunc;
        tsdf <- (tsdf w + min(1, s / trunc)) / (w + 1), rgb likewise, w <- w + 1: Open3D's projective z-depth TSDF with unit
        weights.  float32 state, cameras in order, no atomics: integrating B cameras at once, one at a time or in any split
        gives the same bits.  Nothing is read back: capturable.  alpha_min = 0.5 is a pointer from 2DGS's usage, not tuned."""
        if not (torch.is_tensor(depth) and depth.dim() == 4 and depth.shape[1] == 1 and alpha.shape == depth.shape):
            raise RuntimeError("integrate expects depth and alpha of one shape (B, 1, H, W)")
        b, _, h, w = depth.shape
        if tuple(P.shape) != (b, 3, 4) or tuple(K.shape) != (b, 3, 3):
            raise RuntimeError(f"integrate expects P (B, 3, 4) and K (B, 3, 3) with B = {b}")
        maps = [depth, alpha, P, K]
        if self.rgb is not None:
            if image is None or tuple(image.shape) != (b, 3, h, w):
                raise RuntimeError(f"integrate: a colour volume needs image ({b}, 3, {h}, {w})")
            maps.append(image)
        if any(t.device != self.device for t in maps):
            raise RuntimeError(f"integrate: every tensor must live on {self.device} (P and K too: the kernel reads them)")
        maps = [t.detach().contiguous().float() for t in maps]
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gcp_tsdf_integrate(
                self.tsdf.data_ptr(), self.weight.data_ptr(), None if self.rgb is None else self.rgb.data_ptr(), self.nx, self.ny, self.nz,
                *self.origin, self.voxel, self.trunc, maps[0].data_ptr(), maps[1].data_ptr(),
                maps[4].data_ptr() if self.rgb is not None else None, maps[2].data_ptr(), maps[3].data_ptr(), b, h, w, float(alpha_min),
                float(depth_max), _stream(self.device)), "gcp_tsdf_integrate")
        return self

    def extract(self, iso=0.0):
        """`extract_surface` of this volume: only cells whose 8 corners were all observed (weight > 0) are cut."""
        return extract_surface(self.tsdf, self.weight, self.rgb, self.origin, self.voxel, iso)
