"""Scenes as standard 3DGS .ply files: what viewers and other trainers read and write.  numpy only.

Layout (binary little-endian, every property `float`), one vertex per Gaussian, nb = (degree + 1)^2:

    x y z  nx ny nz  f_dc_0..2  f_rest_0..(3 (nb - 1) - 1)  opacity  scale_0..2  rot_0..3

  * f_rest is channel-major: f_rest_[c (nb - 1) + (k - 1)] = color[:, k, c];
  * rot is (w, x, y, z); this project keeps (x, y, z, w).  Stored un-normalised, as it is;
  * opacity is the logit and scale_* the log, both as stored; the normals are zeros.

convention="3dgs": other renderers add 0.5 to the SH sum, this project does not, so the file holds
f_dc = color[:, 0, :] - 0.5 / C0 and loading undoes it (two fp32 roundings on the DC row).  convention="raw" writes
the numbers as they are: an exact resume, but a file other renderers show 0.5 too bright.

Other renderers evaluate the SH basis on world-space directions: train with `sh_frame="world"` for a file whose view
dependence means the same elsewhere (GS_model_with_param.save_ply warns otherwise).
"""
import numpy as np
import torch

__all__ = ["save_ply", "load_ply", "property_names", "save_mesh", "load_mesh"]

SH_C0 = 0.28209479177387814
CONVENTIONS = ("3dgs", "raw")
_REST_COUNTS = {0: 0, 9: 1, 24: 2, 45: 3}  # number of f_rest_* properties -> degree


def property_names(n_basis):
    """The vertex properties of a scene with `n_basis` SH coefficients per channel, in file order."""
    return (["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(3 * (n_basis - 1))]
            + ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)])


def _dc_shift(convention):
    if convention not in CONVENTIONS:
        raise ValueError(f"convention: one of {CONVENTIONS}, got {convention!r}")
    return np.float32(0.5 / SH_C0) if convention == "3dgs" else None


def save_ply(path, mean, variance_q, variance_scale, opacity, color, convention="3dgs"):
    """Write the five parameter tensors (mean (N,3), variance_q (N,4 xyzw), variance_scale (N,3 log), opacity (N,1 logit),
    color (N,nb,3) with nb in {1, 4, 9, 16}) to `path`."""
    shift = _dc_shift(convention)
    mean, q, scale, opacity, color = (np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
                                      for t in (mean, variance_q, variance_scale, opacity, color))
    n = mean.shape[0]
    nb = color.shape[1] if color.ndim == 3 else 0
    if nb not in (1, 4, 9, 16) or color.shape != (n, nb, 3):
        raise ValueError(f"color: (N, 1 | 4 | 9 | 16, 3), got {color.shape}")
    if mean.shape != (n, 3) or q.shape != (n, 4) or scale.shape != (n, 3) or opacity.reshape(n, -1).shape != (n, 1):
        raise ValueError("mean (N,3), variance_q (N,4), variance_scale (N,3), opacity (N,1) expected")
    names = property_names(nb)
    rows = np.zeros((n, len(names)), dtype="<f4")  # the normals stay zero
    rows[:, 0:3] = mean
    rows[:, 6:9] = color[:, 0, :] if shift is None else color[:, 0, :] - shift
    rows[:, 9:9 + 3 * (nb - 1)] = color[:, 1:, :].transpose(0, 2, 1).reshape(n, 3 * (nb - 1))  # channel-major
    at = 9 + 3 * (nb - 1)
    rows[:, at] = opacity.reshape(n)
    rows[:, at + 1:at + 4] = scale
    rows[:, at + 4:at + 8] = q[:, [3, 0, 1, 2]]  # (x, y, z, w) -> (w, x, y, z)
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {n}\n" + "".join(f"property float {p}\n" for p in names) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rows.tobytes())


def _read_header(f):
    """-> (vertex count, [property names of the vertex element]); raises ValueError for what load_ply does not read."""
    if f.readline().strip() != b"ply":
        raise ValueError("not a .ply file")
    fmt, n, names, element, seen_vertex = None, None, [], None, False
    while True:
        raw = f.readline()
        if not raw:
            raise ValueError("the .ply header does not end")
        words = raw.decode("ascii", errors="replace").split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "end_header":
            break
        if words[0] == "format":
            fmt = words[1] if len(words) > 1 else None
        elif words[0] == "element":
            if len(words) != 3:
                raise ValueError(f"malformed .ply header line: {raw!r}")
            element = words[1]
            if element == "vertex":
                if seen_vertex:
                    raise ValueError("two vertex elements")
                seen_vertex, n = True, int(words[2])
            elif not seen_vertex:
                raise ValueError(f"element {element!r} in front of the vertices is not supported")
        elif words[0] == "property" and element == "vertex":
            if len(words) != 3 or words[1] not in ("float", "float32"):
                raise ValueError(f"vertex property {' '.join(words[1:])!r}: only float properties are supported")
            names.append(words[2])
    if fmt != "binary_little_endian":
        raise ValueError(f".ply format {fmt!r}: only binary_little_endian is supported")
    if n is None:
        raise ValueError("the .ply file has no vertex element")
    return n, names


def load_ply(path, device="cpu", convention="3dgs"):
    """-> (mean, variance_q, variance_scale, opacity, color) on `device`, the inverse of save_ply.  The SH degree follows
    from the number of f_rest_* properties (0, 9, 24 or 45); float properties with other names are ignored."""
    shift = _dc_shift(convention)
    with open(path, "rb") as f:
        n, names = _read_header(f)
        body = f.read(4 * n * len(names))
    if len(body) != 4 * n * len(names):
        raise ValueError(f"{path}: {n} vertices of {len(names)} floats expected, the file is shorter")
    if len(set(names)) != len(names):
        raise ValueError("a vertex property is listed twice")
    rows = np.frombuffer(body, dtype="<f4").reshape(n, len(names))
    col = {p: i for i, p in enumerate(names)}
    n_rest = sum(1 for p in names if p.startswith("f_rest_"))
    if n_rest not in _REST_COUNTS:
        raise ValueError(f"{n_rest} f_rest_* properties: 0, 9, 24 or 45 (degree 0..3) expected")
    nb = (_REST_COUNTS[n_rest] + 1) ** 2
    required = [p for p in property_names(nb) if p not in ("nx", "ny", "nz")]
    missing = [p for p in required if p not in col]
    if missing:
        raise ValueError(f"missing vertex properties: {', '.join(missing)}")

    def take(props):
        return np.ascontiguousarray(rows[:, [col[p] for p in props]], dtype=np.float32)

    color = np.empty((n, nb, 3), dtype=np.float32)
    dc = take([f"f_dc_{i}" for i in range(3)])
    color[:, 0, :] = dc if shift is None else dc + shift
    color[:, 1:, :] = take([f"f_rest_{i}" for i in range(3 * (nb - 1))]).reshape(n, 3, nb - 1).transpose(0, 2, 1)
    out = (take(["x", "y", "z"]), take(["rot_1", "rot_2", "rot_3", "rot_0"]), take([f"scale_{i}" for i in range(3)]),
           take(["opacity"]), color)
    return tuple(torch.from_numpy(a).to(device) for a in out)


# ---- triangle meshes (mesh.py) -------------------------------------------------------------------------------------------------
def _mesh_header(n_vert, n_face, coloured, with_normals=False):
    return ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {n_vert}\n" + "property float x\nproperty float y\nproperty float z\n"
            + ("property float nx\nproperty float ny\nproperty float nz\n" if with_normals else "")
            + ("property uchar red\nproperty uchar green\nproperty uchar blue\n" if coloured else "")
            + f"element face {n_face}\n" + "property list uchar int vertex_indices\nend_header\n")


def _mesh_dtypes(coloured, with_normals=False):
    vertex = ([("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")] if with_normals else [])
              + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if coloured else []))
    return np.dtype(vertex), np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def save_mesh(path, vertices, faces, colours=None, normals=None):
    """Write an indexed triangle mesh (mesh.extract_surface's outputs) as a binary little-endian .ply that MeshLab, Blender and
    Open3D read: vertex `x y z` float, plus `nx ny nz` float when `normals` (V, 3) is given (mesh.vertex_normals'; between z
    and red, where those programs look for them), plus `red green blue` uchar when `colours` (V, 3) in [0, 1] is given (clamped,
    scaled by 255 and rounded); face `property list uchar int vertex_indices`, three indices each.  vertices (V, 3), faces (F, 3)
    with indices in [0, V); tensors or arrays; V = 0 or F = 0 is a valid (empty) file.  Without normals the file is byte for byte
    what it was before normals existed."""
    as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)  # noqa: E731
    v, f = as_np(vertices), as_np(faces)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"vertices (V, 3) and faces (F, 3) expected, got {v.shape} and {f.shape}")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("faces: an index outside [0, V)")
    vertex_t, face_t = _mesh_dtypes(colours is not None, normals is not None)
    rows = np.zeros(v.shape[0], dtype=vertex_t)
    rows["x"], rows["y"], rows["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        n = as_np(normals)
        if n.shape != v.shape:
            raise ValueError(f"normals: {v.shape} expected, got {n.shape}")
        rows["nx"], rows["ny"], rows["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if colours is not None:
        c = as_np(colours)
        if c.shape != v.shape:
            raise ValueError(f"colours: {v.shape} expected, got {c.shape}")
        c8 = np.rint(np.clip(np.nan_to_num(c.astype(np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8)
        rows["red"], rows["green"], rows["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
    tris = np.zeros(f.shape[0], dtype=face_t)
    tris["n"], tris["v"] = 3, f
    with open(path, "wb") as out:
        out.write(_mesh_header(v.shape[0], f.shape[0], colours is not None, normals is not None).encode("ascii"))
        out.write(rows.tobytes())
        out.write(tris.tobytes())


def load_mesh(path, device="cpu", with_normals=False):
    """-> (vertices float32 (V, 3), faces int32 (F, 3), colours float32 (V, 3) in [0, 1] or None) on `device`: the inverse of
    save_mesh (colours come back as multiples of 1 / 255).  with_normals=True: a fourth element, the stored normals float32
    (V, 3), or None if the file has none; by default stored normals are ignored.  Reads the layouts save_mesh writes and
    nothing else."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError("not a .ply file")
    header, body = data[:end + 11].decode("ascii", errors="replace"), data[end + 11:]
    lines = [ln.split() for ln in header.splitlines() if ln and not ln.startswith(("comment", "obj_info"))]
    elements = [(ln[1], int(ln[2])) for ln in lines if ln[0] == "element" and len(ln) == 3]
    if [e[0] for e in elements] != ["vertex", "face"]:
        raise ValueError("a vertex element followed by a face element expected")
    (_, n_vert), (_, n_face) = elements
    for coloured, has_normals in ((False, False), (True, False), (False, True), (True, True)):
        if header == _mesh_header(n_vert, n_face, coloured, has_normals):
            break
    else:
        raise ValueError(f"{path}: not the mesh layout save_mesh writes (binary little-endian; x y z float [nx ny nz float] "
                         "[red green blue uchar]; list uchar int vertex_indices)")
    vertex_t, face_t = _mesh_dtypes(coloured, has_normals)
    if len(body) != n_vert * vertex_t.itemsize + n_face * face_t.itemsize:
        raise ValueError(f"{path}: {n_vert} vertices and {n_face} faces expected, the file's length does not match")
    rows = np.frombuffer(body, dtype=vertex_t, count=n_vert)
    tris = np.frombuffer(body, dtype=face_t, count=n_face, offset=n_vert * vertex_t.itemsize)
    if n_face and not (tris["n"] == 3).all():
        raise ValueError("only triangles are supported")
    v = np.stack([rows["x"], rows["y"], rows["z"]], axis=1).astype(np.float32)
    c = np.stack([rows["red"], rows["green"], rows["blue"]], axis=1).astype(np.float32) / np.float32(255.0) if coloured else None
    faces = np.zeros((n_face, 3), dtype=np.int32)
    faces[:] = tris["v"]
    out = (torch.from_numpy(v).to(device), torch.from_numpy(faces).to(device), None if c is None else torch.from_numpy(c).to(device))
    if not with_normals:
        return out
    n = np.stack([rows["nx"], rows["ny"], rows["nz"]], axis=1).astype(np.float32) if has_normals else None
    return out + (None if n is None else torch.from_numpy(n).to(device),)
