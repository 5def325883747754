"""What csrc/gcp_meshclean.hip is tested against, in numpy and scipy (no GPU, no library): the integer statements of the
components and of the selection rule, the order-preserving subset, and the float64 vertex normals with their condition number.
Meshes are (vertices (V, 3), faces (F, 3)) arrays; every face index lies in [0, V)."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from tests import mesh_ref as mr

EPS32 = float(np.finfo(np.float32).eps)


def components(faces, n_vertices):
    """-> (label int64 (V,): the smallest vertex index of the vertex's component under the shared-vertex rule, size int64 (V,): at
    a label the number of faces of that component — a face belongs to the component of its first vertex — and 0 elsewhere)."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    rows = np.concatenate([faces[:, 0], faces[:, 0]])
    cols = np.concatenate([faces[:, 1], faces[:, 2]])
    graph = coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(n_vertices, n_vertices))
    _, member = connected_components(graph, directed=False)
    smallest = np.full(member.max() + 1 if n_vertices else 0, n_vertices, dtype=np.int64)
    np.minimum.at(smallest, member, np.arange(n_vertices))
    label = smallest[member]
    size = np.zeros(n_vertices, dtype=np.int64)
    np.add.at(size, label[faces[:, 0]], 1)
    return label, size


def threshold(size, keep_largest, min_faces):
    """T = max(c_k, m): c_k the k-th largest face count over the components (the smallest count with fewer than k of them).
    Components are the rows with label == index; a component without faces counts 0 and can never reach T >= 1."""
    counts = np.sort(np.asarray(size)[np.asarray(size) > 0])[::-1]
    if len(counts) == 0:
        return int(min_faces)
    ck = counts[keep_largest - 1] if keep_largest <= len(counts) else counts[-1]
    return max(int(ck), int(min_faces))


def clean(vertices, faces, keep_largest, min_faces, *attributes):
    """-> (vertices, faces, *attributes) of the kept components: rows in input order, bit copies, faces renumbered."""
    vertices, faces = np.asarray(vertices), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    label, size = components(faces, len(vertices))
    t = threshold(size, keep_largest, min_faces)
    face_keep = size[label[faces[:, 0]]] >= t
    vert_keep = np.zeros(len(vertices), dtype=bool)
    vert_keep[faces[face_keep].reshape(-1)] = True
    new_id = np.cumsum(vert_keep) - 1
    return (vertices[vert_keep], new_id[faces[face_keep]].astype(np.int32).reshape(-1, 3),
            *(None if a is None else np.asarray(a)[vert_keep] for a in attributes))


def vertex_normals(vertices, faces):
    """float64 -> (n (V, 3) = S / |S| with S_v = sum over the corners naming v of (b - a) x (c - a), rows of zeros where S = 0;
    kappa (V,) = sum |b - a| |c - a| / |S| (inf where S = 0); valence (V,): the number of corners naming v)."""
    v, faces = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = (v[faces[:, n]] for n in range(3))
    cross = np.cross(b - a, c - a)
    weight = np.linalg.norm(b - a, axis=1) * np.linalg.norm(c - a, axis=1)
    total, scale, valence = np.zeros_like(v), np.zeros(len(v)), np.zeros(len(v), dtype=np.int64)
    for n in range(3):
        np.add.at(total, faces[:, n], cross)
        np.add.at(scale, faces[:, n], weight)
        np.add.at(valence, faces[:, n], 1)
    length = np.linalg.norm(total, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        n_hat = np.where(length[:, None] > 0, total / length[:, None], 0.0)
        kappa = np.where(length > 0, scale / length, np.inf)
    return n_hat, kappa, valence


def normal_bound(kappa, valence):
    """|n - n_hat|_inf per vertex for the float32 chain of k_vertex_normals, first order in u = eps32 / 2, from its roundings:
      * an edge component b - a: 1 rounding, relative u;
      * a product u_y w_z of two such: 2 u from the edges + u of its own = 3 u |u_y w_z|; the difference of two products adds
        u (|p1| + |p2|): a cross component is off by at most 4 u (|p1| + |p2|) <= 4 u |b - a| |c - a| (Cauchy-Schwarz);
      * d - 1 additions for valence d (the first one, to 0, is exact), each off by u |partial sum| <= u sum |b - a| |c - a|;
      so every component of S is off by at most (d + 3) u A, A = sum |b - a| |c - a|, and S by sqrt(3) times that in length;
      * normalising moves n by at most |dS| / |S| = sqrt(3) (d + 3) u kappa; the scaling by a power of two is exact;
      * the normalisation itself: squares u, two additions 2 u, halved by the root, + u root + u division = 3.5 u < 4 eps32.
    C = sqrt(3) (d + 3) / 2 in units of eps32 — counted, not fitted."""
    return np.sqrt(3.0) * (np.asarray(valence) + 3) / 2 * EPS32 * np.asarray(kappa) + 4 * EPS32


def euler_per_shell(n_vertices, faces):
    """V - E + F of every connected component of a mesh without unreferenced vertices, as a sorted list."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    label, size = components(faces, n_vertices)
    out = []
    for root in np.nonzero(size > 0)[0]:
        sub = faces[label[faces[:, 0]] == root]
        ids = np.unique(sub)
        chi, _, _ = mr.topology(len(ids), np.searchsorted(ids, sub))
        out.append(chi)
    return sorted(out)


# ---- the fixtures of tests/test_mesh_clean_*.py --------------------------------------------------------------------------------
BLOB_DIMS = (29, 17, 9)
BLOBS = (((5.37, 5.21, 4.13), 3.6), ((13.29, 4.17, 4.23), 2.3), ((20.29, 4.17, 4.23), 2.3), ((13.41, 11.63, 4.31), 1.7),
         ((19.57, 11.29, 4.07), 1.2), ((25.43, 11.61, 4.37), 0.8))
BLOB_COUNTS = (1560, 3096, (1432, 584, 584, 300, 148, 48))  # vertices, faces, faces per component


def blobs_field():
    f = mr.sphere_field(BLOB_DIMS, *BLOBS[0])
    for centre, radius in BLOBS[1:]:
        f = np.minimum(f, mr.sphere_field(BLOB_DIMS, centre, radius))
    return f


def strips_mesh(seed=5):
    """The arbitrary-numbering case -> (vertices float32 (V, 3), faces int32 (F, 3)): a triangle strip of 20 011 vertices cut into
    7 strips of unequal length, two fans that share exactly one vertex, 13 unreferenced vertices, one face repeated, one face
    naming a vertex twice; vertex ids scrambled by a fixed permutation, the faces shuffled."""
    rng = np.random.default_rng(seed)
    n_strip = 20011
    cuts = {1500, 1501, 4200, 4201, 9001, 9002, 9700, 9701, 15000, 15001, 19800, 19801}  # a cut removes two faces in a row: 7 strips
    faces = [(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(n_strip - 2) if i not in cuts]
    at = n_strip
    hub = at  # two fans around one shared vertex: one component under the shared-vertex rule
    for first in (at + 1, at + 9):
        ring = list(range(first, first + 8))
        faces += [(hub, ring[j], ring[j + 1]) for j in range(7)]
    at += 17
    faces.append(faces[100])            # repeated
    faces.append((at, at, at + 1))      # names a vertex twice; a component of two vertices and one face
    at += 2
    n_vertices = at + 13                # 13 unreferenced
    perm = rng.permutation(n_vertices)
    faces = perm[np.asarray(faces, dtype=np.int64)]
    faces = faces[rng.permutation(len(faces))].astype(np.int32)
    vertices = rng.standard_normal((n_vertices, 3)).astype(np.float32)
    return vertices, faces
