// gcp_meshclean.hip — what follows the extraction of gcp_tsdf.hip: connected components of an indexed triangle
// list, 2DGS's keep-the-largest-clusters rule, an order-preserving compaction, and area-weighted vertex normals.  Everything is
// integer, or float32 summed in a pinned order: a function of the input alone, the same bits on every run.  The kernels take ANY
// triangle list: unreferenced vertices, repeated faces, faces that name a vertex twice, vertex ids in any order.  A face index
// outside [0, V) is tested BEFORE anything is addressed with it, in every kernel that reads the face list.
//
// 1. Components (shared-VERTEX rule).  A union-find over the vertices, in the `label` output itself:
//      k_cc_init     label[v] = v, size[v] = 0, the status word cleared
//      k_cc_hook     one thread per face (a, b, c): unite(a, b), unite(a, c).  unite walks both to their roots with path halving
//                    and hooks the LARGER root under the smaller with one compare-and-swap; a failed swap hands back the root's
//                    real parent and the walk goes on from there.  Every non-root points at a smaller index of its own set, at
//                    all times and in every (also stale) view, so every walk is a strictly decreasing sequence: lock-free, no
//                    thread waits for a store of another, and the root of a set is its smallest vertex.
//      k_cc_flatten  one thread per vertex: label[v] = its root
//      k_cc_count    one thread per face: size[label[a]] += 1, INTEGER atomics, one per distinct label of a wave (faces come in
//                    cell order: mostly one).  It needs the final labels, hence a launch of its own.
// 2. Selection and compaction.  c_k = the k-th largest face count from the library's radix sort of `size` (the zeros of the
//    non-label rows sort first and change nothing: T >= 1), T = max(c_k, m), keep flags per vertex and per face from
//    size[label[.]] >= T — a vertex of a kept component always has a kept face, and an unreferenced vertex has size 0 — two
//    gcp_exclusive_scan_i32, one host read of (status, V', F'), ranked writes.
// 3. Vertex normals.  The 3 F corners are stably sorted by vertex id (gcp_sort_pairs_u32; corners of a face with a bad index get
//    the key V and sort behind every vertex), the run of vertex v starts where the sorted key first reaches v, and one thread
//    per vertex sums (b - a) x (c - a) of its corners' faces in ascending corner index.  No atomics.
#include <math.h>

#include "gcp_device.hpp"
#include "grouped_cumprod_hip.h"

namespace {

using gcp::align256;
using gcp::i64;

constexpr int kThreads = 256;
constexpr int64_t kMaxRows = INT32_MAX / 3;  // 3 V and 3 F are int32 offsets

inline bool sizes_ok(int64_t n_vertices, int64_t n_faces) {
  return n_vertices >= 0 && n_faces >= 0 && n_vertices <= kMaxRows && n_faces <= kMaxRows;
}
inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }
inline int bit_length(int64_t x) {
  int b = 1;
  while (b < 32 && (x >> b)) ++b;
  return b;
}

// ---- 1. components -----------------------------------------------------------------------------------------------------------

// Other blocks write `parent` during the hook launch: every access is a relaxed agent-scope atomic, never a cached copy.
__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x, halving the path on the way.  A value read here that differs from its index is final in kind: a vertex that was
// ever hooked never becomes a root again, so the store below only ever replaces one ancestor by another.
__device__ __forceinline__ int find_root(int* parent, int x) {
  for (;;) {
    const int p = ld(parent + x);
    if (p == x) return x;
    const int g = ld(parent + p);
    if (g == p) return p;
    st(parent + x, g);
    x = g;
  }
}

__device__ __forceinline__ void unite(int* parent, int a, int b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    a = old, b = lo;  // hi had been hooked meanwhile: old < hi is of its set
  }
}

__device__ __forceinline__ bool face_ok(int a, int b, int c, int n_vertices) {
  return (unsigned)a < (unsigned)n_vertices && (unsigned)b < (unsigned)n_vertices && (unsigned)c < (unsigned)n_vertices;
}

__global__ __launch_bounds__(kThreads) void k_cc_init(int n_vertices, int* __restrict__ label, int* __restrict__ size, int* __restrict__ status) {
  const i64 v = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (v == 0) *status = 0;
  if (v >= n_vertices) return;
  label[v] = (int)v;
  size[v] = 0;
}

__global__ __launch_bounds__(kThreads) void k_cc_hook(const int* __restrict__ faces, int n_faces, int n_vertices, int* parent, int* status) {
  const i64 f = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (f >= n_faces) return;
  const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  if (!face_ok(a, b, c, n_vertices)) {  // before any access through them
    atomicOr(status, 1);
    return;
  }
  if (b != a) unite(parent, a, b);
  if (c != a && c != b) unite(parent, a, c);
}

__global__ __launch_bounds__(kThreads) void k_cc_flatten(int n_vertices, int* label) {
  const i64 v = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (v >= n_vertices) return;
  int x = (int)v;
  for (;;) {  // other threads store roots into label meanwhile: any value read is an ancestor
    const int p = ld(label + x);
    if (p == x) break;
    x = p;
  }
  st(label + v, x);
}

__global__ __launch_bounds__(kThreads) void k_cc_count(const int* __restrict__ faces, int n_faces, int n_vertices, const int* __restrict__ label,
                                                       int* size) {
  const i64 f = (i64)blockIdx.x * kThreads + threadIdx.x;
  int root = -1;
  if (f < n_faces) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (face_ok(a, b, c, n_vertices)) root = label[a];
  }
  const int lane = (int)(threadIdx.x & 63);
  unsigned long long todo = __ballot(root >= 0);
  while (todo) {  // one round per distinct label of the wave
    const int first = __ffsll((long long)todo) - 1;
    const int lead = __shfl(root, first);
    const unsigned long long same = __ballot(root == lead);
    if (lane == first) atomicAdd(size + lead, (int)__popcll(same));
    todo &= ~same;
  }
}

int launch_components(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* label, int32_t* size, int32_t* status,
                      hipStream_t stream) {
  hipLaunchKernelGGL(k_cc_init, dim3(blocks_for(n_vertices)), dim3(kThreads), 0, stream, (int)n_vertices, label, size, status);
  GCP_HIP(hipGetLastError());
  if (n_faces == 0) return GCP_OK;
  hipLaunchKernelGGL(k_cc_hook, dim3(blocks_for(n_faces)), dim3(kThreads), 0, stream, faces, (int)n_faces, (int)n_vertices, label, status);
  GCP_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_cc_flatten, dim3(blocks_for(n_vertices)), dim3(kThreads), 0, stream, (int)n_vertices, label);
  GCP_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_cc_count, dim3(blocks_for(n_faces)), dim3(kThreads), 0, stream, faces, (int)n_faces, (int)n_vertices,
                     (const int*)label, size);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

// ---- 2. selection and compaction ---------------------------------------------------------------------------------------------

struct CleanWorkspace {
  int* words;      // [0] status, [1] V', [2] F'
  int* label;      // [V]
  int* size;       // [V]
  unsigned* sorted_size;  // [V] ascending
  int* sorted_at;  // [V] the sort's permutation (not used)
  int* vert_keep;  // [V]
  int* vert_off;   // [V + 1]
  int* face_keep;  // [F]
  int* face_off;   // [F + 1]
  char* sort;
  char* scan;
};

inline size_t carve_clean(char* base, int64_t n_vertices, int64_t n_faces, CleanWorkspace* w) {
  char* p = base;
  CleanWorkspace l;
  const size_t nv = (size_t)n_vertices, nf = (size_t)n_faces;
  l.words = gcp::carve<int>(p, 4);
  l.label = gcp::carve<int>(p, nv);
  l.size = gcp::carve<int>(p, nv);
  l.sorted_size = gcp::carve<unsigned>(p, nv);
  l.sorted_at = gcp::carve<int>(p, nv);
  l.vert_keep = gcp::carve<int>(p, nv);
  l.vert_off = gcp::carve<int>(p, nv + 1);
  l.face_keep = gcp::carve<int>(p, nf);
  l.face_off = gcp::carve<int>(p, nf + 1);
  l.sort = p;
  p += align256(gcp_sort_workspace_bytes(n_vertices));
  l.scan = p;
  p += align256(gcp_scan_i32_workspace_bytes(n_vertices > n_faces ? n_vertices : n_faces));
  if (w) *w = l;
  return (size_t)(p - base);
}

__global__ __launch_bounds__(kThreads) void k_keep_flags(const int* __restrict__ faces, int n_faces, int n_vertices, const int* __restrict__ label,
                                                         const int* __restrict__ size, const unsigned* __restrict__ sorted_size, int kth_at,
                                                         int min_faces, int* __restrict__ vert_keep, int* __restrict__ face_keep) {
  const i64 i = (i64)blockIdx.x * kThreads + threadIdx.x;
  const int ck = (int)sorted_size[kth_at];  // wave-uniform
  const int threshold = ck > min_faces ? ck : min_faces;
  if (i < n_vertices) vert_keep[i] = size[label[i]] >= threshold ? 1 : 0;
  if (i < n_faces) {
    const int a = faces[3 * i], b = faces[3 * i + 1], c = faces[3 * i + 2];
    face_keep[i] = (face_ok(a, b, c, n_vertices) && size[label[a]] >= threshold) ? 1 : 0;
  }
}

__global__ void k_clean_totals(const int* __restrict__ vert_off, const int* __restrict__ face_off, int n_vertices, int n_faces, int* __restrict__ words) {
  if (threadIdx.x == 0 && blockIdx.x == 0) words[1] = vert_off[n_vertices], words[2] = face_off[n_faces];
}

// One thread per float of the vertex rows: coalesced reads, runs of kept rows are coalesced writes.  Bit copies.
__global__ __launch_bounds__(kThreads) void k_compact_rows(int n_words, const int* __restrict__ vert_keep, const int* __restrict__ vert_off,
                                                           int n_kept, const unsigned* __restrict__ v_in, const unsigned* __restrict__ c_in,
                                                           const unsigned* __restrict__ n_in, unsigned* __restrict__ v_out,
                                                           unsigned* __restrict__ c_out, unsigned* __restrict__ n_out) {
  const i64 e = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (e >= n_words) return;
  const int v = (int)(e / 3);
  if (!vert_keep[v]) return;
  const int row = vert_off[v];
  if (row >= n_kept) return;  // a caller's count smaller than select's: nothing is written past the outputs
  const i64 o = 3 * (i64)row + (e - 3 * (i64)v);
  v_out[o] = v_in[e];
  if (c_out) c_out[o] = c_in[e];
  if (n_out) n_out[o] = n_in[e];
}

__global__ __launch_bounds__(kThreads) void k_compact_faces(const int* __restrict__ faces, int n_faces, const int* __restrict__ face_keep,
                                                            const int* __restrict__ face_off, const int* __restrict__ vert_off, int n_kept,
                                                            int* __restrict__ out) {
  const i64 f = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (f >= n_faces) return;
  if (!face_keep[f]) return;  // kept: its three indices were found in range
  const int row = face_off[f];
  if (row >= n_kept) return;
#pragma unroll
  for (int j = 0; j < 3; ++j) out[3 * (i64)row + j] = vert_off[faces[3 * f + j]];
}

// ---- 3. vertex normals -------------------------------------------------------------------------------------------------------

struct NormalWorkspace {
  unsigned* key;         // [3 F] the vertex a corner names, V for the corners of a face with a bad index
  unsigned* sorted_key;  // [3 F]
  int* corner;           // [3 F] corner indices 3 f + j by (vertex, corner)
  int* start;            // [V + 1] first sorted position with key >= v
  char* sort;
};

inline size_t carve_normals(char* base, int64_t n_vertices, int64_t n_faces, NormalWorkspace* w) {
  char* p = base;
  NormalWorkspace l;
  const size_t nc = 3 * (size_t)n_faces;
  l.key = gcp::carve<unsigned>(p, nc);
  l.sorted_key = gcp::carve<unsigned>(p, nc);
  l.corner = gcp::carve<int>(p, nc);
  l.start = gcp::carve<int>(p, (size_t)n_vertices + 1);
  l.sort = p;
  p += align256(gcp_sort_workspace_bytes(3 * n_faces));
  if (w) *w = l;
  return (size_t)(p - base);
}

__global__ __launch_bounds__(kThreads) void k_corner_keys(const int* __restrict__ faces, int n_faces, int n_vertices, unsigned* __restrict__ key) {
  const i64 f = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (f >= n_faces) return;
  const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  const bool ok = face_ok(a, b, c, n_vertices);
  key[3 * f] = ok ? (unsigned)a : (unsigned)n_vertices;
  key[3 * f + 1] = ok ? (unsigned)b : (unsigned)n_vertices;
  key[3 * f + 2] = ok ? (unsigned)c : (unsigned)n_vertices;
}

// Position i in 0 .. 3 F: every vertex id in (key[i - 1], key[i]] starts at i (key[-1] = -1, key[3 F] = V).  Each start[v] has one
// writer; the loop runs once where vertex ids are consecutive and further only over unreferenced vertices.
__global__ __launch_bounds__(kThreads) void k_run_starts(const unsigned* __restrict__ sorted_key, int n_corners, int n_vertices, int* __restrict__ start) {
  const i64 i = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (i > n_corners) return;
  const int prev = i > 0 ? (int)sorted_key[i - 1] : -1;
  const int cur = i < n_corners ? (int)sorted_key[i] : n_vertices;
  for (int v = prev + 1; v <= cur; ++v) start[v] = (int)i;
}

__global__ __launch_bounds__(kThreads) void k_vertex_normals(const float* __restrict__ vertices, const int* __restrict__ faces, int n_vertices,
                                                             const int* __restrict__ corner, const int* __restrict__ start,
                                                             float* __restrict__ normals) {
  const i64 v = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (v >= n_vertices) return;
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  const int end = start[v + 1];
  for (int i = start[v]; i < end; ++i) {  // ascending corner index: the sort is stable
    const i64 f = corner[i] / 3;
    const i64 a = 3 * (i64)faces[3 * f], b = 3 * (i64)faces[3 * f + 1], c = 3 * (i64)faces[3 * f + 2];  // in range: the key was < V
    const float ax = vertices[a], ay = vertices[a + 1], az = vertices[a + 2];
    const float ux = vertices[b] - ax, uy = vertices[b + 1] - ay, uz = vertices[b + 2] - az;
    const float wx = vertices[c] - ax, wy = vertices[c + 1] - ay, wz = vertices[c + 2] - az;
    sx += uy * wz - uz * wy;
    sy += uz * wx - ux * wz;
    sz += ux * wy - uy * wx;
  }
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  const float m = fmaxf(fmaxf(fabsf(sx), fabsf(sy)), fabsf(sz));
  if (isfinite(sx) && isfinite(sy) && isfinite(sz) && m > 0.0f) {
    const int e = ilogbf(m);  // scaled by a power of two, exactly: the squares neither overflow nor vanish
    sx = scalbnf(sx, -e), sy = scalbnf(sy, -e), sz = scalbnf(sz, -e);
    const float len = sqrtf((sx * sx + sy * sy) + sz * sz);
    nx = sx / len, ny = sy / len, nz = sz / len;
  }
  normals[3 * v] = nx, normals[3 * v + 1] = ny, normals[3 * v + 2] = nz;
}

}  // namespace

extern "C" {

size_t gcp_mesh_components_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
  if (!sizes_ok(n_vertices, n_faces)) return 0;
  return 256;  // the status word of a call that passes no status_dev
}

int gcp_mesh_components(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* label, int32_t* size, int32_t* status_dev,
                        void* ws, size_t ws_bytes, void* stream) {
  if (!sizes_ok(n_vertices, n_faces)) return GCP_ERR_INVALID_ARGUMENT;
  if (n_vertices == 0) return GCP_OK;  // no output row; faces, if any, name no vertex and are ignored
  if (!label || !size || !ws || (n_faces > 0 && !faces)) return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < gcp_mesh_components_workspace_bytes(n_vertices, n_faces) || ((uintptr_t)ws & 255)) return GCP_ERR_WORKSPACE;
  return launch_components(faces, n_faces, n_vertices, label, size, status_dev ? status_dev : (int32_t*)ws, (hipStream_t)stream);
}

size_t gcp_mesh_clean_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
  if (!sizes_ok(n_vertices, n_faces)) return 0;
  return carve_clean(nullptr, n_vertices, n_faces, nullptr);
}

int gcp_mesh_select(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int64_t keep_largest, int64_t min_faces, void* ws,
                    size_t ws_bytes, int64_t* totals_host, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!sizes_ok(n_vertices, n_faces) || keep_largest < 1 || min_faces < 1 || !totals_host) return GCP_ERR_INVALID_ARGUMENT;
  totals_host[0] = totals_host[1] = 0;
  if (n_vertices == 0 || n_faces == 0) return GCP_OK;  // nothing is kept: nothing is launched
  if (!faces || !ws) return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < gcp_mesh_clean_workspace_bytes(n_vertices, n_faces) || ((uintptr_t)ws & 255)) return GCP_ERR_WORKSPACE;
  CleanWorkspace w;
  carve_clean((char*)ws, n_vertices, n_faces, &w);
  int st = launch_components(faces, n_faces, n_vertices, w.label, w.size, w.words, stream);
  if (st != GCP_OK) return st;
  // a face count is at most F: that many key bits; the k-th largest sits k from the end, the smallest count when there are fewer
  st = gcp_sort_pairs_u32((const uint32_t*)w.size, n_vertices, bit_length(n_faces), w.sorted_size, w.sorted_at, w.sort,
                          gcp_sort_workspace_bytes(n_vertices), stream_);
  if (st != GCP_OK) return st;
  const int kth_at = keep_largest <= n_vertices ? (int)(n_vertices - keep_largest) : 0;
  const int m = min_faces > INT32_MAX ? INT32_MAX : (int)min_faces;
  const int64_t n = n_vertices > n_faces ? n_vertices : n_faces;
  hipLaunchKernelGGL(k_keep_flags, dim3(blocks_for(n)), dim3(kThreads), 0, stream, faces, (int)n_faces, (int)n_vertices, (const int*)w.label,
                     (const int*)w.size, (const unsigned*)w.sorted_size, kth_at, m, w.vert_keep, w.face_keep);
  GCP_HIP(hipGetLastError());
  const size_t scan_bytes = gcp_scan_i32_workspace_bytes(n);
  st = gcp_exclusive_scan_i32(w.vert_keep, w.vert_off, n_vertices, w.scan, scan_bytes, stream_);
  if (st != GCP_OK) return st;
  st = gcp_exclusive_scan_i32(w.face_keep, w.face_off, n_faces, w.scan, scan_bytes, stream_);
  if (st != GCP_OK) return st;
  hipLaunchKernelGGL(k_clean_totals, dim3(1), dim3(64), 0, stream, (const int*)w.vert_off, (const int*)w.face_off, (int)n_vertices,
                     (int)n_faces, w.words);
  GCP_HIP(hipGetLastError());
  int words[3] = {0, 0, 0};
  GCP_HIP(hipMemcpyAsync(words, w.words, sizeof(words), hipMemcpyDeviceToHost, stream));  // the one read
  GCP_HIP(hipStreamSynchronize(stream));
  if (words[0] != 0) return GCP_ERR_INVALID_ARGUMENT;  // a face index outside [0, V): skipped by every kernel, reported here
  totals_host[0] = words[1];
  totals_host[1] = words[2];
  return GCP_OK;
}

int gcp_mesh_compact(const int32_t* faces, int64_t n_faces, int64_t n_vertices, const float* vertices, const float* colours,
                     const float* normals, const void* ws, size_t ws_bytes, int64_t n_vertices_out, int64_t n_faces_out, float* vertices_out,
                     int32_t* faces_out, float* colours_out, float* normals_out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!sizes_ok(n_vertices, n_faces) || n_vertices_out < 0 || n_faces_out < 0 || n_vertices_out > n_vertices || n_faces_out > n_faces)
    return GCP_ERR_INVALID_ARGUMENT;
  if ((colours_out && !colours) || (normals_out && !normals)) return GCP_ERR_INVALID_ARGUMENT;
  if (n_vertices_out == 0 && n_faces_out == 0) return GCP_OK;
  if (!ws || !faces || (n_vertices_out > 0 && (!vertices || !vertices_out)) || (n_faces_out > 0 && !faces_out)) return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < gcp_mesh_clean_workspace_bytes(n_vertices, n_faces) || ((uintptr_t)ws & 255)) return GCP_ERR_WORKSPACE;
  CleanWorkspace w;
  carve_clean((char*)ws, n_vertices, n_faces, &w);
  if (n_vertices_out > 0) {
    hipLaunchKernelGGL(k_compact_rows, dim3(blocks_for(3 * n_vertices)), dim3(kThreads), 0, stream, (int)(3 * n_vertices),
                       (const int*)w.vert_keep, (const int*)w.vert_off, (int)n_vertices_out, (const unsigned*)vertices, (const unsigned*)colours,
                       (const unsigned*)normals, (unsigned*)vertices_out, (unsigned*)colours_out, (unsigned*)normals_out);
    GCP_HIP(hipGetLastError());
  }
  if (n_faces_out > 0) {
    hipLaunchKernelGGL(k_compact_faces, dim3(blocks_for(n_faces)), dim3(kThreads), 0, stream, faces, (int)n_faces, (const int*)w.face_keep,
                       (const int*)w.face_off, (const int*)w.vert_off, (int)n_faces_out, faces_out);
    GCP_HIP(hipGetLastError());
  }
  return GCP_OK;
}

size_t gcp_mesh_vertex_normals_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
  if (!sizes_ok(n_vertices, n_faces)) return 0;
  return carve_normals(nullptr, n_vertices, n_faces, nullptr);
}

int gcp_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float* normals, void* ws,
                            size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!sizes_ok(n_vertices, n_faces)) return GCP_ERR_INVALID_ARGUMENT;
  if (n_vertices == 0) return GCP_OK;
  if (!vertices || !normals || (n_faces > 0 && (!faces || !ws))) return GCP_ERR_INVALID_ARGUMENT;
  if (n_faces == 0) {  // no face: every sum is empty
    GCP_HIP(hipMemsetAsync(normals, 0, 3 * (size_t)n_vertices * sizeof(float), stream));
    return GCP_OK;
  }
  if (ws_bytes < gcp_mesh_vertex_normals_workspace_bytes(n_vertices, n_faces) || ((uintptr_t)ws & 255)) return GCP_ERR_WORKSPACE;
  NormalWorkspace w;
  carve_normals((char*)ws, n_vertices, n_faces, &w);
  const int64_t n_corners = 3 * n_faces;
  hipLaunchKernelGGL(k_corner_keys, dim3(blocks_for(n_faces)), dim3(kThreads), 0, stream, faces, (int)n_faces, (int)n_vertices, w.key);
  GCP_HIP(hipGetLastError());
  const int st = gcp_sort_pairs_u32(w.key, n_corners, bit_length(n_vertices), w.sorted_key, w.corner, w.sort, gcp_sort_workspace_bytes(n_corners),
                                    stream_);
  if (st != GCP_OK) return st;
  hipLaunchKernelGGL(k_run_starts, dim3(blocks_for(n_corners + 1)), dim3(kThreads), 0, stream, (const unsigned*)w.sorted_key, (int)n_corners,
                     (int)n_vertices, w.start);
  GCP_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_vertex_normals, dim3(blocks_for(n_vertices)), dim3(kThreads), 0, stream, vertices, faces, (int)n_vertices,
                     (const int*)w.corner, (const int*)w.start, normals);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

}  // extern "C"
