// gcp_tsdf.hip — a triangle mesh out of rendered depth maps: TSDF fusion, then marching tetrahedra.
//
// The volume: nz x ny x nx lattice points, x fastest; point (i, j, k) sits at origin + voxel (i, j, k).  A point's flat index
// is p = (k ny + j) nx + i < 2^31.
//
// 1. Integration (k_tsdf_integrate): Open3D's projective z-depth TSDF with nearest-pixel lookup and unit weights.  One thread
//    per lattice point, flat over the volume, so a wave's 64 lanes load and store 256 contiguous bytes of every state plane.
//    The point's state (tsdf, weight, rgb) is loaded once, stays in registers over the loop over the B cameras of the launch
//    and is stored once: 8 B read + 8 B written per point (20 + 20 with colour), whatever B.  P and K are read through
//    addresses that depend on the loop counter alone: scalar loads, scalar registers.  The maps are gathered — neighbouring
//    points project to neighbouring pixels.  Cameras are visited in order and the state is float32 in registers exactly as in
//    memory, so B cameras in one launch, one at a time or in any split give the same bits.  No atomics, no workspace, no
//    device->host read (capturable).  The pixel test is made in float BEFORE the conversion to int: z -> 0+ makes u huge.
//
// 2. Extraction: marching tetrahedra on the Kuhn decomposition — every cell is cut into the 6 tetrahedra
//    {c, c + e_a, c + e_a + e_b, c + (1,1,1)}, one per permutation (a, b, c) of the axes, in the order (x,y,z), (x,z,y),
//    (y,x,z), (y,z,x), (z,x,y), (z,y,x).  All share the body diagonal; the face diagonals are translates of each other, so
//    neighbouring cells agree and the surface is watertight by construction.  No case table: the 16 cases are the popcount of
//    the 4 inside bits, and the winding comes from the sign of a 3 x 3 integer determinant of corner offsets (below).
//    Vertices live on lattice edges of 7 kinds seen from their lower end point (+x, +y, +z, +xy, +xz, +yz, +xyz: kind 0..6),
//    which owns them.  Passes, each one thread per lattice point:
//      k_mesh_cells   the cell whose lowest corner the point is: valid (all 8 corners have weight > 0), its triangle count
//      k_mesh_edges   the point's 7 owned edges: a 7-bit mask of those that carry a vertex (end points differ in side, both in
//                     the grid, at least one valid cell contains the edge), its popcount
//      two gcp_exclusive_scan_i32, the two 64-bit totals read by the host (the one read; extraction is not capturable)
//      k_mesh_vertices / k_mesh_faces   ranked writes: vertex id = offset[owner] + popcount(mask below the kind)
//    Vertices come out by (owner, kind), faces by (cell, tetrahedron, triangle): the same bits on every run.
#include <math.h>

#include "gcp_device.hpp"
#include "grouped_cumprod_hip.h"

namespace {

using gcp::align256;
using gcp::i64;

constexpr int kThreads = 256;

inline bool dims_ok(int32_t nx, int32_t ny, int32_t nz) {
  return nx >= 2 && ny >= 2 && nz >= 2 && (int64_t)nx * ny * nz <= INT32_MAX;
}

// ---- 1. integration ----------------------------------------------------------------------------------------------------------

template <bool COLOUR>
__global__ __launch_bounds__(kThreads) void k_tsdf_integrate(float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ rgb,
                                                             int nx, int ny, int n, float ox, float oy, float oz, float voxel, float trunc,
                                                             const float* __restrict__ depth, const float* __restrict__ alpha,
                                                             const float* __restrict__ image, const float* __restrict__ P,
                                                             const float* __restrict__ K, int cameras, int height, int width,
                                                             float alpha_min, float depth_max) {
  const i64 p64 = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (p64 >= n) return;
  const int p = (int)p64;
  const int i = p % nx, j = (p / nx) % ny, k = p / (nx * ny);
  const float xw = ox + voxel * (float)i, yw = oy + voxel * (float)j, zw = oz + voxel * (float)k;
  float f = tsdf[p], w = weight[p];
  float c0 = 0.f, c1 = 0.f, c2 = 0.f;
  if (COLOUR) c0 = rgb[p], c1 = rgb[(i64)n + p], c2 = rgb[2 * (i64)n + p];
  const i64 plane = (i64)height * width;
  const float fw = (float)width, fh = (float)height;
  for (int c = 0; c < cameras; ++c) {
    const float* __restrict__ Pc = P + 12 * (i64)c;  // wave-uniform: scalar loads
    const float* __restrict__ Kc = K + 9 * (i64)c;
    const float z = ((Pc[8] * xw + Pc[9] * yw) + Pc[10] * zw) + Pc[11];
    if (!(z > 0.0f)) continue;
    const float px = ((Pc[0] * xw + Pc[1] * yw) + Pc[2] * zw) + Pc[3];
    const float py = ((Pc[4] * xw + Pc[5] * yw) + Pc[6] * zw) + Pc[7];
    const float u = Kc[0] * px / z + Kc[2], v = Kc[4] * py / z + Kc[5];
    if (!(u >= 0.0f && u < fw && v >= 0.0f && v < fh)) continue;  // in float, NaN included, before any conversion
    const int x = (int)u, y = (int)v;                              // floor: both are >= 0
    const i64 o = (i64)c * plane + (i64)y * width + x;
    const float a = alpha[o], D = depth[o];
    if (!(a >= alpha_min && D > 0.0f)) continue;
    const float d = D / a;
    if (depth_max > 0.0f && d > depth_max) continue;
    const float s = d - z;
    if (s < -trunc) continue;
    const float tau = fminf(1.0f, s / trunc);
    const float w1 = w + 1.0f;
    f = (f * w + tau) / w1;
    if (COLOUR) {
      const i64 o3 = 3 * (i64)c * plane + (i64)y * width + x;
      c0 = (c0 * w + image[o3]) / w1;
      c1 = (c1 * w + image[o3 + plane]) / w1;
      c2 = (c2 * w + image[o3 + 2 * plane]) / w1;
    }
    w = w1;
  }
  tsdf[p] = f;
  weight[p] = w;
  if (COLOUR) rgb[p] = c0, rgb[(i64)n + p] = c1, rgb[2 * (i64)n + p] = c2;
}

// ---- 2. marching tetrahedra --------------------------------------------------------------------------------------------------

// A corner of a cell is named by its offset bits dx | dy << 1 | dz << 2.  Edge kinds by the offset between the end points:
// +x +y +z +xy +xz +yz +xyz = 0..6.
__device__ __forceinline__ int kind_of(int dbits) { return (0x65423100 >> (4 * dbits)) & 7; }  // 1,2,3,4,5,6,7 -> 0,1,3,2,4,5,6
__device__ __forceinline__ int bits_of(int kind) { return (0x7653421 >> (4 * kind)) & 7; }     // 0..6 -> 1,2,4,3,5,6,7

// The axes (a, b) of tetrahedron t: corners 0, 1 << a, 1 << a | 1 << b, 7.
__device__ __forceinline__ void tet_corners(int t, int cn[4]) {
  const int a = t >> 1, b = (0x102021 >> (4 * t)) & 3;  // (0,1) (0,2) (1,0) (1,2) (2,0) (2,1)
  cn[0] = 0, cn[1] = 1 << a, cn[2] = (1 << a) | (1 << b), cn[3] = 7;
}

// Signed components of corner q minus corner p.
__device__ __forceinline__ void diff(int q, int p, int d[3]) {
  d[0] = (q & 1) - (p & 1), d[1] = ((q >> 1) & 1) - ((p >> 1) & 1), d[2] = ((q >> 2) & 1) - ((p >> 2) & 1);
}
__device__ __forceinline__ int det(int p, int q0, int q1, int q2) {  // det [q0 - p, q1 - p, q2 - p]
  int a[3], b[3], c[3];
  diff(q0, p, a), diff(q1, p, b), diff(q2, p, c);
  return a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// The position of the n-th (from 0) set bit of a 4-bit mask.
__device__ __forceinline__ int nth_set(int m, int n) {
  int seen = 0, at = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int bit = (m >> s) & 1;
    if (bit && seen == n) at = s;
    seen += bit;
  }
  return at;
}

struct Workspace {
  unsigned long long* totals;  // [2]: vertices, triangles
  unsigned char* valid;        // [n] the cell whose lowest corner is the point
  unsigned char* mask;         // [n] the owned edges that carry a vertex
  int* vert_cnt;               // [n]
  int* vert_off;               // [n + 1]
  int* tri_cnt;                // [n]
  int* tri_off;                // [n + 1]
  char* scan;
};

inline size_t carve_workspace(char* base, int64_t n, Workspace* w) {
  char* p = base;
  Workspace l;
  l.totals = gcp::carve<unsigned long long>(p, 2);
  l.valid = gcp::carve<unsigned char>(p, (size_t)n);
  l.mask = gcp::carve<unsigned char>(p, (size_t)n);
  l.vert_cnt = gcp::carve<int>(p, (size_t)n);
  l.vert_off = gcp::carve<int>(p, (size_t)n + 1);
  l.tri_cnt = gcp::carve<int>(p, (size_t)n);
  l.tri_off = gcp::carve<int>(p, (size_t)n + 1);
  l.scan = p;
  p += align256(gcp_scan_i32_workspace_bytes(n));
  if (w) *w = l;
  return (size_t)(p - base);
}

__global__ __launch_bounds__(kThreads) void k_mesh_cells(const float* __restrict__ f, const float* __restrict__ weight, int nx, int ny,
                                                         int nz, int n, float iso, unsigned char* __restrict__ valid,
                                                         int* __restrict__ tri_cnt, unsigned long long* __restrict__ totals) {
  const i64 p64 = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (p64 >= n) return;
  const int p = (int)p64;
  const int i = p % nx, j = (p / nx) % ny, k = p / (nx * ny);
  int ok = 0, count = 0;
  if (i < nx - 1 && j < ny - 1 && k < nz - 1) {
    ok = 1;
    int inside = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const i64 q = (i64)p + (c & 1) + (i64)((c >> 1) & 1) * nx + (i64)((c >> 2) & 1) * nx * ny;
      if (weight && !(weight[q] > 0.0f)) ok = 0;
      inside |= (f[q] < iso ? 1 : 0) << c;
    }
    if (ok) {
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        int cn[4];
        tet_corners(t, cn);
        const int m = ((inside >> cn[0]) & 1) + ((inside >> cn[1]) & 1) + ((inside >> cn[2]) & 1) + ((inside >> cn[3]) & 1);
        count += (m == 2) ? 2 : ((m == 1 || m == 3) ? 1 : 0);
      }
    }
  }
  valid[p] = (unsigned char)ok;
  tri_cnt[p] = count;
  if (count) atomicAdd(&totals[1], (unsigned long long)count);  // an integer sum: the same whatever the order
}

__global__ __launch_bounds__(kThreads) void k_mesh_edges(const float* __restrict__ f, const unsigned char* __restrict__ valid, int nx, int ny,
                                                         int nz, int n, float iso, unsigned char* __restrict__ mask,
                                                         int* __restrict__ vert_cnt, unsigned long long* __restrict__ totals) {
  const i64 p64 = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (p64 >= n) return;
  const int p = (int)p64;
  const int i = p % nx, j = (p / nx) % ny, k = p / (nx * ny);
  const bool in_p = f[p] < iso;
  const i64 sy = nx, sz = (i64)nx * ny;
  int m = 0;
#pragma unroll
  for (int kind = 0; kind < 7; ++kind) {
    const int d = bits_of(kind), dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
    if (i + dx >= nx || j + dy >= ny || k + dz >= nz) continue;
    const i64 q = (i64)p + dx + dy * sy + dz * sz;
    if ((f[q] < iso) == in_p) continue;
    // the cells that contain the edge: the lowest corner steps back along every axis the edge does not move along
    bool any = false;
    for (int bz = 0; bz <= 1 - dz; ++bz)
      for (int by = 0; by <= 1 - dy; ++by)
        for (int bx = 0; bx <= 1 - dx; ++bx)
          if (i - bx >= 0 && j - by >= 0 && k - bz >= 0 && valid[(i64)p - bx - by * sy - bz * sz]) any = true;  // 0 past the last cell
    if (any) m |= 1 << kind;
  }
  const int count = __builtin_popcount(m);
  mask[p] = (unsigned char)m;
  vert_cnt[p] = count;
  if (count) atomicAdd(&totals[0], (unsigned long long)count);
}

__global__ __launch_bounds__(kThreads) void k_mesh_vertices(const float* __restrict__ f, const float* __restrict__ rgb, int nx, int ny, int n,
                                                            float ox, float oy, float oz, float voxel, float iso,
                                                            const unsigned char* __restrict__ mask, const int* __restrict__ vert_off,
                                                            float* __restrict__ vertices, float* __restrict__ colours) {
  const i64 p64 = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (p64 >= n) return;
  const int p = (int)p64;
  const int m = mask[p];
  if (!m) return;
  const int i = p % nx, j = (p / nx) % ny, k = p / (nx * ny);
  const float fp = f[p];
  const float xp[3] = {ox + voxel * (float)i, oy + voxel * (float)j, oz + voxel * (float)k};
  i64 at = vert_off[p];
  for (int kind = 0; kind < 7; ++kind) {
    if (!((m >> kind) & 1)) continue;
    const int d = bits_of(kind), dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
    const i64 q = (i64)p + dx + (i64)dy * nx + (i64)dz * nx * ny;
    const float t = (iso - fp) / (f[q] - fp);
    const float xq[3] = {ox + voxel * (float)(i + dx), oy + voxel * (float)(j + dy), oz + voxel * (float)(k + dz)};
#pragma unroll
    for (int a = 0; a < 3; ++a) vertices[3 * at + a] = xp[a] + t * (xq[a] - xp[a]);
    if (colours) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float cp = rgb[(i64)a * n + p], cq = rgb[(i64)a * n + q];
        colours[3 * at + a] = cp + t * (cq - cp);
      }
    }
    ++at;
  }
}

// The id of the vertex on the edge between corners lo and hi of the cell at p (lo's bits are a subset of hi's: lo owns it).
__device__ __forceinline__ int vertex_id(i64 p, int lo, int hi, int nx, i64 sz, const unsigned char* __restrict__ mask,
                                         const int* __restrict__ vert_off) {
  const i64 owner = p + (lo & 1) + (i64)((lo >> 1) & 1) * nx + (i64)((lo >> 2) & 1) * sz;
  const int kind = kind_of(hi ^ lo);
  return vert_off[owner] + __builtin_popcount(mask[owner] & ((1 << kind) - 1));
}

// Triangles of one tetrahedron, wound counter-clockwise seen from the side f grows towards.  With a the lone corner of its
// side and q0, q1, q2 the others, the cut triangle keeps, for every position of its vertices on the open edges, the
// orientation of (q0, q1, q2): its normal points away from a when det [q0 - a, q1 - a, q2 - a] > 0.  With two corners a, b
// inside and o0, o1 outside, the quadrilateral (a o0, a o1, b o1, b o0) is planar and its normal is (o1 - o0) x (b - a) up to a
// positive factor, which points from a towards o0 when det [o0 - a, o1 - a, b - a] > 0.
__global__ __launch_bounds__(kThreads) void k_mesh_faces(const float* __restrict__ f, int nx, int ny, int n, float iso,
                                                         const unsigned char* __restrict__ mask, const int* __restrict__ vert_off,
                                                         const int* __restrict__ tri_cnt, const int* __restrict__ tri_off,
                                                         int* __restrict__ faces) {
  const i64 p64 = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (p64 >= n) return;
  const i64 p = p64;
  if (!tri_cnt[p]) return;  // not a cell, not valid, or not cut
  const i64 sz = (i64)nx * ny;
  int inside = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) inside |= (f[p + (c & 1) + (i64)((c >> 1) & 1) * nx + (i64)((c >> 2) & 1) * sz] < iso ? 1 : 0) << c;
  i64 at = tri_off[p];
  for (int t = 0; t < 6; ++t) {
    int cn[4];
    tet_corners(t, cn);
    const int chain = cn[0] | (cn[1] << 3) | (cn[2] << 6) | (cn[3] << 9);  // corner of chain position s: bits 3 s .. 3 s + 2
    int im = 0;                                                             // inside bits by chain position
#pragma unroll
    for (int s = 0; s < 4; ++s) im |= ((inside >> cn[s]) & 1) << s;
    const int n_in = __builtin_popcount(im);
    if (n_in == 0 || n_in == 4) continue;
    const int om = ~im & 15;
    auto corner = [&](int s) { return (chain >> (3 * s)) & 7; };
    auto vid = [&](int s0, int s1) {  // chain positions in any order: the lower one owns the edge
      const int lo = s0 < s1 ? s0 : s1, hi = s0 < s1 ? s1 : s0;
      return vertex_id(p, corner(lo), corner(hi), nx, sz, mask, vert_off);
    };
    if (n_in == 2) {
      const int a = nth_set(im, 0), b = nth_set(im, 1), o0 = nth_set(om, 0), o1 = nth_set(om, 1);  // ascending chain positions
      int q0 = vid(a, o0), q1 = vid(a, o1), q2 = vid(b, o1), q3 = vid(b, o0);
      if (!(det(corner(a), corner(o0), corner(o1), corner(b)) > 0)) {  // reverse the cycle, keeping q0
        const int s = q1;
        q1 = q3, q3 = s;
      }
      faces[3 * at] = q0, faces[3 * at + 1] = q1, faces[3 * at + 2] = q2;
      faces[3 * at + 3] = q0, faces[3 * at + 4] = q2, faces[3 * at + 5] = q3;
      at += 2;
    } else {
      const bool lone_in = n_in == 1;
      const int lone = lone_in ? im : om, rest = lone_in ? om : im;
      const int a = nth_set(lone, 0), o0 = nth_set(rest, 0), o1 = nth_set(rest, 1), o2 = nth_set(rest, 2);
      int q0 = vid(a, o0), q1 = vid(a, o1), q2 = vid(a, o2);
      const bool positive = det(corner(a), corner(o0), corner(o1), corner(o2)) > 0;
      if (positive != lone_in) {  // lone inside corner: the normal leaves it; lone outside corner: the normal points at it
        const int s = q1;
        q1 = q2, q2 = s;
      }
      faces[3 * at] = q0, faces[3 * at + 1] = q1, faces[3 * at + 2] = q2;
      at += 1;
    }
  }
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

extern "C" {

int gcp_tsdf_integrate(float* tsdf, float* weight, float* rgb, int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y,
                       float origin_z, float voxel, float trunc, const float* depth, const float* alpha, const float* image,
                       const float* P, const float* K, int64_t cameras, int32_t height, int32_t width, float alpha_min,
                       float depth_max, void* stream) {
  if (!dims_ok(nx, ny, nz) || !(voxel > 0.0f) || !(trunc > 0.0f) || cameras < 0 || cameras > INT32_MAX) return GCP_ERR_INVALID_ARGUMENT;
  if (!isfinite(voxel) || !isfinite(trunc) || !isfinite(origin_x) || !isfinite(origin_y) || !isfinite(origin_z)) return GCP_ERR_INVALID_ARGUMENT;
  if (cameras == 0) return GCP_OK;
  if (height < 1 || width < 1 || (int64_t)height * width > INT32_MAX) return GCP_ERR_INVALID_ARGUMENT;
  if (!tsdf || !weight || !depth || !alpha || !P || !K || (rgb && !image)) return GCP_ERR_INVALID_ARGUMENT;
  const int n = nx * ny * nz;
  if (rgb)
    hipLaunchKernelGGL(k_tsdf_integrate<true>, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, tsdf, weight, rgb, (int)nx,
                       (int)ny, n, origin_x, origin_y, origin_z, voxel, trunc, depth, alpha, image, P, K, (int)cameras, (int)height,
                       (int)width, alpha_min, depth_max);
  else
    hipLaunchKernelGGL(k_tsdf_integrate<false>, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, tsdf, weight, rgb, (int)nx,
                       (int)ny, n, origin_x, origin_y, origin_z, voxel, trunc, depth, alpha, image, P, K, (int)cameras, (int)height,
                       (int)width, alpha_min, depth_max);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

size_t gcp_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
  if (!dims_ok(nx, ny, nz)) return 0;
  return carve_workspace(nullptr, (int64_t)nx * ny * nz, nullptr);
}

int gcp_mesh_count(const float* tsdf, const float* weight, int32_t nx, int32_t ny, int32_t nz, float iso, void* ws, size_t ws_bytes,
                   int64_t* totals_host, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!dims_ok(nx, ny, nz) || !(iso == iso) || !tsdf || !ws || !totals_host) return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < gcp_mesh_workspace_bytes(nx, ny, nz) || ((uintptr_t)ws & 255)) return GCP_ERR_WORKSPACE;
  totals_host[0] = totals_host[1] = 0;
  const int n = nx * ny * nz;
  Workspace w;
  carve_workspace((char*)ws, n, &w);
  GCP_HIP(hipMemsetAsync(w.totals, 0, 2 * sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(k_mesh_cells, dim3(blocks_for(n)), dim3(kThreads), 0, stream, tsdf, weight, (int)nx, (int)ny, (int)nz, n, iso, w.valid,
                     w.tri_cnt, w.totals);
  GCP_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_mesh_edges, dim3(blocks_for(n)), dim3(kThreads), 0, stream, tsdf, (const unsigned char*)w.valid, (int)nx, (int)ny,
                     (int)nz, n, iso, w.mask, w.vert_cnt, w.totals);
  GCP_HIP(hipGetLastError());
  unsigned long long totals[2] = {0, 0};
  GCP_HIP(hipMemcpyAsync(totals, w.totals, sizeof(totals), hipMemcpyDeviceToHost, stream));
  GCP_HIP(hipStreamSynchronize(stream));
  if (totals[0] > 0x7fffffffull / 3 || totals[1] > 0x7fffffffull / 3) return GCP_ERR_INVALID_ARGUMENT;  // 3 V and 3 F are int32 offsets
  const size_t scan_bytes = gcp_scan_i32_workspace_bytes(n);
  int st = gcp_exclusive_scan_i32(w.vert_cnt, w.vert_off, n, w.scan, scan_bytes, stream_);
  if (st != GCP_OK) return st;
  st = gcp_exclusive_scan_i32(w.tri_cnt, w.tri_off, n, w.scan, scan_bytes, stream_);
  if (st != GCP_OK) return st;
  totals_host[0] = (int64_t)totals[0];
  totals_host[1] = (int64_t)totals[1];
  return GCP_OK;
}

int gcp_mesh_write(const float* tsdf, const float* rgb, int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z,
                   float voxel, float iso, const void* ws, size_t ws_bytes, int64_t n_vertices, int64_t n_faces, float* vertices,
                   int32_t* faces, float* colours, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!dims_ok(nx, ny, nz) || !(voxel > 0.0f) || !(iso == iso) || n_vertices < 0 || n_faces < 0 || n_vertices > INT32_MAX / 3 ||
      n_faces > INT32_MAX / 3 || !tsdf || !ws)
    return GCP_ERR_INVALID_ARGUMENT;
  if ((n_vertices > 0 && !vertices) || (n_faces > 0 && !faces) || (colours && !rgb)) return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < gcp_mesh_workspace_bytes(nx, ny, nz) || ((uintptr_t)ws & 255)) return GCP_ERR_WORKSPACE;
  const int n = nx * ny * nz;
  Workspace w;
  carve_workspace((char*)ws, n, &w);
  if (n_vertices > 0) {
    hipLaunchKernelGGL(k_mesh_vertices, dim3(blocks_for(n)), dim3(kThreads), 0, stream, tsdf, rgb, (int)nx, (int)ny, n, origin_x, origin_y,
                       origin_z, voxel, iso, (const unsigned char*)w.mask, (const int*)w.vert_off, vertices, colours);
    GCP_HIP(hipGetLastError());
  }
  if (n_faces > 0) {
    hipLaunchKernelGGL(k_mesh_faces, dim3(blocks_for(n)), dim3(kThreads), 0, stream, tsdf, (int)nx, (int)ny, n, iso,
                       (const unsigned char*)w.mask, (const int*)w.vert_off, (const int*)w.tri_cnt, (const int*)w.tri_off, faces);
    GCP_HIP(hipGetLastError());
  }
  return GCP_OK;
}

}  // extern "C"
