// gcp_knn.hip — exact k nearest neighbours of every point of a cloud among the OTHER points of the same cloud: what the
// initial scale of every Gaussian is made of (upstream 3DGS: simple-knn's distCUDA2; the reference: torch.cdist + topk).
//
// The definition (pinned in grouped_cumprod_hip.h): d2(i, j) = (dx dx + dy dy) + dz dz in float32, in that association, of the
// float32 differences (the library is compiled with -ffp-contract=off); row i lists the k smallest pairs (d2, j), j != i,
// ascending, lexicographic.  The result is a function of the input alone: nothing below depends on the launch shape, the
// stream, the workspace's earlier contents or the spatial order, and no atomic exists in this file.
//
// The method is simple-knn's, made hierarchical:
//   k_knn_box_partial / k_knn_box_final   bounding box of the cloud (min / max: any order gives the same bits)
//   k_knn_keys                            30-bit Morton key per point, 10 bits per axis, clamped; zero extent -> cell 0
//   gcp_sort_pairs_u32(key_bits = 30)     stable radix sort: the permutation
//   k_knn_gather                          points in sorted order, (x, y, z, original index) as one 16-byte word
//   k_knn_leaf_boxes                      exact min / max box of every LEAF = 64 consecutive sorted points, one wave each
//   k_knn_group_boxes                     box of every GROUP = 64 consecutive leaves, one wave each
//   k_knn_search<KC>                      one wave per leaf, one lane per query: own leaf first, then every group (the own one
//                                         first), the leaves of the groups that could not be pruned, their points
// The keys decide only how tight the boxes are, never the result: a cloud whose points all share one key is searched by brute
// force.  Pruning stays exact in float32: per axis e = max(lo - q, q - hi, 0), the squares summed in the association of d2 — a
// bound that is <= the COMPUTED d2 of every point in the box because rounding is monotone — and a node is skipped only when
// the bound is STRICTLY greater than the query's current worst kept distance in every lane of the wave (on equality a lower
// index may still win).  The decision is taken per lane and combined by a ballot, so the branch is wave-uniform and the
// addresses of boxes and candidate points are too: they are read through the scalar cache, once per wave.
// All loops are counted (groups, leaves, points): no input can keep a kernel running.  The best list of a lane lives in
// registers: capacity KC in {2, 4, 8, 16} is a template parameter, k is rounded up to it and the list is only ever indexed by
// unrolled loop counters (pruning then uses the KC-th best, which is >= the k-th: still exact).
#include <math.h>

#include "gcp_device.hpp"
#include "grouped_cumprod_hip.h"

namespace {

using gcp::align256;
using gcp::carve;
using gcp::i64;

constexpr int kThreads = 256;
constexpr int kLeaf = 64;        // points per leaf: one wave's worth
constexpr int kFan = 64;         // leaves per group
constexpr int kBoxChunk = 4096;  // points per block of the bounding-box pass (16 per thread): one partial box each
constexpr int kEmpty = 0x7fffffff;  // index of a slot that holds nothing yet: above every real index (n < 2^31)

struct Box { float lo[3], pad0, hi[3], pad1; };  // 32 bytes

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

// Lane 0 of the wave writes the box of the wave's (lo, hi) values; lanes without a value bring (+inf, -inf).
__device__ __forceinline__ void wave_box_store(const float lo[3], const float hi[3], Box* out) {
  float l[3], h[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    l[a] = wave_min(lo[a]);
    h[a] = wave_max(hi[a]);
  }
  if ((threadIdx.x & 63) == 0) {
    Box b;
    b.lo[0] = l[0], b.lo[1] = l[1], b.lo[2] = l[2], b.pad0 = 0.0f;
    b.hi[0] = h[0], b.hi[1] = h[1], b.hi[2] = h[2], b.pad1 = 0.0f;
    *out = b;
  }
}

// Block b reduces points [b kBoxChunk, (b + 1) kBoxChunk) to partial[b].
__global__ __launch_bounds__(kThreads) void k_knn_box_partial(const float* __restrict__ xyz, i64 n, Box* __restrict__ partial) {
  __shared__ Box s_box[kThreads / 64];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const i64 base = (i64)blockIdx.x * kBoxChunk;
  for (int r = 0; r < kBoxChunk / kThreads; ++r) {
    const i64 i = base + r * kThreads + threadIdx.x;
    if (i < n) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float v = xyz[3 * i + a];
        lo[a] = fminf(lo[a], v);
        hi[a] = fmaxf(hi[a], v);
      }
    }
  }
  wave_box_store(lo, hi, &s_box[threadIdx.x >> 6]);
  __syncthreads();
  if (threadIdx.x < 64) {
    const bool have = threadIdx.x < kThreads / 64;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = have ? s_box[threadIdx.x].lo[a] : INFINITY;
      hi[a] = have ? s_box[threadIdx.x].hi[a] : -INFINITY;
    }
    wave_box_store(lo, hi, &partial[blockIdx.x]);
  }
}

// One block: the box of all partial boxes.
__global__ __launch_bounds__(kThreads) void k_knn_box_final(const Box* __restrict__ partial, i64 n_partial, Box* __restrict__ box) {
  __shared__ Box s_box[kThreads / 64];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (i64 i = threadIdx.x; i < n_partial; i += kThreads) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = fminf(lo[a], partial[i].lo[a]);
      hi[a] = fmaxf(hi[a], partial[i].hi[a]);
    }
  }
  wave_box_store(lo, hi, &s_box[threadIdx.x >> 6]);
  __syncthreads();
  if (threadIdx.x < 64) {
    const bool have = threadIdx.x < kThreads / 64;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = have ? s_box[threadIdx.x].lo[a] : INFINITY;
      hi[a] = have ? s_box[threadIdx.x].hi[a] : -INFINITY;
    }
    wave_box_store(lo, hi, box);
  }
}

// Cell 0..1023 of v on an axis [lo, hi]; a zero (or non-finite) extent maps to cell 0; fmaxf / fminf swallow a NaN.
__device__ __forceinline__ unsigned knn_cell(float v, float lo, float hi) {
  const float ext = hi - lo;
  const float t = ext > 0.0f ? (v - lo) / ext * 1024.0f : 0.0f;
  return (unsigned)(int)fminf(fmaxf(t, 0.0f), 1023.0f);
}
__device__ __forceinline__ unsigned spread10(unsigned v) {  // bit i of the low 10 -> bit 3 i
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

__global__ __launch_bounds__(kThreads) void k_knn_keys(const float* __restrict__ xyz, i64 n, const Box* __restrict__ box,
                                                        unsigned* __restrict__ key) {
  const i64 i = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const Box b = *box;
  const unsigned cx = knn_cell(xyz[3 * i], b.lo[0], b.hi[0]);
  const unsigned cy = knn_cell(xyz[3 * i + 1], b.lo[1], b.hi[1]);
  const unsigned cz = knn_cell(xyz[3 * i + 2], b.lo[2], b.hi[2]);
  key[i] = spread10(cx) | (spread10(cy) << 1) | (spread10(cz) << 2);
}

__global__ __launch_bounds__(kThreads) void k_knn_gather(const float* __restrict__ xyz, const int* __restrict__ perm, i64 n,
                                                          float4* __restrict__ pts) {
  const i64 i = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int j = perm[i];
  pts[i] = make_float4(xyz[3 * (i64)j], xyz[3 * (i64)j + 1], xyz[3 * (i64)j + 2], __int_as_float(j));
}

// Wave w of the grid: the box of sorted points [64 w, 64 w + 64) cut at n.
__global__ __launch_bounds__(kThreads) void k_knn_leaf_boxes(const float4* __restrict__ pts, i64 n, i64 n_leaves, Box* __restrict__ leaf) {
  const i64 w = (i64)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (w >= n_leaves) return;
  const i64 i = w * kLeaf + (threadIdx.x & 63);
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < n) {
    const float4 p = pts[i];
    lo[0] = hi[0] = p.x, lo[1] = hi[1] = p.y, lo[2] = hi[2] = p.z;
  }
  wave_box_store(lo, hi, &leaf[w]);
}

// Wave w of the grid: the box of leaves [64 w, 64 w + 64) cut at n_leaves.
__global__ __launch_bounds__(kThreads) void k_knn_group_boxes(const Box* __restrict__ leaf, i64 n_leaves, i64 n_groups, Box* __restrict__ group) {
  const i64 w = (i64)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (w >= n_groups) return;
  const i64 i = w * kFan + (threadIdx.x & 63);
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < n_leaves) {
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = leaf[i].lo[a], hi[a] = leaf[i].hi[a];
  }
  wave_box_store(lo, hi, &group[w]);
}

// (d, j) < (e, m), lexicographic
__device__ __forceinline__ bool pair_less(float d, int j, float e, int m) { return d < e || (d == e && j < m); }

template <int KC>
struct Best {
  float d[KC];
  int j[KC];

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int s = 0; s < KC; ++s) d[s] = INFINITY, j[s] = kEmpty;
  }
  // Sorted insertion by selects, every index a compile-time constant: slot s takes its left neighbour where the candidate
  // goes in front of that, the candidate where it goes in front of slot s only, and keeps its value otherwise.
  __device__ __forceinline__ void insert(float cd, int cj) {
    if (!pair_less(cd, cj, d[KC - 1], j[KC - 1])) return;
#pragma unroll
    for (int s = KC - 1; s >= 1; --s) {
      const bool before_left = pair_less(cd, cj, d[s - 1], j[s - 1]);
      const bool before_this = pair_less(cd, cj, d[s], j[s]);
      d[s] = before_left ? d[s - 1] : (before_this ? cd : d[s]);
      j[s] = before_left ? j[s - 1] : (before_this ? cj : j[s]);
    }
    if (pair_less(cd, cj, d[0], j[0])) d[0] = cd, j[0] = cj;
  }
};

// The lower bound of d2 from q to every point of the box, in the arithmetic of d2.
__device__ __forceinline__ float box_bound(const Box& b, float qx, float qy, float qz) {
  const float ex = fmaxf(fmaxf(b.lo[0] - qx, qx - b.hi[0]), 0.0f);
  const float ey = fmaxf(fmaxf(b.lo[1] - qy, qy - b.hi[1]), 0.0f);
  const float ez = fmaxf(fmaxf(b.lo[2] - qz, qz - b.hi[2]), 0.0f);
  return (ex * ex + ey * ey) + ez * ez;
}

// True when no lane of the wave can gain anything from the box (`live`: the lane holds a query).  A NaN bound descends.
template <int KC>
__device__ __forceinline__ bool wave_prunes(const Box& b, float qx, float qy, float qz, const Best<KC>& best, bool live) {
  const bool wants = live && !(box_bound(b, qx, qy, qz) > best.d[KC - 1]);
  return __builtin_amdgcn_ballot_w64(wants) == 0;
}

template <int KC>
__device__ __forceinline__ void scan_leaf(const float4* __restrict__ pts, i64 n, i64 l, float qx, float qy, float qz, int qj, bool live,
                                          Best<KC>& best) {
  const i64 first = l * kLeaf;
  const int count = (int)(n - first < kLeaf ? n - first : kLeaf);
  for (int p = 0; p < count; ++p) {
    const float4 c = pts[first + p];  // a wave-uniform address
    const int cj = __float_as_int(c.w);
    const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    if (live && cj != qj) best.insert(d2, cj);
  }
}

template <int KC>
__global__ __launch_bounds__(kThreads) void k_knn_search(const float4* __restrict__ pts, const Box* __restrict__ leaf, const Box* __restrict__ group,
                                                          i64 n, i64 n_leaves, i64 n_groups, int k, int* __restrict__ index,
                                                          float* __restrict__ dist2) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const i64 own = (i64)blockIdx.x * (kThreads / 64) + wave;  // the leaf this wave's lanes are the points of
  if (own >= n_leaves) return;
  const i64 own_group = own / kFan;
  const i64 i = own * kLeaf + (threadIdx.x & 63);
  const bool live = i < n;
  const float4 q = pts[live ? i : n - 1];
  const int qj = __float_as_int(q.w);
  Best<KC> best;
  best.clear();
  scan_leaf<KC>(pts, n, own, q.x, q.y, q.z, qj, live, best);
  for (i64 gi = 0; gi < n_groups; ++gi) {
    const i64 g = gi == 0 ? own_group : (gi <= own_group ? gi - 1 : gi);  // the own group first, then the others in order
    if (wave_prunes<KC>(group[g], q.x, q.y, q.z, best, live)) continue;
    const i64 l0 = g * kFan;
    const int leaves = (int)(n_leaves - l0 < kFan ? n_leaves - l0 : kFan);
    for (int li = 0; li < leaves; ++li) {
      const i64 l = l0 + li;
      if (l == own) continue;
      if (wave_prunes<KC>(leaf[l], q.x, q.y, q.z, best, live)) continue;
      scan_leaf<KC>(pts, n, l, q.x, q.y, q.z, qj, live, best);
    }
  }
  if (!live) return;
#pragma unroll
  for (int s = 0; s < KC; ++s) {
    if (s < k) {
      const bool filled = best.j[s] != kEmpty;
      index[(i64)qj * k + s] = filled ? best.j[s] : -1;
      dist2[(i64)qj * k + s] = filled ? best.d[s] : INFINITY;
    }
  }
}

struct Plan {
  i64 n_leaves, n_groups, n_partial;
};
inline Plan plan_for(i64 n) {
  Plan p;
  p.n_leaves = (n + kLeaf - 1) / kLeaf;
  p.n_groups = (p.n_leaves + kFan - 1) / kFan;
  p.n_partial = (n + kBoxChunk - 1) / kBoxChunk;
  return p;
}
inline unsigned blocks_for(i64 items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

}  // namespace

extern "C" size_t gcp_knn_workspace_bytes(int64_t n) {
  const i64 m = n > 0 ? n : 1;
  const Plan p = plan_for(m);
  size_t b = 2 * align256((size_t)m * sizeof(unsigned));  // keys, sorted keys
  b += align256((size_t)m * sizeof(int));                  // permutation
  b += align256((size_t)m * sizeof(float4));               // sorted points
  b += align256((size_t)p.n_leaves * sizeof(Box)) + align256((size_t)p.n_groups * sizeof(Box));
  b += align256((size_t)p.n_partial * sizeof(Box)) + align256(sizeof(Box));
  return b + gcp_sort_workspace_bytes(m) + 256;  // + what moving `ws` up to a 16-byte boundary may cost
}

extern "C" int gcp_knn(const float* xyz, int64_t n, int32_t k, int32_t* index, float* dist2, void* ws, size_t ws_bytes, void* stream_) {
  if (n < 0 || n > 0x7fffffffLL - 1 || k < 1 || k > 16) return GCP_ERR_INVALID_ARGUMENT;
  if (n == 0) return GCP_OK;
  if (!xyz || !index || !dist2 || !ws) return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < gcp_knn_workspace_bytes(n)) return GCP_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const Plan pl = plan_for(n);
  char* p = (char*)(((uintptr_t)ws + 15u) & ~(uintptr_t)15u);  // the 16-byte points and the sort's vector loads
  float4* pts = carve<float4>(p, (size_t)n);
  unsigned* key = carve<unsigned>(p, (size_t)n);
  unsigned* key_sorted = carve<unsigned>(p, (size_t)n);
  int* perm = carve<int>(p, (size_t)n);
  Box* leaf = carve<Box>(p, (size_t)pl.n_leaves);
  Box* group = carve<Box>(p, (size_t)pl.n_groups);
  Box* partial = carve<Box>(p, (size_t)pl.n_partial);
  Box* box = carve<Box>(p, 1);
  void* sort_ws = p;
  const size_t sort_bytes = gcp_sort_workspace_bytes(n);

  hipLaunchKernelGGL(k_knn_box_partial, dim3((unsigned)pl.n_partial), dim3(kThreads), 0, stream, xyz, (i64)n, partial);
  GCP_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_knn_box_final, dim3(1), dim3(kThreads), 0, stream, (const Box*)partial, pl.n_partial, box);
  GCP_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_knn_keys, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, stream, xyz, (i64)n, (const Box*)box, key);
  GCP_HIP(hipGetLastError());
  const int st = gcp_sort_pairs_u32(key, n, 30, key_sorted, perm, sort_ws, sort_bytes, stream_);
  if (st != GCP_OK) return st;
  hipLaunchKernelGGL(k_knn_gather, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, stream, xyz, (const int*)perm, (i64)n, pts);
  GCP_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_knn_leaf_boxes, dim3(blocks_for(pl.n_leaves, kThreads / 64)), dim3(kThreads), 0, stream, (const float4*)pts, (i64)n,
                     pl.n_leaves, leaf);
  GCP_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_knn_group_boxes, dim3(blocks_for(pl.n_groups, kThreads / 64)), dim3(kThreads), 0, stream, (const Box*)leaf, pl.n_leaves,
                     pl.n_groups, group);
  GCP_HIP(hipGetLastError());
  const dim3 grid(blocks_for(pl.n_leaves, kThreads / 64)), block(kThreads);
#define GCP_KNN_SEARCH(KC)                                                                                                          \
  hipLaunchKernelGGL((k_knn_search<KC>), grid, block, 0, stream, (const float4*)pts, (const Box*)leaf, (const Box*)group, (i64)n, \
                     pl.n_leaves, pl.n_groups, (int)k, index, dist2)
  if (k <= 2) GCP_KNN_SEARCH(2);
  else if (k <= 4) GCP_KNN_SEARCH(4);
  else if (k <= 8) GCP_KNN_SEARCH(8);
  else GCP_KNN_SEARCH(16);
#undef GCP_KNN_SEARCH
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}
