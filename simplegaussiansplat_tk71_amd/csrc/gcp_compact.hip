// gcp_compact.hip — the two stream compactions behind the scan / the tile-list walk.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gcp_tiles.hpp"

namespace {
using namespace gcp;

// ---- the tail of _create_alpha_brend (gs_model.py:557-564): `!= 0` mask, boolean-mask compaction, / self or - self ----
// One 256-thread block per tile of kCompactTile elements of the ORIGINAL pair order; wave w owns elements
// [1024 w, 1024 w + 1024) of the tile as 4 rows of 64 lanes x 4 consecutive elements (16-byte loads).  WRITE = false:
// the tile's kept count.  WRITE = true: every kept element's rank = tile offset (exclusive scan of the counts) + kept
// elements before it in the tile (per-lane popcounts -> wave prefix in DPP -> 4 LDS words), its value written to that
// slot — neighbouring lanes write neighbouring slots — and the mask as one packed word per lane.
template <bool VEC, bool WRITE>
__global__ __launch_bounds__(256) void k_compact(const float* __restrict__ incl, const float* __restrict__ self, i64 n, int mode,
                                                 int* __restrict__ cnt, const int* __restrict__ off, float* __restrict__ values,
                                                 unsigned char* __restrict__ keep, int* __restrict__ count_dev) {
  __shared__ int s_w[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const i64 base = (i64)blockIdx.x * kCompactTile + (i64)w * 1024;
  float v[4][4], x[4][4];
  unsigned m[4];
  int c[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const i64 p = base + r * 256 + lane * 4;
    if (VEC && p + 3 < n) {
      const float4 a = *reinterpret_cast<const float4*>(incl + p);
      v[r][0] = a.x; v[r][1] = a.y; v[r][2] = a.z; v[r][3] = a.w;
      if (WRITE) {
        const float4 b = *reinterpret_cast<const float4*>(self + p);
        x[r][0] = b.x; x[r][1] = b.y; x[r][2] = b.z; x[r][3] = b.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[r][k] = (p + k < n) ? incl[p + k] : 0.0f;
        if (WRITE) x[r][k] = (p + k < n) ? self[p + k] : 1.0f;
      }
    }
    m[r] = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) m[r] |= (v[r][k] != 0.0f ? 1u : 0u) << k;  // NaN != 0 is true, as in torch (gs_model.py:577)
    c[r] = __builtin_popcount(m[r]);
  }
  // kept elements before this lane inside the wave's 1024: rows in order, lanes in order inside a row
  int before[4];
  int wtot = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int inc = wave_incl_scan_i(c[r]);
    before[r] = wtot + inc - c[r];
    wtot += __builtin_amdgcn_readlane(inc, 63);
  }
  if (lane == 0) s_w[w] = wtot;
  __syncthreads();
  if (!WRITE) {
    if (threadIdx.x == 0) cnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return;
  }
  int woff = off[blockIdx.x];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < w) woff += s_w[j];
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) count_dev[0] = off[blockIdx.x] + s_w[0] + s_w[1] + s_w[2] + s_w[3];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const i64 p = base + r * 256 + lane * 4;
    int o = woff + before[r];
    if (m[r] == 0xfu) {
      // all four kept (every lane of a stretch that drops nothing): one 16-byte store at a 4-byte-aligned slot — a wave
      // then writes 1 KB contiguous with one instruction instead of four strided ones
      typedef float float4_u __attribute__((ext_vector_type(4), aligned(4)));
      float4_u q;
      q.x = mode == 0 ? v[r][0] / x[r][0] : v[r][0] - x[r][0];
      q.y = mode == 0 ? v[r][1] / x[r][1] : v[r][1] - x[r][1];
      q.z = mode == 0 ? v[r][2] / x[r][2] : v[r][2] - x[r][2];
      q.w = mode == 0 ? v[r][3] / x[r][3] : v[r][3] - x[r][3];
      *reinterpret_cast<float4_u*>(values + o) = q;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if ((m[r] >> k) & 1u) {
          values[o] = mode == 0 ? v[r][k] / x[r][k] : v[r][k] - x[r][k];
          ++o;
        }
      }
    }
    if (VEC && p + 3 < n) {
      // bytes 0/1 per element, memory order: bit k of m -> byte k
      *reinterpret_cast<unsigned*>(keep + p) = (m[r] & 1u) | ((m[r] & 2u) << 7) | ((m[r] & 4u) << 14) | ((m[r] & 8u) << 21);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p + k < n) keep[p + k] = (unsigned char)((m[r] >> k) & 1u);
    }
  }
}

// ---- the compaction that is left when the walk has written final values: only where something was dropped ---------------
// per-tile kept counts from the keep bytes of [begin, end) (tile t = elements [begin + 4096 t, ...)): 1 B per element
__global__ __launch_bounds__(256) void k_count_keep(const unsigned char* __restrict__ keep, i64 n, int* __restrict__ cnt) {
  __shared__ int s_w[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const i64 p = (i64)blockIdx.x * kCompactTile + (i64)threadIdx.x * 16;
  int c = 0;
  if ((((uintptr_t)keep) & 15u) == 0 && p + 15 < n) {
    const uint4 q = *reinterpret_cast<const uint4*>(keep + p);
    c = __builtin_popcount(q.x & 0x01010101u) + __builtin_popcount(q.y & 0x01010101u) + __builtin_popcount(q.z & 0x01010101u) +
        __builtin_popcount(q.w & 0x01010101u);
  } else {
    for (int k = 0; k < 16; ++k) c += (p + k < n && keep[p + k]) ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) s_w[w] = c;
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// kept values of [begin, end) to their ranks (tile offsets from the exclusive scan of the counts + ranks inside the tile)
template <bool VEC>
__global__ __launch_bounds__(256) void k_compact_kept(const float* __restrict__ vals, const unsigned char* __restrict__ keep, i64 n,
                                                      const int* __restrict__ off, float* __restrict__ out) {
  __shared__ int s_w[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const i64 base = (i64)blockIdx.x * kCompactTile + (i64)w * 1024;
  float v[4][4];
  unsigned m[4];
  int c[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const i64 p = base + r * 256 + lane * 4;
    m[r] = 0u;
    if (VEC && p + 3 < n) {
      const float4 a = *reinterpret_cast<const float4*>(vals + p);
      v[r][0] = a.x; v[r][1] = a.y; v[r][2] = a.z; v[r][3] = a.w;
      const unsigned q = *reinterpret_cast<const unsigned*>(keep + p);  // bytes 0 / 1, memory order
      m[r] = (q & 1u) | ((q >> 7) & 2u) | ((q >> 14) & 4u) | ((q >> 21) & 8u);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[r][k] = (p + k < n) ? vals[p + k] : 0.0f;
        m[r] |= ((p + k < n && keep[p + k]) ? 1u : 0u) << k;
      }
    }
    c[r] = __builtin_popcount(m[r]);
  }
  int before[4];
  int wtot = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int inc = wave_incl_scan_i(c[r]);
    before[r] = wtot + inc - c[r];
    wtot += __builtin_amdgcn_readlane(inc, 63);
  }
  if (lane == 0) s_w[w] = wtot;
  __syncthreads();
  int woff = off[blockIdx.x];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < w) woff += s_w[j];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int o = woff + before[r];
    if (m[r] == 0xfu) {
      typedef float float4_u __attribute__((ext_vector_type(4), aligned(4)));
      float4_u q;
      q.x = v[r][0]; q.y = v[r][1]; q.z = v[r][2]; q.w = v[r][3];
      *reinterpret_cast<float4_u*>(out + o) = q;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((m[r] >> k) & 1u) out[o++] = v[r][k];
    }
  }
}

}  // namespace

extern "C" {

size_t gcp_compact_workspace_bytes(int64_t n) {
  const int64_t nb = ((n > 0 ? n : 1) + kCompactTile - 1) / kCompactTile + 1;
  return align256((size_t)(nb + 1) * sizeof(int)) * 2 + gcp_scan_i32_workspace_bytes(nb);
}

// per-tile kept counts from the counts of dropped elements gcp_pairs_scan_boxes took while writing the array
static __global__ void k_counts_from_dropped(const int* __restrict__ dropped, i64 n, i64 nb, int* __restrict__ cnt) {
  const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nb) return;
  const i64 len = n - t * kCompactTile;
  cnt[t] = (int)(len < kCompactTile ? len : kCompactTile) - dropped[t];
}

int gcp_compact_finish(const float* inclusive, const float* self, int64_t begin, int64_t end, int32_t mode, float* values,
                       uint8_t* keep, int32_t* count_dev, const int32_t* dropped_per_tile, void* ws, size_t ws_bytes,
                       void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (begin < 0 || end < begin || end - begin > 0x7fffffffLL || (mode != 0 && mode != 1) || !count_dev) return GCP_ERR_INVALID_ARGUMENT;
  if (dropped_per_tile && begin % kCompactTile != 0) return GCP_ERR_INVALID_ARGUMENT;
  const i64 n = end - begin;
  if (n == 0) {
    GCP_HIP(hipMemsetAsync(count_dev, 0, sizeof(int), stream));
    return GCP_OK;
  }
  if (!inclusive || !self || !values || !keep || !ws) return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < gcp_compact_workspace_bytes(n)) return GCP_ERR_WORKSPACE;
  const i64 nb = (n + kCompactTile - 1) / kCompactTile;
  char* p = (char*)ws;
  int* cnt = carve<int>(p, (size_t)(nb + 1));
  int* off = carve<int>(p, (size_t)(nb + 1));
  int* sws = (int*)p;
  const bool vec = (((uintptr_t)(inclusive + begin) | (uintptr_t)(self + begin) | (uintptr_t)keep) & 15u) == 0;
  // (a last tile cut short by `end` gets a count that covers elements beyond it: never used — ranks come from the
  // exclusive scan of the tiles before, the total from the write pass)
  if (dropped_per_tile)
    hipLaunchKernelGGL(k_counts_from_dropped, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, stream,
                       dropped_per_tile + begin / kCompactTile, n, nb, cnt);
  else if (vec) hipLaunchKernelGGL((k_compact<true, false>), dim3((unsigned)nb), dim3(256), 0, stream, inclusive + begin, self + begin, n, mode, cnt,
                                   (const int*)nullptr, (float*)nullptr, (unsigned char*)nullptr, (int*)nullptr);
  else hipLaunchKernelGGL((k_compact<false, false>), dim3((unsigned)nb), dim3(256), 0, stream, inclusive + begin, self + begin, n, mode, cnt,
                          (const int*)nullptr, (float*)nullptr, (unsigned char*)nullptr, (int*)nullptr);
  GCP_HIP(hipGetLastError());
  const int st = launch_excl_scan(cnt, off, nb, sws, stream);
  if (st != GCP_OK) return st;
  if (vec) hipLaunchKernelGGL((k_compact<true, true>), dim3((unsigned)nb), dim3(256), 0, stream, inclusive + begin, self + begin, n, mode,
                              (int*)nullptr, (const int*)off, values, keep, count_dev);
  else hipLaunchKernelGGL((k_compact<false, true>), dim3((unsigned)nb), dim3(256), 0, stream, inclusive + begin, self + begin, n, mode,
                          (int*)nullptr, (const int*)off, values, keep, count_dev);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

size_t gcp_compact_kept_workspace_bytes(int64_t n) { return gcp_compact_workspace_bytes(n); }

// One launch, one block: the per-tile kept counts from what the walk dropped (or, from_dropped = false, the counts as
// k_count_keep left them) and their TOTAL — all the read-back that sizes the result needs; the prefix sums are only made
// when something has to be moved (gcp_compact_kept_write).
static __global__ __launch_bounds__(1024) void k_kept_total(const int* __restrict__ dropped, i64 n, i64 nb, int* __restrict__ cnt,
                                                            int* __restrict__ count_dev, bool from_dropped) {
  __shared__ int s_w[16];
  int s = 0;
  // eight loads in flight per thread (one at a time, the 40 rounds of a 1.65e8-pair list took 27 us: a round trip each)
  for (i64 t0 = threadIdx.x; t0 < nb; t0 += 8 * 1024) {
    int v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const i64 t = t0 + u * 1024;
      v[u] = t < nb ? (from_dropped ? dropped[t] : cnt[t]) : 0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const i64 t = t0 + u * 1024;
      if (t >= nb) continue;
      int c = v[u];
      if (from_dropped) {
        const i64 len = n - t * kCompactTile;
        c = (int)(len < kCompactTile ? len : kCompactTile) - c;
        cnt[t] = c;
      }
      s += c;
    }
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int j = 0; j < 16; ++j) tot += s_w[j];
    count_dev[0] = tot;
  }
}

int gcp_compact_kept_count(const uint8_t* keep, const int32_t* dropped_per_tile, int64_t n_total, int64_t begin, int64_t end,
                           int32_t* count_dev, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (begin < 0 || end < begin || end > n_total || end - begin > 0x7fffffffLL || !count_dev) return GCP_ERR_INVALID_ARGUMENT;
  const i64 n = end - begin;
  if (n == 0) {
    GCP_HIP(hipMemsetAsync(count_dev, 0, sizeof(int), stream));
    return GCP_OK;
  }
  if (!keep || !ws) return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < gcp_compact_kept_workspace_bytes(n)) return GCP_ERR_WORKSPACE;
  const i64 nb = (n + kCompactTile - 1) / kCompactTile;
  int* cnt = (int*)ws;  // (the prefix sums behind the counts are gcp_compact_kept_write's)
  // the walk's own counts serve when the range's tiles are the array's tiles and its last tile is not cut short by `end`
  if (dropped_per_tile && begin % kCompactTile == 0 && (end == n_total || end % kCompactTile == 0)) {
    hipLaunchKernelGGL(k_kept_total, dim3(1), dim3(1024), 0, stream, dropped_per_tile + begin / kCompactTile, n, nb, cnt, count_dev, true);
  } else {
    hipLaunchKernelGGL(k_count_keep, dim3((unsigned)nb), dim3(256), 0, stream, keep + begin, n, cnt);
    hipLaunchKernelGGL(k_kept_total, dim3(1), dim3(1024), 0, stream, (const int*)nullptr, n, nb, cnt, count_dev, false);
  }
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int gcp_compact_kept_write(const float* values_in, const uint8_t* keep, int64_t begin, int64_t end, float* values_out, void* ws,
                           size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (begin < 0 || end < begin || end - begin > 0x7fffffffLL) return GCP_ERR_INVALID_ARGUMENT;
  const i64 n = end - begin;
  if (n == 0) return GCP_OK;
  if (!values_in || !keep || !values_out || !ws) return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < gcp_compact_kept_workspace_bytes(n)) return GCP_ERR_WORKSPACE;
  const i64 nb = (n + kCompactTile - 1) / kCompactTile;
  // ranks of the tiles from the counts gcp_compact_kept_count left in ws
  char* p = (char*)ws;
  const int* cnt = carve<int>(p, (size_t)(nb + 1));
  int* off = carve<int>(p, (size_t)(nb + 1));
  const int st = launch_excl_scan(cnt, off, nb, (int*)p, stream);
  if (st != GCP_OK) return st;
  const bool vec = (((uintptr_t)(values_in + begin)) & 15u) == 0 && (((uintptr_t)(keep + begin)) & 3u) == 0;
  if (vec) hipLaunchKernelGGL((k_compact_kept<true>), dim3((unsigned)nb), dim3(256), 0, stream, values_in + begin, keep + begin, n, off, values_out);
  else hipLaunchKernelGGL((k_compact_kept<false>), dim3((unsigned)nb), dim3(256), 0, stream, values_in + begin, keep + begin, n, off, values_out);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

}  // extern "C"
