// gcp_median.hip — the median depth of one camera (2DGS's depth_ratio = 1, gsplat's 2DGS mode, RaDe-GS): per pixel the depth of
// the layer at which the transmittance falls through 1/2.  A property of the per-pixel ORDER of layers, so it is formed where the
// weights are, in the tile walk, and cannot be built from the colour, depth and alpha maps.
//
//   Per pixel p of the (H+1) x (W+1) frame, over its list front to back — the pair rule is k_blend_fwd's to the letter: inside the
//   integer box clamped to the frame, g = exp(-1/2 d Λ d^T), T_k the exclusive product of 1 - o g, w_k = T_k o_k g_k, and a pair whose
//   inclusive product T_k (1 - o_k g_k) is exactly 0 is dropped (w = 0).  A pair CONTRIBUTES iff w_k != 0 (the distortion's notion).
//     m(p)            = the LAST contributing pair k of p with T_k > 0.5   (strict)
//     median(p)       = z_m   — a copy of depth[m]: not an interpolation, NOT multiplied by alpha
//     median_index(p) = the Gaussian's row in the call's arrays (what tile_list holds), int32
//     median(p) = 0, median_index(p) = -1 where p has no contributing pair
//   (2DGS's `if (T > 0.5) { median_depth = depth; median_contributor = ...; }`).  Where the pixel's transmittance crosses 1/2, m is
//   the layer that crosses it; where it never does (alpha < 1/2), the pixel's last contributing layer; behind an exactly opaque
//   dropped pair, the last contributing pair in front of it.
//   Backward: median is piecewise constant in everything but z_m,
//     dL/dz_g = sum_{p : median_index(p) = g} G(p),  G = dL/d median;   zero to mean, vinv and opacity.
//
//   k_median_fwd     one 256-thread block per 16x16 tile, one pixel per lane, the list front to back as k_distort_fwd walks it (256
//                    entries staged at a time, the per-wave hit words, the forward blend's association and contraction: the T
//                    compared with 1/2 is the T the image was painted with).  A lane carries T and the LIST POSITION of its
//                    candidate — one select per entry — and reads the Gaussian's row and its depth once, at the end.  T never
//                    rises, so a lane is finished once its T <= 0.5: a wave skips a chunk's hits when none of its lanes is above,
//                    and the block stops staging once none of its four waves is (one LDS word per round parity, decided at the
//                    barrier the staging has anyway).  No checkpoints.
//   k_median_bwd     one block per tile: (index, G) of its 256 pixels into LDS; the lowest pixel that holds each distinct index adds
//                    the matching G in pixel order and writes the (tile, Gaussian) entry's Gaussian-major slot, which follows
//                    from tile_off[g] and g's box alone.  Slots nobody picked stay at the 0 k_median_zero left.
//   k_median_reduce  one thread per Gaussian: the in-order sum of its slots (reduce_slots: a whole-frame splat is folded by its
//                    wave), into grad_depth.
// No float atomics: every sum is taken in a fixed order => the same bits on every run.  No read-back: capture-safe.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gcp_blend_shared.hpp"

namespace {
using namespace gcp;

__global__ __launch_bounds__(256) void k_median_fwd(const BlendArgs a, const float* __restrict__ z, float* __restrict__ median,
                                                    int* __restrict__ index) {
  // the forward blend's arithmetic, contraction included: T here is the T the image was painted with
#pragma clang fp contract(fast)
  __shared__ Staged<kStage> s;
  __shared__ int s_live[2];  // per round parity: some lane of the block is still above 1/2
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave id in an SGPR
  const int tile = blockIdx.x;
  const int ttx = tile % a.tiles_x, tty = tile / a.tiles_x;
  const int px = ttx * kTile + (lane & 15), py = tty * kTile + w * 4 + (lane >> 4);
  const float fx = (float)px, fy = (float)py;
  const bool inside = px <= a.W && py <= a.H;
  const unsigned lane_bits = (1u << (lane & 15)) | (1u << (16 + w * 4 + (lane >> 4)));
  const int first = a.tile_start[tile], last = a.tile_start[tile + 1];
  // a lane outside the frame is in no box: finished from the start, or a partial tile would never stop early
  float T = inside ? 1.0f : 0.0f;
  int km = -1;  // list position of the candidate
  int round = 0;
  for (int base = first; base < last; base += kStage, ++round) {
    const int cnt = __builtin_amdgcn_readfirstlane(min(kStage, last - base));  // scalar loop bound
    // the word of this round's parity was cleared one round ago, behind that round's first barrier
    const bool wave_live = __ballot(T > 0.5f) != 0ull;
    if (round > 0 && wave_live && lane == 0) s_live[round & 1] = 1;
    __syncthreads();
    if (round > 0 && s_live[round & 1] == 0) break;  // block-uniform: nothing behind here can move either output
    if (threadIdx.x == 0) s_live[(round + 1) & 1] = 0;
    stage_entries<false, false>(a, s, base, cnt, ttx * kTile, tty * kTile);
    __syncthreads();
    const int chunks = (cnt + 63) >> 6;
    for (int c = 0; c < chunks; ++c) {
      unsigned long long hits = uniform64(s.hits[w][c]);
      // wave-uniform: no pixel of the strip is above 1/2 any more — T never rises, no candidate can change
      if (__ballot(T > 0.5f) == 0ull) hits = 0ull;
      while (hits) {
        const int k = c * 64 + __builtin_ctzll(hits);
        hits &= hits - 1ull;
        const float4 ge = s.geo[k], vi = s.vin[k];
        if ((__float_as_uint(ge.w) & lane_bits) == lane_bits) {
          const float dx = fx - ge.x, dy = fy - ge.y;
          const float t0 = dx * vi.x + dy * vi.z;  // (d Λ) d^T with the forward blend's association
          const float t1 = dx * vi.y + dy * vi.w;
          const float g = __builtin_amdgcn_exp2f(t0 * dx + t1 * dy);
          const float incl = T * (1.0f - ge.z * g);  // inclusive product
          const float wgt = T * ge.z * g;
          // contributing (kept and w != 0) in front of the crossing
          if (T > 0.5f && incl != 0.0f && wgt != 0.0f) km = base + k;
          T = incl;
        }
      }
    }
  }
  if (inside) {
    const i64 o = (i64)py * (a.W + 1) + px;
    const int g = km >= 0 ? (int)a.tile_list[km] : -1;
    median[o] = km >= 0 ? z[g] : 0.0f;
    index[o] = g;
  }
}

__global__ __launch_bounds__(256) void k_median_fill_empty(float* __restrict__ median, int* __restrict__ index, i64 n) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    median[i] = 0.0f;
    index[i] = -1;
  }
}

__global__ __launch_bounds__(256) void k_median_zero(float* __restrict__ partial, i64 n) {
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) partial[i] = 0.0f;
}

// one block per tile: per distinct index of the tile's pixels, the sum of G in pixel order into the entry's Gaussian-major slot
__global__ __launch_bounds__(256) void k_median_bwd(const int* __restrict__ start, const int* __restrict__ end, i64 n_gauss, int W, int H,
                                                    int tiles_x, const int* __restrict__ tile_off, const int* __restrict__ index,
                                                    const float* __restrict__ grad_median, i64 n_slots, float* __restrict__ partial /*[K]*/) {
  __shared__ int s_idx[256];
  __shared__ float s_g[256];
  const int t = threadIdx.x;
  const int tile = blockIdx.x;
  const int ttx = tile % tiles_x, tty = tile / tiles_x;
  const int px = ttx * kTile + (t & 15), py = tty * kTile + (t >> 4);  // pixel order: row by row inside the tile
  int mine = -1;
  float G = 0.0f;
  if (px <= W && py <= H) {
    const i64 o = (i64)py * (W + 1) + px;
    mine = index[o];
    G = grad_median[o];
  }
  s_idx[t] = mine;
  s_g[t] = G;
  __syncthreads();
  if (__ballot(mine >= 0) == 0ull) return;  // wave-uniform, behind the only barrier
  bool owner = mine >= 0;
  float sum = 0.0f;
  for (int j = 0; j < 256; ++j) {  // every lane reads the same word: a broadcast
    const bool same = s_idx[j] == mine;
    if (same && j < t) owner = false;  // a lower pixel holds this index: the sum is that pixel's
    if (same) sum += s_g[j];
  }
  if (!owner || (i64)mine >= n_gauss) return;
  // the slot of (tile, mine): from tile_off and the Gaussian's box, as entry_slot
  Box b;
  if (!load_box(start, end, mine, W, H, b)) return;
  const int tx0 = b.x0 >> kTileLog2, tx1 = b.x1 >> kTileLog2, ty0 = b.y0 >> kTileLog2, ty1 = b.y1 >> kTileLog2;
  if (ttx < tx0 || ttx > tx1 || tty < ty0 || tty > ty1) return;  // an index the forward on these bins cannot have written
  const i64 e0 = tile_off[mine], e1 = tile_off[mine + 1];
  const i64 e = e0 + (i64)(tty - ty0) * (tx1 - tx0 + 1) + (ttx - tx0);
  if (e0 >= 0 && e < e1 && e < n_slots) partial[e] = sum;  // (a listed entry always is: the binning lists whole Gaussians)
}

__global__ __launch_bounds__(256) void k_median_reduce(const float* __restrict__ partial, const int* __restrict__ tile_off,
                                                       const int* __restrict__ tile_start, int n_tiles, i64 n, i64 capacity,
                                                       float* __restrict__ grad_z) {
  const i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const SlotSums<1> sums = reduce_slots<SlotSums<1>>(partial, tile_off, tile_start, n_tiles, g, n, capacity);
  if (g < n) grad_z[g] = sums.v[0];
}

}  // namespace

extern "C" {

int gcp_blend_median_forward(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv,
                             const float* opacity, const float* depth, int64_t n_gauss, int32_t width, int32_t height,
                             const int32_t* tile_start, const int32_t* tile_list, float* median_map, int32_t* median_index,
                             void* stream) {
  if (n_gauss < 0 || width < 0 || height < 0 || !median_map || !median_index) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss > 0 && (!start_xy || !end_xy || !mean_xy || !vinv || !opacity || !depth || !tile_start || !tile_list))
    return GCP_ERR_INVALID_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
  if (n_gauss == 0) {  // nothing to walk: no pixel has a pair
    const i64 px = (i64)(width + 1) * (i64)(height + 1);
    hipLaunchKernelGGL(k_median_fill_empty, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, st, median_map, median_index, px);
    GCP_HIP(hipGetLastError());
    return GCP_OK;
  }
  BlendArgs a;
  if (make_args(a, start_xy, end_xy, mean_xy, vinv, opacity, nullptr, width, height, tile_start, tile_list) != GCP_OK)
    return GCP_ERR_INVALID_ARGUMENT;
  const TileGrid tg = tile_grid(width, height);
  hipLaunchKernelGGL(k_median_fwd, dim3((unsigned)(tg.tx * tg.ty)), dim3(256), 0, st, a, depth, median_map, median_index);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

size_t gcp_blend_median_backward_workspace_bytes(int64_t n_tile_pairs) {
  return align256((size_t)(n_tile_pairs > 0 ? n_tile_pairs : 1) * sizeof(float));  // one float per entry
}

int gcp_blend_median_backward(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width, int32_t height,
                              const int32_t* tile_off, int64_t n_tile_pairs, const int32_t* tile_start,
                              const int32_t* median_index, const float* grad_median, float* grad_depth, void* ws, size_t ws_bytes,
                              void* stream) {
  if (n_gauss < 0 || n_tile_pairs < 0 || width < 0 || height < 0 || n_tile_pairs > 0x7fffffffLL) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0) return GCP_OK;
  if (!start_xy || !end_xy || !tile_off || !tile_start || !median_index || !grad_median || !grad_depth || !ws)
    return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < gcp_blend_median_backward_workspace_bytes(n_tile_pairs)) return GCP_ERR_WORKSPACE;
  const TileGrid tg = tile_grid(width, height);
  const int n_tiles = tg.tx * tg.ty;
  float* partial = (float*)ws;
  hipStream_t st = (hipStream_t)stream;
  if (n_tile_pairs > 0) {
    // a slot no pixel picked is read by the reduce all the same.  Cleared by a kernel: with hipMemsetAsync in its place, replays
    // of a captured step returned the sums of earlier replays in such slots (profiles/r32_median.md; the cause is not established)
    hipLaunchKernelGGL(k_median_zero, dim3((unsigned)((n_tile_pairs + 255) / 256)), dim3(256), 0, st, partial, (i64)n_tile_pairs);
    GCP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_median_bwd, dim3((unsigned)n_tiles), dim3(256), 0, st, start_xy, end_xy, (i64)n_gauss, (int)width,
                       (int)height, tg.tx, tile_off, median_index, grad_median, (i64)n_tile_pairs, partial);
    GCP_HIP(hipGetLastError());
  }
  // without entries nothing is listed below the capacity 0: the reduce writes zeros
  hipLaunchKernelGGL(k_median_reduce, dim3((unsigned)((n_gauss + 255) / 256)), dim3(256), 0, st, (const float*)partial, tile_off,
                     tile_start, n_tiles, (i64)n_gauss, (i64)n_tile_pairs, grad_depth);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

}  // extern "C"
