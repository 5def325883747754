// gcp_contrib.hip — what every Gaussian contributes to one camera's image: per Gaussian the maximum and the sum, over the
// pixels of its box, of the colour weight w = T o g that k_blend_fwd (gcp_blend.hip) forms for every splat-pixel pair and
// throws away.  The maximum is RadSplat's importance score, the sum LightGaussian's significance; the prune built on
// them is GS_model_with_param.prune_by_contribution.
//
//   The pair rule is k_blend_fwd's to the letter: a pixel belongs to a Gaussian if it lies inside the Gaussian's integer
//   box clamped to the frame; g = exp(-0.5 d Λ d^T); T the exclusive product of 1 - o g over the earlier entries whose box
//   holds the pixel; w = T o g, and w = 0 where the inclusive product T (1 - o g) is exactly 0 (the dropped pair).
//
//   k_contrib_tile    one 256-thread block per 16x16 tile, one pixel per lane, the tile's list front to back as the forward
//                     blend walks it (entries staged through LDS 256 at a time, the per-wave hit words, the wave-uniform
//                     exit behind an exact zero, exp2 on Λ' = -0.5 log2(e) Λ) — without colours.  Per entry a wave reduces
//                     its 64 values of w to a maximum and a sum (a fixed DPP scan: the 16 lanes of a pixel row, then the
//                     four rows) and parks the pair in LDS at [entry][wave]; after every staged chunk one thread per entry
//                     folds the waves that hit it, in wave order, and writes the entry's Gaussian-major slot (the slot
//                     k_blend_bwd writes its partial sums to).
//   k_contrib_reduce  one thread per Gaussian: the maximum and the in-order sum of its slots (reduce_slots, as k_grad_reduce: a
//                     Gaussian with 128 slots or more is taken by its whole wave).
// No float atomics: a maximum is exact in any order and every sum is taken in a fixed order => the same bits on every run.
// The staging, the slot address and the slot reduction are those of gcp_blend_shared.hpp; the record staged is its common part
// (no colour) with the parked pairs added.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gcp_blend_shared.hpp"

namespace {
using namespace gcp;

struct ContribStaged : Staged<kStage> {  // the common record, no colour: box, geo, vin (a b c d), hits
  float2 part[kStage][4];  // [entry][wave]: (max, sum) of w over the wave's 64 pixels; written only where hits says so
};

// Maximum and sum of a value over the wave in a fixed order, valid in lane 63: an inclusive scan along each 16-lane DPP
// row (= one pixel row of the tile), then row 0 into row 1 and row 2 into row 3, then row 1 into row 3.  A lane without a
// source takes 0.  The maximum is taken on the bit patterns: w >= 0 (a product of factors in [0, 1]), so its bits order
// as integers do, and v_max_i32 takes the DPP operand directly where fmaxf costs a canonicalising instruction per step.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void scan_step(int& mx, float& sm) {
  mx = max(mx, dpp_i<CTRL, ROW_MASK>(0, mx));
  sm += dpp_f<CTRL, ROW_MASK>(0.0f, sm);
}
__device__ __forceinline__ void wave_max_sum(float& w_max, float& sm) {
  int mx = __float_as_int(w_max);
  scan_step<0x111, 0xf>(mx, sm);
  scan_step<0x112, 0xf>(mx, sm);
  scan_step<0x114, 0xf>(mx, sm);
  scan_step<0x118, 0xf>(mx, sm);
  scan_step<0x142, 0xa>(mx, sm);
  scan_step<0x143, 0xc>(mx, sm);
  w_max = __int_as_float(mx);
}

__global__ __launch_bounds__(256) void k_contrib_tile(const BlendArgs a, const int* __restrict__ tile_off, i64 n_slots,
                                                      float2* __restrict__ slot /*[n_slots] (max, sum)*/) {
  // the forward blend's arithmetic, contraction included: w here is the weight the image was painted with
#pragma clang fp contract(fast)
  __shared__ ContribStaged s;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave id in an SGPR
  const int tile = blockIdx.x;
  const int ttx = tile % a.tiles_x, tty = tile / a.tiles_x;
  const float fx = (float)(ttx * kTile + (lane & 15)), fy = (float)(tty * kTile + w * 4 + (lane >> 4));
  const unsigned lane_bits = (1u << (lane & 15)) | (1u << (16 + w * 4 + (lane >> 4)));
  const int first = a.tile_start[tile], last = a.tile_start[tile + 1];
  float T = 1.0f;
  for (int base = first; base < last; base += kStage) {
    const int cnt = __builtin_amdgcn_readfirstlane(min(kStage, last - base));  // scalar loop bound
    __syncthreads();
    stage_entries<false, false>(a, s, base, cnt, ttx * kTile, tty * kTile);
    __syncthreads();
    const int chunks = (cnt + 63) >> 6;
    for (int c = 0; c < chunks; ++c) {
      const unsigned long long hits64 = uniform64(s.hits[w][c]);
      if (!hits64) continue;
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const int e0 = c * 64 + sub * 32;
        unsigned hits = (unsigned)(hits64 >> (sub * 32));
        // wave-uniform: every pixel of the strip is behind an exact zero — T stays 0, every further w is exactly 0: the wave
        // hands the fold its zeros for the rest of its hits, 32 entries per store
        if (__ballot(T != 0.0f) == 0ull) {
          if (lane < 32 && ((hits >> lane) & 1u)) s.part[e0 + lane][w] = make_float2(0.0f, 0.0f);
          continue;
        }
        while (hits) {
          const int k = e0 + __builtin_ctz(hits);
          hits &= hits - 1;
          const float4 ge = s.geo[k], vi = s.vin[k];
          // straight-line for all 64 lanes (every lane joins the reduction); pixels outside the box and dropped pairs are
          // zeroed with selects
          const bool in = (__float_as_uint(ge.w) & lane_bits) == lane_bits;
          const float dx = fx - ge.x, dy = fy - ge.y;
          const float t0 = dx * vi.x + dy * vi.z;  // (d Λ) d^T with the forward blend's association
          const float t1 = dx * vi.y + dy * vi.w;
          const float g = __builtin_amdgcn_exp2f(t0 * dx + t1 * dy);
          const float incl = T * (1.0f - ge.z * g);            // inclusive product
          const float wgt = (in && incl != 0.0f) ? T * ge.z * g : 0.0f;  // dropped when exactly 0
          T = in ? incl : T;
          float mx = wgt, sm = wgt;
          wave_max_sum(mx, sm);
          if (lane == 63) s.part[k][w] = make_float2(mx, sm);
        }
      }
    }
    __syncthreads();
    // one thread per entry: the waves that hit it in wave order, into the entry's Gaussian-major slot
    for (int j = threadIdx.x; j < cnt; j += 256) {
      const i64 e = entry_slot(a, tile_off, base + j, s.box[j], ttx, tty);
      float mx = 0.0f, sm = 0.0f;
#pragma unroll
      for (int wv = 0; wv < 4; ++wv) {
        if (!((s.hits[wv][j >> 6] >> (j & 63)) & 1ull)) continue;  // that wave never wrote its pair for this entry
        const float2 p = s.part[j][wv];
        mx = fmaxf(mx, p.x);
        sm += p.y;
      }
      if (e >= 0 && e < n_slots) slot[e] = make_float2(mx, sm);  // (a listed entry always is: the binning lists whole Gaussians)
    }
  }
}

// (max, sum) per slot; the maximum of non-negative values from 0
struct SlotMaxSum {
  float mx = 0.0f, sm = 0.0f;
  __device__ __forceinline__ void add(const float2* __restrict__ slot, i64 e) {
    const float2 p = slot[e];
    mx = fmaxf(mx, p.x);
    sm += p.y;
  }
  __device__ __forceinline__ void wave_all() {
    for (int o = 32; o > 0; o >>= 1) {
      mx = fmaxf(mx, __shfl_xor(mx, o));
      sm += __shfl_xor(sm, o);
    }
  }
};

// per Gaussian: the maximum and the in-order sum of its tile slots (reduce_slots of gcp_blend_shared.hpp: only slots
// k_contrib_tile wrote are read)
__global__ __launch_bounds__(256) void k_contrib_reduce(const float2* __restrict__ slot, const int* __restrict__ tile_off,
                                                        const int* __restrict__ tile_start, int n_tiles, i64 n, i64 capacity,
                                                        float* __restrict__ w_max, float* __restrict__ w_sum) {
  const i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const SlotMaxSum r = reduce_slots<SlotMaxSum>(slot, tile_off, tile_start, n_tiles, g, n, capacity);
  if (g >= n) return;
  w_max[g] = r.mx;
  w_sum[g] = r.sm;
}

}  // namespace

extern "C" {

size_t gcp_blend_contrib_workspace_bytes(int64_t n_tile_pairs) {
  return align256((size_t)(n_tile_pairs > 0 ? n_tile_pairs : 1) * sizeof(float2));  // one (max, sum) per entry
}

int gcp_blend_contrib(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv, const float* opacity,
                      int64_t n_gauss, int32_t width, int32_t height, const int32_t* tile_off, int64_t n_tile_pairs,
                      const int32_t* tile_start, const int32_t* tile_list, float* w_max, float* w_sum, void* ws, size_t ws_bytes,
                      void* stream) {
  if (n_gauss < 0 || n_tile_pairs < 0 || width < 0 || height < 0 || n_tile_pairs > 0x7fffffffLL) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0) return GCP_OK;
  if (!start_xy || !end_xy || !mean_xy || !vinv || !opacity || !tile_off || !tile_start || !w_max || !w_sum || !ws ||
      (n_tile_pairs > 0 && !tile_list))
    return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < gcp_blend_contrib_workspace_bytes(n_tile_pairs)) return GCP_ERR_WORKSPACE;
  BlendArgs a;
  if (make_args(a, start_xy, end_xy, mean_xy, vinv, opacity, nullptr, width, height, tile_start, tile_list) != GCP_OK)
    return GCP_ERR_INVALID_ARGUMENT;
  const TileGrid tg = tile_grid(width, height);
  const int n_tiles = tg.tx * tg.ty;
  const dim3 tiles((unsigned)n_tiles), gauss((unsigned)((n_gauss + 255) / 256)), block(256);
  float2* slot = (float2*)ws;
  hipStream_t st = (hipStream_t)stream;
  if (n_tile_pairs > 0) {
    hipLaunchKernelGGL(k_contrib_tile, tiles, block, 0, st, a, tile_off, (i64)n_tile_pairs, slot);
    GCP_HIP(hipGetLastError());
  }
  // without entries nothing is listed below the capacity 0: the reduce writes zeros
  hipLaunchKernelGGL(k_contrib_reduce, gauss, block, 0, st, (const float2*)slot, tile_off, tile_start, n_tiles, (i64)n_gauss,
                     (i64)n_tile_pairs, w_max, w_sum);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

}  // extern "C"
