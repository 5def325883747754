// gcp_absgrad.hip — the absolute screen-space gradient of one camera (AbsGS; gsplat's absgrad): per Gaussian the sums, over
// the pixels of its box, of |dL/dmu_x(p)| and |dL/dmu_y(p)|, where the blend backward (gcp_blend.hip) returns the signed sums
// — per-pixel gradients of a large splat that is too bright on one side and too dark on the other cancel there.
//
//   Per splat-pixel pair (k, p) the backward counts:   m(k,p) = T_k o_k g_k (c_k - R_k) Λ_k (p - mu_k)
//   with the terms as the back-to-front walk forms them (walk_back, gcp_blend_shared.hpp): c_k = (dL/dI . l_k) (+ dL/dD z_k),
//   the suffix recursion R_{k-1} = R_k + a_k (c_k - R_k) from R = 0 behind the list (depth variant: dL/dI . bg - dL/dA where
//   T_N != 0), m = 0 outside the box clamped to the frame and for a dropped pair (inclusive product exactly 0), and
//   Λ (p - mu) = (A dx + C dy, B dx + D dy) with the raw vinv entries, as grad_reduce expands its moments.
//   grad_mean[k] of the backward is sum_p m(k,p);  absgrad[k] = (sum_p |m_x(k,p)|, sum_p |m_y(k,p)|).
//
//   k_absgrad_tile    one 256-thread block per 16x16 tile, one pixel per lane, on the walk k_blend_bwd runs — the same code, so
//                     the pair set and T_k are the backward's.  Per entry two 16-lane row sums (DPP), parked in LDS at
//                     [entry][pixel row][2]; after every chunk one thread per entry adds the rows in fixed order into the
//                     entry's Gaussian-major slot (the slot k_blend_bwd writes its partial sums to), 2 floats per slot.
//   k_absgrad_reduce  one thread per Gaussian: the in-order sums of its slots (reduce_slots, as k_grad_reduce).
// No float atomics: every sum is taken in a fixed order => the same bits on every run.
// The staging record (here with the raw Λ), the walk and the slot reduction are those of gcp_blend_shared.hpp.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gcp_blend_shared.hpp"

namespace {
using namespace gcp;

// [entry][pixel row of the tile * 2 + axis]; one word of padding per entry: the fold reads with one thread per entry, and a
// stride of 32 words would put all of them on one LDS bank
constexpr int kPartStride = 16 * 2 + 1;

template <bool DEPTH>
__device__ __forceinline__ void absgrad_tile(const BlendArgs& a, const int* __restrict__ tile_off, const float* __restrict__ t_ckpt,
                                             const float* __restrict__ grad_image, i64 n_slots, float2* __restrict__ slot,
                                             const DepthArgs& da) {
#pragma clang fp contract(fast)  // the backward's arithmetic, contraction included
  __shared__ StagedColRaw<kStageBwd> s;
  __shared__ float s_part[kStageBwd][kPartStride];
  const WalkPixel p = walk_pixel<DEPTH>(a, t_ckpt, grad_image, da);
  const int lane = p.lane;
  float* const row_slot = &s_part[0][(p.w * 4 + (lane >> 4)) * 2];
  walk_back<DEPTH>(
      a, da, s, p,
      [&](int k, float op, float dx, float dy, float tg, float d) {
        const float4 ra = s.raw[k];
        const float r_c = (tg * op) * d;              // T o g (c - R): the backward's "common" factor
        const float ax = row_sum16(fabsf(r_c * (ra.x * dx + ra.z * dy)));  // |m_x|: Λ (p - mu) with the raw entries
        const float ay = row_sum16(fabsf(r_c * (ra.y * dx + ra.w * dy)));  // |m_y|
        if ((lane & 15) == 15) {
          row_slot[k * kPartStride] = ax;
          row_slot[k * kPartStride + 1] = ay;
        }
      },
      [&](unsigned hits) {
        if ((lane & 15) == 15)
          for (unsigned hz = hits; hz; hz &= hz - 1) {
            row_slot[__builtin_ctz(hz) * kPartStride] = 0.0f;
            row_slot[__builtin_ctz(hz) * kPartStride + 1] = 0.0f;
          }
      },
      [&](int j, int entry) {
        // add the 16 pixel rows in fixed order; the slot's two dependent loads go first, behind them the LDS reads
        const i64 e = entry_slot(a, tile_off, entry, s.box[j], p.ttx, p.tty);
        float sx = 0.0f, sy = 0.0f;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) {
          if (!(((unsigned)s.hits[wv][0] >> j) & 1u)) continue;  // (j < 32) that wave never wrote its rows for this entry
#pragma unroll
          for (int r = 4 * wv; r < 4 * wv + 4; ++r) {
            sx += s_part[j][2 * r];
            sy += s_part[j][2 * r + 1];
          }
        }
        if (e >= 0 && e < n_slots) slot[e] = make_float2(sx, sy);  // (a listed entry always is: the binning lists whole Gaussians)
      });
}

__global__ __launch_bounds__(256) void k_absgrad_tile(const BlendArgs a, const int* __restrict__ tile_off,
                                                      const float* __restrict__ t_ckpt, const float* __restrict__ grad_image,
                                                      i64 n_slots, float2* __restrict__ slot) {
  absgrad_tile<false>(a, tile_off, t_ckpt, grad_image, n_slots, slot, DepthArgs{});
}

__global__ __launch_bounds__(256) void k_absgrad_tile_depth(const BlendArgs a, const DepthArgs da, const int* __restrict__ tile_off,
                                                            const float* __restrict__ t_ckpt, const float* __restrict__ grad_image,
                                                            i64 n_slots, float2* __restrict__ slot) {
  absgrad_tile<true>(a, tile_off, t_ckpt, grad_image, n_slots, slot, da);
}

// per Gaussian: the in-order sums of its tile slots (reduce_slots: only slots k_absgrad_tile wrote are read)
__global__ __launch_bounds__(256) void k_absgrad_reduce(const float2* __restrict__ slot, const int* __restrict__ tile_off,
                                                        const int* __restrict__ tile_start, int n_tiles, i64 n, i64 capacity,
                                                        float* __restrict__ absgrad /*[n][2]*/) {
  const i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const SlotSums<2> r = reduce_slots<SlotSums<2>>((const float*)slot, tile_off, tile_start, n_tiles, g, n, capacity);
  if (g >= n) return;
  absgrad[2 * g] = r.v[0];
  absgrad[2 * g + 1] = r.v[1];
}


int blend_absgrad(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv, const float* opacity,
                  const float* l_d, int64_t n_gauss, int32_t width, int32_t height, const int32_t* tile_off, int64_t n_tile_pairs,
                  const int32_t* tile_start, const int32_t* tile_list, const float* t_ckpt, const float* grad_image, float* absgrad,
                  const DepthArgs* da, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (n_gauss < 0 || n_tile_pairs < 0 || width < 0 || height < 0 || n_tile_pairs > 0x7fffffffLL) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0) return GCP_OK;
  if (!start_xy || !end_xy || !mean_xy || !vinv || !opacity || !l_d || !tile_off || !tile_start || !t_ckpt || !grad_image || !absgrad ||
      !ws || (n_tile_pairs > 0 && !tile_list) || (da && !da->z))
    return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < gcp_blend_absgrad_workspace_bytes(n_tile_pairs)) return GCP_ERR_WORKSPACE;
  BlendArgs a;
  if (make_args(a, start_xy, end_xy, mean_xy, vinv, opacity, l_d, width, height, tile_start, tile_list) != GCP_OK)
    return GCP_ERR_INVALID_ARGUMENT;
  const TileGrid tg = tile_grid(width, height);
  const int n_tiles = tg.tx * tg.ty;
  const dim3 tiles((unsigned)n_tiles), gauss((unsigned)((n_gauss + 255) / 256)), block(256);
  float2* slot = (float2*)ws;
  if (n_tile_pairs > 0) {
    if (da) hipLaunchKernelGGL(k_absgrad_tile_depth, tiles, block, 0, stream, a, *da, tile_off, t_ckpt, grad_image, (i64)n_tile_pairs, slot);
    else hipLaunchKernelGGL(k_absgrad_tile, tiles, block, 0, stream, a, tile_off, t_ckpt, grad_image, (i64)n_tile_pairs, slot);
    GCP_HIP(hipGetLastError());
  }
  // without entries nothing is listed below the capacity 0: the reduce writes zeros
  hipLaunchKernelGGL(k_absgrad_reduce, gauss, block, 0, stream, (const float2*)slot, tile_off, tile_start, n_tiles, (i64)n_gauss,
                     (i64)n_tile_pairs, absgrad);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

}  // namespace

extern "C" {

size_t gcp_blend_absgrad_workspace_bytes(int64_t n_tile_pairs) {
  return align256((size_t)(n_tile_pairs > 0 ? n_tile_pairs : 1) * sizeof(float2));  // one (sum |m_x|, sum |m_y|) per entry
}

int gcp_blend_absgrad(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv, const float* opacity,
                      const float* l_d, int64_t n_gauss, int32_t width, int32_t height, const int32_t* tile_off,
                      int64_t n_tile_pairs, const int32_t* tile_start, const int32_t* tile_list, const float* t_ckpt,
                      const float* grad_image, float* absgrad, void* ws, size_t ws_bytes, void* stream) {
  return blend_absgrad(start_xy, end_xy, mean_xy, vinv, opacity, l_d, n_gauss, width, height, tile_off, n_tile_pairs, tile_start,
                       tile_list, t_ckpt, grad_image, absgrad, nullptr, ws, ws_bytes, (hipStream_t)stream);
}

int gcp_blend_absgrad_depth(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv,
                            const float* opacity, const float* l_d, const float* depth, const float* background, int64_t n_gauss,
                            int32_t width, int32_t height, const int32_t* tile_off, int64_t n_tile_pairs, const int32_t* tile_start,
                            const int32_t* tile_list, const float* t_ckpt, const float* grad_image, const float* grad_depth_map,
                            const float* grad_alpha_map, float* absgrad, void* ws, size_t ws_bytes, void* stream) {
  DepthArgs da{};
  da.z = depth; da.bg = background; da.grad_depth = grad_depth_map; da.grad_alpha = grad_alpha_map;
  return blend_absgrad(start_xy, end_xy, mean_xy, vinv, opacity, l_d, n_gauss, width, height, tile_off, n_tile_pairs, tile_start,
                       tile_list, t_ckpt, grad_image, absgrad, &da, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"