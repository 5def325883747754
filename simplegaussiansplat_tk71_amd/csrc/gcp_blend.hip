// gcp_blend.hip — fused per-pixel alpha blending over the tile lists, colour-only and with
// depth / alpha / background.
//
//   f1  One 256-thread block per tile, one pixel per lane.  The tile's list is staged through LDS
//       256 entries at a time; every lane walks it in depth order keeping its own transmittance
//       T (the exclusive grouped cumprod of the scan path, sequential per pixel), box-tests,
//       evaluates g = exp(-0.5 d Λ d^T), and accumulates colour.  Pixels are owned by lanes:
//       no atomics, deterministic.  A wave skips an entry when no lane is inside its box.
//       Backward walks each tile list BACK TO FRONT in chunks of kStageBwd entries: the exclusive suffix
//       sum S_k of (dL/dI . p) the reference gets from a flipped grouped cumsum (gs_model.py:716-722)
//       is carried in the normalised form S_k / (1 - o_k g_k) = T_k * R_k with the recurrence
//       R_{k-1} = R_k + o_k g_k ((dL/dI . l_k) - R_k)  — a convex combination: no accumulated sum is
//       subtracted — and T_k (the exclusive transmittance) comes from the entry behind it,
//       T_k = T_{k+1} / (1 - o_k g_k), restarted at every chunk from the checkpoint the forward kernel
//       saved for the chunk's end (T per pixel every kStageBwd entries, and behind the whole list); the
//       one chunk per pixel in which T underflows is recomputed front to back instead.  Every gradient
//       term is T_k times a bounded quantity, so its round-off is relative to the transmittance of
//       ITS OWN layer whatever the depth.
//       Per-pair gradients collapse to 7 per-lane values;
//       they are summed along each pixel row of the tile (16 lanes = one DPP row, 4 fused
//       v_add_f32_dpp) into LDS, one thread per entry folds the 16 rows (dy is constant along a
//       row) into the entry's slot in Gaussian-major order, and a last kernel sums each Gaussian's
//       few slots.  (An entry-parallel variant with the pair values parked in LDS was measured
//       slower, 1.88 vs 1.69 ms: it cannot skip the waves an entry does not touch.)
//       No float atomics anywhere => bitwise reproducible.
//   The staging of a list chunk, the back-to-front walk itself (T_k, c_k - R_k, the recurrence; the slow and the dead chunk), the
//   slot address and the per-Gaussian slot reduction live in gcp_blend_shared.hpp, where gcp_absgrad.hip and gcp_contrib.hip
//   take them from too; this file holds the forward walk, what the backward does per entry, the folds and the host side.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gcp_blend_shared.hpp"

namespace {
using namespace gcp;

constexpr int kGradVals = 9;        // per (tile, Gaussian) slot: go, gl0..2, S(c dx), S(c dy), S(c dx dx), S(c dx dy), S(c dy dy)
constexpr int kGradValsDepth = 10;  // (depth variant: + S(dL/dD w), the depth gradient)
constexpr int kRowVals = 7;         // per pixel row in LDS: go, gl0..2, S(c), S(c dx), S(c dx dx)   (dy is constant along a row)
constexpr int kRowSlots = 8;        // LDS slots per pixel row (the transposed reduction below leaves 8 values in 8 lane classes)

// One step of the transposed reduction: lanes with `second` false keep value a, the others keep b; each adds its
// partner's copy of the value it keeps (partner = DPP pattern CTRL, which must flip the class bit).
template <int CTRL>
__device__ __forceinline__ float xchg_sum(bool second, float a, float b) {
  const float keep = second ? b : a, send = second ? a : b;
  return keep + dpp_f<CTRL, 0xf>(0.0f, send);
}

inline size_t ckpt_floats(i64 n_tile_pairs, int n_tiles) {  // the checkpoint slots of gcp_blend_shared.hpp: ckpt_slot0
  return (size_t)((n_tile_pairs > 0 ? n_tile_pairs : 0) / kCkpt + 2 * (i64)n_tiles + 2) * 256u;
}

template <bool CKPT, bool DEPTH>
__device__ __forceinline__ void blend_fwd_tile(const BlendArgs& a, float* __restrict__ image, float* __restrict__ t_ckpt,
                                               const DepthArgs& da) {
  // The blend kernels are VALU-issue bound: let a*b+c contract into v_fma_f32 here (the library is otherwise built
  // with -ffp-contract=off).  One rounding instead of two per contraction; results stay within the 1e-5 bar.
#pragma clang fp contract(fast)
  __shared__ StagedCol<kStage> s;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave id in an SGPR: the row test below is scalar
  const int tile = blockIdx.x;
  const int px = (tile % a.tiles_x) * kTile + (lane & 15);
  const int py = (tile / a.tiles_x) * kTile + w * 4 + (lane >> 4);
  const float fx = (float)px, fy = (float)py;
  const unsigned lane_bits = (1u << (lane & 15)) | (1u << (16 + w * 4 + (lane >> 4)));
  const int first = a.tile_start[tile], last = a.tile_start[tile + 1];
  float* const ck = CKPT ? t_ckpt + ckpt_slot0(first, tile) * 256 + threadIdx.x : nullptr;
  float T = 1.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, cz = 0.0f;
  for (int base = first; base < last; base += kStage) {
    const int cnt = __builtin_amdgcn_readfirstlane(min(kStage, last - base));  // scalar loop bound
    __syncthreads();
    stage_entries<false, DEPTH>(a, s, base, cnt, (tile % a.tiles_x) * kTile, (tile / a.tiles_x) * kTile, da.z);
    __syncthreads();
    // Only the entries whose rows reach this wave (hits[w]), in list order.  Every listed entry is used, so all
    // three of its LDS records are read together, ahead of the membership branch.  (Reading one entry ahead of the
    // blend, with two register sets, changes nothing: 93 % of the launch is VALU issue.)
    auto blend = [&](const float4& ge, const float4& vi, const float4& co) {
      if ((__float_as_uint(ge.w) & lane_bits) == lane_bits) {  // (the branch-free form of the backward is 4 % slower here)
        const float dx = fx - ge.x, dy = fy - ge.y;
        // (d Λ) d^T with the association of the reference's two matmuls (gs_model.py:495)
        const float t0 = dx * vi.x + dy * vi.z;
        const float t1 = dx * vi.y + dy * vi.w;
        const float g = __builtin_amdgcn_exp2f(t0 * dx + t1 * dy);  // = exp(-0.5 (d Λ) d^T), gs_model.py:495
        const float anti = 1.0f - ge.z * g;             // gs_model.py:535
        const float incl = T * anti;                    // inclusive grouped cumprod
        if (incl != 0.0f) {                             // gs_model.py:560: dropped when exactly 0
          const float wgt = T * ge.z * g;               // gs_model.py:500
          c0 += wgt * co.x; c1 += wgt * co.y; c2 += wgt * co.z;
          if (DEPTH) cz += wgt * co.w;                  // expected depth: one more weighted channel
        }
        T = incl;
      }
    };
    const int chunks = (cnt + 63) >> 6;
    for (int c = 0; c < chunks; ++c) {
      const unsigned long long hits64 = uniform64(s.hits[w][c]);
      if (!CKPT && !hits64) continue;
#pragma unroll
      for (int sub = 0; sub < 64 / kCkpt; ++sub) {
        const int e0 = c * 64 + sub * kCkpt;  // first staged entry of this checkpoint interval
        if (CKPT) {
          if (e0 >= cnt) break;  // wave-uniform
          // the transmittance entering list entry base + e0 (the backward restarts its front-to-back pass from here)
          ck[(i64)((base - first + e0) / kCkpt) * 256] = T;
        }
        unsigned hits = (unsigned)(hits64 >> (sub * kCkpt)) & (unsigned)((1ull << kCkpt) - 1ull);
        // wave-uniform: every pixel of the strip is behind an exact zero (an opaque layer, or a product that underflowed
        // hundreds of layers deep) — T stays 0 and nothing more reaches the image: the rest of the list costs this wave its
        // checkpoints only
        if (__ballot(T != 0.0f) == 0ull) hits = 0u;
        while (hits) {
          const int k = e0 + __builtin_ctz(hits);
          hits &= hits - 1;
          const float4 ge = s.geo[k], vi = s.vin[k], co = s.col[k];
          asm volatile("" :: "v"(vi.x), "v"(co.x));  // keep the reads ahead of the branch
          blend(ge, vi, co);
        }
      }
    }
  }
  if (CKPT) ck[(i64)((last - first + kCkpt - 1) / kCkpt) * 256] = T;  // behind the whole list
  if (px <= a.W && py <= a.H) {
    float* o = image + ((i64)py * (a.W + 1) + px) * 3;
    if (DEPTH && da.bg) {  // composited over the background
      c0 += T * da.bg[0]; c1 += T * da.bg[1]; c2 += T * da.bg[2];
    }
    o[0] = c0; o[1] = c1; o[2] = c2;
    if (DEPTH) {
      da.depth[(i64)py * (a.W + 1) + px] = cz;
      da.alpha[(i64)py * (a.W + 1) + px] = 1.0f - T;
    }
  }
}

template <bool CKPT>
__global__ __launch_bounds__(256) void k_blend_fwd(const BlendArgs a, float* __restrict__ image, float* __restrict__ t_ckpt) {
  blend_fwd_tile<CKPT, false>(a, image, t_ckpt, DepthArgs{});
}

template <bool CKPT>
__global__ __launch_bounds__(256) void k_blend_fwd_depth(const BlendArgs a, const DepthArgs da, float* __restrict__ image,
                                                         float* __restrict__ t_ckpt) {
  blend_fwd_tile<CKPT, true>(a, image, t_ckpt, da);
}

// the sums of three per-pixel values over the tile in a fixed order (a butterfly per wave, then the four waves in order),
// written by threads 0-2: no atomics, the same bits on every run
__device__ __forceinline__ void tile_sum3(float v0, float v1, float v2, float* out) {
  __shared__ float s_w[4][3];
  for (int o = 32; o > 0; o >>= 1) {
    v0 += __shfl_xor(v0, o); v1 += __shfl_xor(v1, o); v2 += __shfl_xor(v2, o);
  }
  if ((threadIdx.x & 63) == 0) {
    s_w[threadIdx.x >> 6][0] = v0; s_w[threadIdx.x >> 6][1] = v1; s_w[threadIdx.x >> 6][2] = v2;
  }
  __syncthreads();
  if (threadIdx.x < 3) out[threadIdx.x] = ((s_w[0][threadIdx.x] + s_w[1][threadIdx.x]) + s_w[2][threadIdx.x]) + s_w[3][threadIdx.x];
}

// Backward: per (tile, entry) partial sums, written to the entry's Gaussian-major slot.  The walk (T_k, c_k, R_k; the quotient,
// the slow chunk, the dead chunk) is walk_back of gcp_blend_shared.hpp; here is what the backward does per entry — seven or
// eight per-lane values summed along each pixel row of the tile — and the fold of the rows into the slot.
template <bool DEPTH>
__device__ __forceinline__ void blend_bwd_tile(const BlendArgs& a, const int* __restrict__ tile_off,
                                               const float* __restrict__ t_ckpt,
                                               const float* __restrict__ grad_image,
                                               float* __restrict__ partial /*[K][kGradVals or kGradValsDepth]*/,
                                               const DepthArgs& da) {
#pragma clang fp contract(fast)  // as in k_blend_fwd
  constexpr int kVals = DEPTH ? kGradValsDepth : kGradVals;
  __shared__ StagedCol<kStageBwd> s;
  // [entry][pixel row of the tile * kRowSlots + value]; one word of padding per entry: the fold below reads with one
  // thread per entry, and a stride of 128 words would put all of them on one LDS bank
  constexpr int kPartStride = 16 * kRowSlots + 1;
  __shared__ float s_part[kStageBwd][kPartStride];
  const WalkPixel p = walk_pixel<DEPTH>(a, t_ckpt, grad_image, da);
  const int lane = p.lane;
  const float g0 = p.g0, g1 = p.g1, g2 = p.g2, gz = p.gz;
  const bool b1 = lane & 2;
  float* const row_slot = &s_part[0][(p.w * 4 + (lane >> 4)) * kRowSlots + ((lane & 2) ? 4 : 0) + ((lane & 4) ? 2 : 0) + ((lane & 8) ? 1 : 0)];
  if (DEPTH && da.tile_bg) tile_sum3(g0 * p.T_N, g1 * p.T_N, g2 * p.T_N, da.tile_bg + 3 * (i64)p.tile);
  walk_back<DEPTH>(
      a, da, s, p,
      [&](int k, float op, float dx, float /*dy*/, float tg, float d) {
        float r_o = tg * d;
        const float wgt = tg * op;                              // T o g (gs_model.py:500 without l)
        float r_c = wgt * d;
        float r_l0 = g0 * wgt, r_l1 = g1 * wgt, r_l2 = g2 * wgt;
        float r_cx = r_c * dx;
        float r_xx = r_cx * dx;
        // Seven 16-lane row sums by a transposed butterfly: at each step a lane keeps half of its values and hands the
        // other half to its partner, so the live registers halve.  Partners: 15-i, 7-i (within each half), i^2, i^1;
        // afterwards lane i holds the row sum of value ((i>>1)&1)*4 + ((i>>2)&1)*2 + ((i>>3)&1) (slot 7 is a dummy).
        // The first two steps split the lanes by bit 3 and bit 2, i.e. by DPP bank: two bank-masked v_add_f32_dpp
        // writing one destination do "keep + partner's copy" for both classes without a select (7 + 4 VALU); the last
        // two need selects (3 + 1).  15 VALU instead of 7 x 4 = 28.
        float q0, q1, q2, q3, p0, p1;
        // s_nop 1: a DPP source written by the preceding VALU instruction needs two wait states
        if constexpr (DEPTH) {
          // slot 7 carries the depth gradient: lanes 8-15 of q3 take S(dL/dD w) instead of a second copy of S(c dx dx)
          const float r_z = gz * wgt;
          asm volatile(
              "s_nop 1\n\t"
              "v_add_f32_dpp %0, %4, %4 row_mirror row_mask:0xf bank_mask:0x3\n\t"    // lanes 0-7 : go
              "v_add_f32_dpp %1, %6, %6 row_mirror row_mask:0xf bank_mask:0x3\n\t"    //             gl1
              "v_add_f32_dpp %2, %8, %8 row_mirror row_mask:0xf bank_mask:0x3\n\t"    //             S(c)
              "v_add_f32_dpp %3, %10, %10 row_mirror row_mask:0xf bank_mask:0x3\n\t"  //             S(c dx dx)
              "v_add_f32_dpp %0, %5, %5 row_mirror row_mask:0xf bank_mask:0xc\n\t"    // lanes 8-15: gl0
              "v_add_f32_dpp %1, %7, %7 row_mirror row_mask:0xf bank_mask:0xc\n\t"    //             gl2
              "v_add_f32_dpp %2, %9, %9 row_mirror row_mask:0xf bank_mask:0xc\n\t"    //             S(c dx)
              "v_add_f32_dpp %3, %11, %11 row_mirror row_mask:0xf bank_mask:0xc\n\t"  //             S(dL/dD w)
              : "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(q3)
              : "v"(r_o), "v"(r_l0), "v"(r_l1), "v"(r_l2), "v"(r_c), "v"(r_cx), "v"(r_xx), "v"(r_z));
        } else {
          asm volatile(
              "s_nop 1\n\t"
              "v_add_f32_dpp %0, %4, %4 row_mirror row_mask:0xf bank_mask:0x3\n\t"    // lanes 0-7 : go
              "v_add_f32_dpp %1, %6, %6 row_mirror row_mask:0xf bank_mask:0x3\n\t"    //             gl1
              "v_add_f32_dpp %2, %8, %8 row_mirror row_mask:0xf bank_mask:0x3\n\t"    //             S(c)
              "v_add_f32_dpp %3, %10, %10 row_mirror row_mask:0xf bank_mask:0xf\n\t"  // all lanes : S(c dx dx)
              "v_add_f32_dpp %0, %5, %5 row_mirror row_mask:0xf bank_mask:0xc\n\t"    // lanes 8-15: gl0
              "v_add_f32_dpp %1, %7, %7 row_mirror row_mask:0xf bank_mask:0xc\n\t"    //             gl2
              "v_add_f32_dpp %2, %9, %9 row_mirror row_mask:0xf bank_mask:0xc\n\t"    //             S(c dx)
              : "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(q3)
              : "v"(r_o), "v"(r_l0), "v"(r_l1), "v"(r_l2), "v"(r_c), "v"(r_cx), "v"(r_xx));
        }
        asm volatile(
            "s_nop 1\n\t"
            "v_add_f32_dpp %0, %2, %2 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"  // bit 2 clear: from q0 / q2
            "v_add_f32_dpp %1, %4, %4 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"
            "v_add_f32_dpp %0, %3, %3 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"  // bit 2 set  : from q1 / q3
            "v_add_f32_dpp %1, %5, %5 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"
            : "=&v"(p0), "=&v"(p1)
            : "v"(q0), "v"(q1), "v"(q2), "v"(q3));
        const float o0 = xchg_sum<0x4e>(b1, p0, p1);
        const float tot = o0 + dpp_f<0xb1, 0xf>(0.0f, o0);
        row_slot[k * kPartStride] = tot;  // lanes i and i^1 store the same word
      },
      [&](unsigned hits) {
        for (unsigned hz = hits; hz; hz &= hz - 1) row_slot[__builtin_ctz(hz) * kPartStride] = 0.0f;
      },
      [&](int j, int entry) {
        // add the 16 pixel rows in fixed order
        float* out = partial + entry_slot(a, tile_off, entry, s.box[j], p.ttx, p.tty) * kVals;
        const float my = s.geo[j].y;
        float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f, o3 = 0.0f, cx = 0.0f, cy = 0.0f, xx = 0.0f, xy = 0.0f, yy = 0.0f, zz = 0.0f;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) {
          if (!((s.hits[wv][0] >> j) & 1ull)) continue;  // that wave never wrote its rows for this entry
#pragma unroll
          for (int r = 4 * wv; r < 4 * wv + 4; ++r) {
            const float* d = &s_part[j][r * kRowSlots];
            const float dy = (float)(p.tty * kTile + r) - my;  // constant along the pixel row
            o0 += d[0]; o1 += d[1]; o2 += d[2]; o3 += d[3];
            cx += d[5]; cy += dy * d[4];
            xx += d[6]; xy += dy * d[5]; yy += dy * dy * d[4];
            if (DEPTH) zz += d[7];
          }
        }
        out[0] = o0; out[1] = o1; out[2] = o2; out[3] = o3; out[4] = cx; out[5] = cy; out[6] = xx; out[7] = xy; out[8] = yy;
        if (DEPTH) out[9] = zz;
      });
}

__global__ __launch_bounds__(256) void k_blend_bwd(const BlendArgs a, const int* __restrict__ tile_off,
                                                   const float* __restrict__ t_ckpt,
                                                   const float* __restrict__ grad_image,
                                                   float* __restrict__ partial /*[K][kGradVals]*/) {
  blend_bwd_tile<false>(a, tile_off, t_ckpt, grad_image, partial, DepthArgs{});
}

__global__ __launch_bounds__(256) void k_blend_bwd_depth(const BlendArgs a, const DepthArgs da, const int* __restrict__ tile_off,
                                                         const float* __restrict__ t_ckpt, const float* __restrict__ grad_image,
                                                         float* __restrict__ partial /*[K][kGradValsDepth]*/) {
  blend_bwd_tile<true>(a, tile_off, t_ckpt, grad_image, partial, da);
}


// per Gaussian: sum its tile slots in order (reduce_slots of gcp_blend_shared.hpp), expand the moments into the four gradients.
template <int NV>
__device__ __forceinline__ void grad_reduce(const float* __restrict__ partial, const int* __restrict__ tile_off,
                                            const int* __restrict__ tile_start, int n_tiles, const float* __restrict__ vinv, i64 n,
                                            i64 capacity, float* grad_mean, float* grad_vinv, float* grad_opacity, float* grad_l,
                                            float* grad_z) {
  const i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const SlotSums<NV> sums = reduce_slots<SlotSums<NV>>(partial, tile_off, tile_start, n_tiles, g, n, capacity);
  const float* r = sums.v;
  if (g >= n) return;
  const float A = vinv[4 * g], B = vinv[4 * g + 1], C = vinv[4 * g + 2], D = vinv[4 * g + 3];
  grad_opacity[g] = r[0];
  grad_l[3 * g] = r[1]; grad_l[3 * g + 1] = r[2]; grad_l[3 * g + 2] = r[3];
  // sum common * (d Λ): x0 = dx a + dy c, x1 = dx b + dy d   (gs_model.py:745)
  grad_mean[2 * g] = r[4] * A + r[5] * C;
  grad_mean[2 * g + 1] = r[4] * B + r[5] * D;
  // -0.5 * sum common * d^T d   (gs_model.py:755-758)
  grad_vinv[4 * g] = -0.5f * r[6];
  grad_vinv[4 * g + 1] = -0.5f * r[7];
  grad_vinv[4 * g + 2] = -0.5f * r[7];
  grad_vinv[4 * g + 3] = -0.5f * r[8];
  if (NV > kGradVals) grad_z[g] = r[NV - 1];
}

__global__ __launch_bounds__(256) void k_grad_reduce(const float* __restrict__ partial, const int* __restrict__ tile_off,
                                                     const int* __restrict__ tile_start, int n_tiles, const float* __restrict__ vinv, i64 n,
                                                     i64 capacity, float* grad_mean, float* grad_vinv, float* grad_opacity, float* grad_l) {
  grad_reduce<kGradVals>(partial, tile_off, tile_start, n_tiles, vinv, n, capacity, grad_mean, grad_vinv, grad_opacity, grad_l, nullptr);
}

__global__ __launch_bounds__(256) void k_grad_reduce_depth(const float* __restrict__ partial, const int* __restrict__ tile_off,
                                                           const int* __restrict__ tile_start, int n_tiles, const float* __restrict__ vinv,
                                                           i64 n, i64 capacity, float* grad_mean, float* grad_vinv, float* grad_opacity,
                                                           float* grad_l, float* grad_z) {
  grad_reduce<kGradValsDepth>(partial, tile_off, tile_start, n_tiles, vinv, n, capacity, grad_mean, grad_vinv, grad_opacity, grad_l,
                              grad_z);
}

// dL/dbg: the per-tile sums k_blend_bwd_depth wrote, added by ONE block in a fixed order (a strided sum per thread, then a
// tree) — the same bits on every run
__global__ __launch_bounds__(256) void k_bg_reduce(const float* __restrict__ tile_bg, int n_tiles, float* __restrict__ grad_bg) {
  __shared__ float s[3][256];
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
  for (int t = threadIdx.x; t < n_tiles; t += 256) {
    a0 += tile_bg[3 * (i64)t]; a1 += tile_bg[3 * (i64)t + 1]; a2 += tile_bg[3 * (i64)t + 2];
  }
  s[0][threadIdx.x] = a0; s[1][threadIdx.x] = a1; s[2][threadIdx.x] = a2;
  for (int o = 128; o > 0; o >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < o)
      for (int c = 0; c < 3; ++c) s[c][threadIdx.x] += s[c][threadIdx.x + o];
  }
  __syncthreads();
  if (threadIdx.x < 3) grad_bg[threadIdx.x] = s[threadIdx.x][0];
}

}  // namespace

extern "C" {

size_t gcp_blend_checkpoint_floats(int64_t n_tile_pairs, int32_t width, int32_t height) {
  if (width < 0 || height < 0) return 0;
  const TileGrid tg = tile_grid(width, height);
  return ckpt_floats((i64)n_tile_pairs, tg.tx * tg.ty);
}

// Forward of both entry points; `da` null: colour only.  The depth call also needs its two maps, the depths and the list.
static int blend_forward(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv,
                         const float* opacity, const float* l_d, int64_t n_gauss, int32_t width, int32_t height,
                         const int32_t* tile_start, const int32_t* tile_list, float* image, float* t_ckpt, const DepthArgs* da,
                         hipStream_t stream) {
  BlendArgs a;
  const int st = make_args(a, start_xy, end_xy, mean_xy, vinv, opacity, l_d, width, height, tile_start, tile_list);
  if (st != GCP_OK || !image || n_gauss < 0) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss > 0 && (!start_xy || !end_xy || !mean_xy || !vinv || !opacity || !l_d)) return GCP_ERR_INVALID_ARGUMENT;
  if (da && (!da->depth || !da->alpha || (n_gauss > 0 && (!da->z || !tile_list)))) return GCP_ERR_INVALID_ARGUMENT;
  const TileGrid tg = tile_grid(width, height);
  const dim3 grid((unsigned)(tg.tx * tg.ty)), block(256);
  if (da && t_ckpt) hipLaunchKernelGGL((k_blend_fwd_depth<true>), grid, block, 0, stream, a, *da, image, t_ckpt);
  else if (da) hipLaunchKernelGGL((k_blend_fwd_depth<false>), grid, block, 0, stream, a, *da, image, (float*)nullptr);
  else if (t_ckpt) hipLaunchKernelGGL((k_blend_fwd<true>), grid, block, 0, stream, a, image, t_ckpt);
  else hipLaunchKernelGGL((k_blend_fwd<false>), grid, block, 0, stream, a, image, (float*)nullptr);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int gcp_blend_forward(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv,
                      const float* opacity, const float* l_d, int64_t n_gauss, int32_t width, int32_t height,
                      const int32_t* tile_start, const int32_t* tile_list, float* image, float* t_ckpt, void* stream) {
  return blend_forward(start_xy, end_xy, mean_xy, vinv, opacity, l_d, n_gauss, width, height, tile_start, tile_list, image, t_ckpt,
                       nullptr, (hipStream_t)stream);
}

int gcp_blend_forward_depth(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv,
                            const float* opacity, const float* l_d, const float* depth, const float* background, int64_t n_gauss,
                            int32_t width, int32_t height, const int32_t* tile_start, const int32_t* tile_list, float* image,
                            float* depth_map, float* alpha_map, float* t_ckpt, void* stream) {
  DepthArgs da{};
  da.z = depth; da.bg = background; da.depth = depth_map; da.alpha = alpha_map;
  return blend_forward(start_xy, end_xy, mean_xy, vinv, opacity, l_d, n_gauss, width, height, tile_start, tile_list, image, t_ckpt,
                       &da, (hipStream_t)stream);
}

size_t gcp_blend_backward_workspace_bytes(int64_t n_tile_pairs) {
  // per-entry partial sums
  return align256((size_t)(n_tile_pairs > 0 ? n_tile_pairs : 1) * kGradVals * sizeof(float));
}

size_t gcp_blend_backward_depth_workspace_bytes(int64_t n_tile_pairs, int32_t width, int32_t height) {
  if (width < 0 || height < 0) return 0;
  const TileGrid tg = tile_grid(width, height);
  // per-entry partial sums, then the per-tile background sums
  return align256((size_t)(n_tile_pairs > 0 ? n_tile_pairs : 1) * kGradValsDepth * sizeof(float)) +
         align256((size_t)tg.tx * tg.ty * 3 * sizeof(float));
}

// Backward of both entry points; `da` null: colour only (grad_z and grad_bg are the depth call's).  The two contracts differ
// and both are kept: without Gaussians the colour call has nothing to do and returns before it looks at anything else, while
// the depth call still owes the background its gradient — it needs t_ckpt and grad_image whatever n_gauss is.
static int blend_backward(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv,
                          const float* opacity, const float* l_d, int64_t n_gauss, int32_t width, int32_t height,
                          const int32_t* tile_off, int64_t n_tile_pairs, const int32_t* tile_start, const int32_t* tile_list,
                          const float* t_ckpt, const float* grad_image, float* grad_mean, float* grad_vinv, float* grad_opacity,
                          float* grad_l, float* grad_z, float* grad_bg, const DepthArgs* da, void* ws, size_t ws_bytes,
                          hipStream_t stream) {
  BlendArgs a;
  const int st = make_args(a, start_xy, end_xy, mean_xy, vinv, opacity, l_d, width, height, tile_start, tile_list);
  if (st != GCP_OK || n_gauss < 0 || n_tile_pairs < 0) return GCP_ERR_INVALID_ARGUMENT;
  if (!da && n_gauss == 0) return GCP_OK;
  if (!t_ckpt || !grad_image) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss > 0 && (!start_xy || !end_xy || !mean_xy || !vinv || !opacity || !l_d || !tile_off || !grad_mean || !grad_vinv ||
                      !grad_opacity || !grad_l))
    return GCP_ERR_INVALID_ARGUMENT;
  if (da && n_gauss > 0 && (!da->z || !tile_list || !grad_z)) return GCP_ERR_INVALID_ARGUMENT;
  if (da && n_gauss == 0 && !grad_bg) return GCP_OK;
  if (!ws) return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < (da ? gcp_blend_backward_depth_workspace_bytes(n_tile_pairs, width, height) : gcp_blend_backward_workspace_bytes(n_tile_pairs)))
    return GCP_ERR_WORKSPACE;
  const TileGrid tg = tile_grid(width, height);
  const int n_tiles = tg.tx * tg.ty;
  const dim3 tiles((unsigned)n_tiles), gauss((unsigned)((n_gauss + 255) / 256)), block(256);
  char* p = (char*)ws;
  float* partial = carve<float>(p, (size_t)(n_tile_pairs > 0 ? n_tile_pairs : 1) * (da ? kGradValsDepth : kGradVals));
  if (!da) {
    if (n_tile_pairs > 0) {
      hipLaunchKernelGGL(k_blend_bwd, tiles, block, 0, stream, a, tile_off, t_ckpt, grad_image, partial);
      GCP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_grad_reduce, gauss, block, 0, stream, (const float*)partial, tile_off, tile_start, n_tiles, vinv,
                       (i64)n_gauss, (i64)n_tile_pairs, grad_mean, grad_vinv, grad_opacity, grad_l);
    GCP_HIP(hipGetLastError());
    return GCP_OK;
  }
  DepthArgs d = *da;
  d.tile_bg = grad_bg ? (float*)p : nullptr;  // the per-tile background sums lie behind the partial sums
  // every tile, also one without entries: the background gradient needs every pixel's T_N
  hipLaunchKernelGGL(k_blend_bwd_depth, tiles, block, 0, stream, a, d, tile_off, t_ckpt, grad_image, partial);
  GCP_HIP(hipGetLastError());
  if (n_gauss > 0) {
    hipLaunchKernelGGL(k_grad_reduce_depth, gauss, block, 0, stream, (const float*)partial, tile_off, tile_start, n_tiles, vinv,
                       (i64)n_gauss, (i64)n_tile_pairs, grad_mean, grad_vinv, grad_opacity, grad_l, grad_z);
    GCP_HIP(hipGetLastError());
  }
  if (grad_bg) {
    hipLaunchKernelGGL(k_bg_reduce, dim3(1), block, 0, stream, (const float*)d.tile_bg, n_tiles, grad_bg);
    GCP_HIP(hipGetLastError());
  }
  return GCP_OK;
}

int gcp_blend_backward(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv,
                       const float* opacity, const float* l_d, int64_t n_gauss, int32_t width, int32_t height,
                       const int32_t* tile_off, int64_t n_tile_pairs, const int32_t* tile_start,
                       const int32_t* tile_list, const float* t_ckpt, const float* grad_image, float* grad_mean,
                       float* grad_vinv, float* grad_opacity, float* grad_l, void* ws, size_t ws_bytes,
                       void* stream) {
  return blend_backward(start_xy, end_xy, mean_xy, vinv, opacity, l_d, n_gauss, width, height, tile_off, n_tile_pairs, tile_start,
                        tile_list, t_ckpt, grad_image, grad_mean, grad_vinv, grad_opacity, grad_l, nullptr, nullptr, nullptr, ws,
                        ws_bytes, (hipStream_t)stream);
}

int gcp_blend_backward_depth(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv,
                             const float* opacity, const float* l_d, const float* depth, const float* background, int64_t n_gauss,
                             int32_t width, int32_t height, const int32_t* tile_off, int64_t n_tile_pairs,
                             const int32_t* tile_start, const int32_t* tile_list, const float* t_ckpt, const float* grad_image,
                             const float* grad_depth_map, const float* grad_alpha_map, float* grad_mean, float* grad_vinv,
                             float* grad_opacity, float* grad_l, float* grad_depth, float* grad_background, void* ws,
                             size_t ws_bytes, void* stream) {
  DepthArgs da{};
  da.z = depth; da.bg = background; da.grad_depth = grad_depth_map; da.grad_alpha = grad_alpha_map;
  return blend_backward(start_xy, end_xy, mean_xy, vinv, opacity, l_d, n_gauss, width, height, tile_off, n_tile_pairs, tile_start,
                        tile_list, t_ckpt, grad_image, grad_mean, grad_vinv, grad_opacity, grad_l, grad_depth, grad_background, &da,
                        ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"