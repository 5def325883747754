// gcp_distort.hip — the depth distortion of one camera (the distortion loss of Mip-NeRF 360, 2DGS, gsplat's distloss): per
// pixel a sum over PAIRS of layers, so it is formed where the weights are, in the tile walk, and cannot be built from the
// colour, depth and alpha maps.
//
//   Per pixel p, over its kept pairs k = 1..n front to back — the pair rule is k_blend_fwd's to the letter: inside the integer
//   box clamped to the frame, w_k = T_k o_k g_k, and a pair whose inclusive product T_k (1 - o_k g_k) is exactly 0 is dropped
//   (w = 0, no gradient) — with z_k the per-Gaussian depth the blend takes, A_k = sum_{j<=k} w_j, B_k = sum_{j<=k} w_j z_j:
//     dist(p) = 2 sum_k w_k (z_k A_{k-1} - B_{k-1})        ( = sum_{i>j} 2 w_i w_j (z_i - z_j) )
//   the order-based form: equal to sum_{i,j} w_i w_j |z_i - z_j| whenever z is non-decreasing in list order, as the camera
//   depth is (the list is sorted by it; ties contribute 0).  Not divided by alpha, in units of z, like the depth map.
//   Backward, G = dL/d dist(p), SA_k = sum_{j>=k} w_j (inclusive suffix sum), s_k = sum_j w_j |z_k - z_j|:
//     c_k = 2 G s_k  (= G d dist / d w_k),    dL/dz_k = 2 G w_k (A_n - 2 SA_k + w_k)
//   and the rest is the blend backward's own recursion with this c_k (walk_back, gcp_blend_shared.hpp): R = 0 behind the list,
//   R_{k-1} = R_k + a_k (c_k - R_k), dL/do_k = T_k g_k (c_k - R_k), common = T_k a_k (c_k - R_k).  It is linear in c: these
//   gradients ADD to those of the image, depth and alpha maps.
//   A_n is not the alpha map (behind an exactly opaque layer alpha = 1, A_n is the sum in front of the dropped pair).
//   In float32 neither kernel forms these expressions as written: z_k A - B is a difference of two numbers of size z A whose
//   value has size dz A, and a surface 1e-2 thick at depth 20 — where the regulariser works — lost three digits with them
//   (profiles/r23_blend_rows.md).  A reference depth per tile does not cure it: z - z_ref is itself rounded when z_ref is far,
//   and a pixel's own layers can lie much closer together than the tile's.  Both kernels therefore carry
//     s(z) = sum_j w_j |z - z_j|   along the pixel's own contributing pairs by DIFFERENCES OF NEIGHBOURING DEPTHS only:
//   forward   D_k = sum_{j<k} w_j (z_k - z_j) = D_k' + (z_k - z_k') A_{k-1}, k' the pixel's contributing pair in front of k: for
//             depths in list order a sum of terms of one sign;  dist = 2 sum_k w_k D_k.  It leaves A_n and, as b_n, D_L of the
//             pixel's LAST contributing pair L (= s(z_L): nothing lies behind L).
//   backward  from s_L = b_n, walking back: s_k = s_k' + (z_k' - z_k) (2 SA_k' - A_n), k' the contributing pair behind k and
//             SA_k' the inclusive suffix sum of w (s is piecewise linear in z with slope A_front - A_behind);
//             c_k = 2 G s_k,  dL/dz_k = 2 G w_k (A_n - 2 SA_k + w_k).
//   Forward and backward each decide which pair is the pixel's last contributing one, by w != 0 on weights that are not the
//   same bits (T from the product / from the quotient or slow branch, another association of the exponent).  Where they
//   disagree, s is off by the SAME (z_k - z_L) A_n on every entry of that pixel.  A constant added to every c_j leaves
//   c_k - R_k = (c_k - sum of the convex weights behind k) unchanged but for the weight T_N-behind-L / T_{k+1} of the empty
//   suffix: harmless wherever the weight vanished because T underflowed (that factor is then ~0).  It would cost accuracy
//   only where a weight underflows at a T_N that is not negligible, i.e. g ~ 1e-38 inside a box that is otherwise visible.
//   Everything is in units of the spread of the pixel's own layers, whatever the offset.  b_n is per-pixel state for the
//   backward of the same bins and depths, not sum w z.
//
//   k_distort_fwd     one 256-thread block per 16x16 tile, one pixel per lane, the list front to back as k_contrib_tile walks it
//                     (256 entries staged at a time, the per-wave hit words, the wave-uniform exit behind an exact zero, the
//                     forward blend's association and contraction: w is the weight the image was painted with), the record
//                     with z instead of colour.  Writes dist, A_n, b_n = D_L; no checkpoints (the backward takes those of the render's
//                     own forward on the same bins).
//   k_distort_bwd     on walk_pixel / walk_back; c_k comes from the lane's s, SA, A_n, G through walk_back's hook.  Per
//                     entry five 16-lane row sums (T g d, z term, w d, w d dx, w d dx dx) by the blend's transposed butterfly cut
//                     to five values (12 VALU), into LDS; one thread per entry folds the 16 rows into the entry's Gaussian-major
//                     slot of 7 floats.
//   k_distort_reduce  one thread per Gaussian: the in-order sums of its slots (reduce_slots), expanded into grad_mean,
//                     grad_vinv, grad_opacity, grad_depth as k_grad_reduce does.
// No float atomics: every sum is taken in a fixed order => the same bits on every run.  No read-back: capture-safe.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gcp_blend_shared.hpp"

namespace {
using namespace gcp;

constexpr int kDistVals = 7;      // per (tile, Gaussian) slot: go, S(c dx), S(c dy), S(c dx dx), S(c dx dy), S(c dy dy), gz
constexpr int kDistRowSlots = 5;  // per pixel row in LDS: go, gz, S(c), S(c dx), S(c dx dx)   (dy is constant along a row)

__global__ __launch_bounds__(256) void k_distort_fwd(const BlendArgs a, const float* __restrict__ z, float* __restrict__ dist,
                                                     float* __restrict__ a_n, float* __restrict__ b_n) {
  // the forward blend's arithmetic, contraction included: w here is the weight the image was painted with
#pragma clang fp contract(fast)
  __shared__ StagedZ<kStage> s;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave id in an SGPR
  const int tile = blockIdx.x;
  const int ttx = tile % a.tiles_x, tty = tile / a.tiles_x;
  const int px = ttx * kTile + (lane & 15), py = tty * kTile + w * 4 + (lane >> 4);
  const float fx = (float)px, fy = (float)py;
  const unsigned lane_bits = (1u << (lane & 15)) | (1u << (16 + w * 4 + (lane >> 4)));
  const int first = a.tile_start[tile], last = a.tile_start[tile + 1];
  float T = 1.0f, A = 0.0f, acc = 0.0f;
  float D = 0.0f, zp = 0.0f;  // D_k' and z_k' of the pixel's last contributing pair (zp counts for nothing while A == 0)
  for (int base = first; base < last; base += kStage) {
    const int cnt = __builtin_amdgcn_readfirstlane(min(kStage, last - base));  // scalar loop bound
    __syncthreads();
    stage_entries<false, false>(a, s, base, cnt, ttx * kTile, tty * kTile, z);
    __syncthreads();
    const int chunks = (cnt + 63) >> 6;
    for (int c = 0; c < chunks; ++c) {
      unsigned long long hits = uniform64(s.hits[w][c]);
      // wave-uniform: every pixel of the strip is behind an exact zero — every further w is exactly 0
      if (__ballot(T != 0.0f) == 0ull) hits = 0ull;
      while (hits) {
        const int k = c * 64 + __builtin_ctzll(hits);
        hits &= hits - 1ull;
        const float4 ge = s.geo[k], vi = s.vin[k];
        const float zk = s.z[k];
        if ((__float_as_uint(ge.w) & lane_bits) == lane_bits) {
          const float dx = fx - ge.x, dy = fy - ge.y;
          const float t0 = dx * vi.x + dy * vi.z;  // (d Λ) d^T with the forward blend's association
          const float t1 = dx * vi.y + dy * vi.w;
          const float g = __builtin_amdgcn_exp2f(t0 * dx + t1 * dy);
          const float incl = T * (1.0f - ge.z * g);  // inclusive product
          if (incl != 0.0f) {                        // dropped when exactly 0
            const float wgt = T * ge.z * g;
            if (wgt != 0.0f) {                       // (a kept pair whose weight underflowed contributes nothing and moves nothing)
              D += (zk - zp) * A;                    // D_k = z_k A_{k-1} - B_{k-1}, by neighbouring differences
              zp = zk;
              acc += wgt * D;
              A += wgt;
            }
          }
          T = incl;
        }
      }
    }
  }
  if (px <= a.W && py <= a.H) {
    const i64 o = (i64)py * (a.W + 1) + px;
    dist[o] = 2.0f * acc;
    a_n[o] = A;
    b_n[o] = D;  // D_L
  }
}

// what walk_back asks per entry: c_k = 2 G s_k, s carried from the pixel's last contributing pair back to front; it keeps the z
// term for the body
struct DistHook {
  static constexpr bool kOn = true;
  float SA = 0.0f;             // inclusive suffix sum of w over the entries handled so far
  float s_ = 0.0f, zp = 0.0f;  // s and z of the contributing pair behind the entry in hand; s starts as the forward's b_n = s_L
  float A_N = 0.0f, G2 = 0.0f; // the forward's A_n and 2 dL/d dist of the pixel; 0 outside the frame
  float zt = 0.0f;             // dL/dz_k of this pixel for the entry in hand
  template <class S>
  __device__ __forceinline__ float c(const S& s, int k, float wk) {
#pragma clang fp contract(fast)
    const float z = s.z[k];
    if (wk != 0.0f) {          // an entry without weight contributes nothing and its c_k is not used: s stays where it is
      const float dz = (SA == 0.0f) ? 0.0f : zp - z;  // nothing behind the last contributing pair: s_L as the forward left it
      s_ += dz * (2.0f * SA - A_N);
      zp = z;
      SA += wk;
    }
    zt = G2 * wk * (A_N - 2.0f * SA + wk);
    return G2 * s_;
  }
};

__global__ __launch_bounds__(256) void k_distort_bwd(const BlendArgs a, const float* __restrict__ z, const int* __restrict__ tile_off,
                                                     const float* __restrict__ t_ckpt, const float* __restrict__ a_n,
                                                     const float* __restrict__ b_n, const float* __restrict__ grad_dist,
                                                     i64 n_slots, float* __restrict__ partial /*[K][kDistVals]*/) {
#pragma clang fp contract(fast)  // the backward's arithmetic, contraction included
  __shared__ StagedZ<kStageBwd> s;
  // [entry][pixel row of the tile * kDistRowSlots + value]; the stride is odd: the fold reads with one thread per entry
  constexpr int kPartStride = 16 * kDistRowSlots + 1;
  __shared__ float s_part[kStageBwd][kPartStride];
  DepthArgs da{};
  da.z = z;
  const WalkPixel p = walk_pixel<false, false>(a, t_ckpt, nullptr, da);
  const int lane = p.lane;
  DistHook hook;
  if (p.px <= a.W && p.py <= a.H) {
    const i64 o = (i64)p.py * (a.W + 1) + p.px;
    hook.A_N = a_n[o];
    hook.s_ = b_n[o];
    hook.G2 = 2.0f * grad_dist[o];
  }
  const bool b1 = lane & 2;
  // after the butterfly lane i holds the row sum of value: bit 1 set: 4; else (bit 2 ? 2 : 0) + (bit 3 ? 1 : 0)
  float* const row_slot = &s_part[0][(p.w * 4 + (lane >> 4)) * kDistRowSlots + ((lane & 2) ? 4 : ((lane & 4) ? 2 : 0) + ((lane & 8) ? 1 : 0))];
  walk_back<false>(
      a, da, s, p,
      [&](int k, float op, float dx, float /*dy*/, float tg, float d) {
        float r_o = tg * d;
        float r_c = (tg * op) * d;  // T o g (c - R): "common"
        float r_cx = r_c * dx;
        float r_xx = r_cx * dx;
        float r_z = hook.zt;
        // Five 16-lane row sums by the blend backward's transposed butterfly, cut to five values: partners 15-i, 7-i (within
        // each half), i^2, i^1; the first two steps split the lanes by DPP bank (no select), the third needs one.
        // 5 + 3 + 3 + 1 = 12 VALU instead of 5 x 4.
        float q0, q1, q2, p0, p1;
        // s_nop 1: a DPP source written by the preceding VALU instruction needs two wait states
        asm volatile(
            "s_nop 1\n\t"
            "v_add_f32_dpp %0, %3, %3 row_mirror row_mask:0xf bank_mask:0x3\n\t"  // lanes 0-7 : go
            "v_add_f32_dpp %1, %5, %5 row_mirror row_mask:0xf bank_mask:0x3\n\t"  //             S(c)
            "v_add_f32_dpp %2, %7, %7 row_mirror row_mask:0xf bank_mask:0xf\n\t"  // all lanes : S(c dx dx)
            "v_add_f32_dpp %0, %4, %4 row_mirror row_mask:0xf bank_mask:0xc\n\t"  // lanes 8-15: gz
            "v_add_f32_dpp %1, %6, %6 row_mirror row_mask:0xf bank_mask:0xc\n\t"  //             S(c dx)
            : "=&v"(q0), "=&v"(q1), "=&v"(q2)
            : "v"(r_o), "v"(r_z), "v"(r_c), "v"(r_cx), "v"(r_xx));
        asm volatile(
            "s_nop 1\n\t"
            "v_add_f32_dpp %0, %2, %2 row_half_mirror row_mask:0xf bank_mask:0x5\n\t"  // bit 2 clear: from q0
            "v_add_f32_dpp %1, %4, %4 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"  // all lanes  : from q2
            "v_add_f32_dpp %0, %3, %3 row_half_mirror row_mask:0xf bank_mask:0xa\n\t"  // bit 2 set  : from q1
            : "=&v"(p0), "=&v"(p1)
            : "v"(q0), "v"(q1), "v"(q2));
        // lanes with bit 1 clear keep p0 and add the partner's (i^2) copy; the others p1
        const float keep = b1 ? p1 : p0, send = b1 ? p0 : p1;
        const float o0 = keep + dpp_f<0x4e, 0xf>(0.0f, send);
        const float tot = o0 + dpp_f<0xb1, 0xf>(0.0f, o0);
        row_slot[k * kPartStride] = tot;  // lanes that hold the same value store the same word
      },
      [&](unsigned hits) {
        for (unsigned hz = hits; hz; hz &= hz - 1) row_slot[__builtin_ctz(hz) * kPartStride] = 0.0f;
      },
      [&](int j, int entry) {
        // add the 16 pixel rows in fixed order
        const i64 e = entry_slot(a, tile_off, entry, s.box[j], p.ttx, p.tty);
        const float my = s.geo[j].y;
        float go = 0.0f, cx = 0.0f, cy = 0.0f, xx = 0.0f, xy = 0.0f, yy = 0.0f, zz = 0.0f;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) {
          if (!((s.hits[wv][0] >> j) & 1ull)) continue;  // that wave never wrote its rows for this entry
#pragma unroll
          for (int r = 4 * wv; r < 4 * wv + 4; ++r) {
            const float* d = &s_part[j][r * kDistRowSlots];
            const float dy = (float)(p.tty * kTile + r) - my;  // constant along the pixel row
            go += d[0]; zz += d[1];
            cx += d[3]; cy += dy * d[2];
            xx += d[4]; xy += dy * d[3]; yy += dy * dy * d[2];
          }
        }
        if (e >= 0 && e < n_slots) {  // (a listed entry always is: the binning lists whole Gaussians)
          float* out = partial + e * kDistVals;
          out[0] = go; out[1] = cx; out[2] = cy; out[3] = xx; out[4] = xy; out[5] = yy; out[6] = zz;
        }
      },
      hook);
}

// per Gaussian: sum its tile slots in order (reduce_slots), expand the moments into the four gradients as k_grad_reduce does
__global__ __launch_bounds__(256) void k_distort_reduce(const float* __restrict__ partial, const int* __restrict__ tile_off,
                                                        const int* __restrict__ tile_start, int n_tiles, const float* __restrict__ vinv,
                                                        i64 n, i64 capacity, float* __restrict__ grad_mean, float* __restrict__ grad_vinv,
                                                        float* __restrict__ grad_opacity, float* __restrict__ grad_z) {
  const i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const SlotSums<kDistVals> sums = reduce_slots<SlotSums<kDistVals>>(partial, tile_off, tile_start, n_tiles, g, n, capacity);
  const float* r = sums.v;
  if (g >= n) return;
  const float A = vinv[4 * g], B = vinv[4 * g + 1], C = vinv[4 * g + 2], D = vinv[4 * g + 3];
  grad_opacity[g] = r[0];
  // sum common * (d Λ): x0 = dx a + dy c, x1 = dx b + dy d
  grad_mean[2 * g] = r[1] * A + r[2] * C;
  grad_mean[2 * g + 1] = r[1] * B + r[2] * D;
  // -0.5 * sum common * d^T d
  grad_vinv[4 * g] = -0.5f * r[3];
  grad_vinv[4 * g + 1] = -0.5f * r[4];
  grad_vinv[4 * g + 2] = -0.5f * r[4];
  grad_vinv[4 * g + 3] = -0.5f * r[5];
  grad_z[g] = r[6];
}

}  // namespace

extern "C" {

int gcp_blend_distort_forward(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv,
                              const float* opacity, const float* depth, int64_t n_gauss, int32_t width, int32_t height,
                              const int32_t* tile_start, const int32_t* tile_list, float* dist_map, float* a_n, float* b_n,
                              void* stream) {
  if (n_gauss < 0 || width < 0 || height < 0 || !dist_map || !a_n || !b_n) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss > 0 && (!start_xy || !end_xy || !mean_xy || !vinv || !opacity || !depth || !tile_start || !tile_list))
    return GCP_ERR_INVALID_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
  if (n_gauss == 0) {  // nothing to walk: the maps are zero
    const size_t bytes = (size_t)(width + 1) * (size_t)(height + 1) * sizeof(float);
    GCP_HIP(hipMemsetAsync(dist_map, 0, bytes, st));
    GCP_HIP(hipMemsetAsync(a_n, 0, bytes, st));
    GCP_HIP(hipMemsetAsync(b_n, 0, bytes, st));
    return GCP_OK;
  }
  BlendArgs a;
  if (make_args(a, start_xy, end_xy, mean_xy, vinv, opacity, nullptr, width, height, tile_start, tile_list) != GCP_OK)
    return GCP_ERR_INVALID_ARGUMENT;
  const TileGrid tg = tile_grid(width, height);
  hipLaunchKernelGGL(k_distort_fwd, dim3((unsigned)(tg.tx * tg.ty)), dim3(256), 0, st, a, depth, dist_map, a_n, b_n);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

size_t gcp_blend_distort_backward_workspace_bytes(int64_t n_tile_pairs) {
  return align256((size_t)(n_tile_pairs > 0 ? n_tile_pairs : 1) * kDistVals * sizeof(float));  // per-entry partial sums
}

int gcp_blend_distort_backward(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv,
                               const float* opacity, const float* depth, int64_t n_gauss, int32_t width, int32_t height,
                               const int32_t* tile_off, int64_t n_tile_pairs, const int32_t* tile_start,
                               const int32_t* tile_list, const float* t_ckpt, const float* a_n, const float* b_n,
                               const float* grad_dist, float* grad_mean, float* grad_vinv, float* grad_opacity,
                               float* grad_depth, void* ws, size_t ws_bytes, void* stream) {
  if (n_gauss < 0 || n_tile_pairs < 0 || width < 0 || height < 0 || n_tile_pairs > 0x7fffffffLL) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0) return GCP_OK;
  if (!start_xy || !end_xy || !mean_xy || !vinv || !opacity || !depth || !tile_off || !tile_start || !t_ckpt || !a_n || !b_n ||
      !grad_dist || !grad_mean || !grad_vinv || !grad_opacity || !grad_depth || !ws || (n_tile_pairs > 0 && !tile_list))
    return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < gcp_blend_distort_backward_workspace_bytes(n_tile_pairs)) return GCP_ERR_WORKSPACE;
  BlendArgs a;
  if (make_args(a, start_xy, end_xy, mean_xy, vinv, opacity, nullptr, width, height, tile_start, tile_list) != GCP_OK)
    return GCP_ERR_INVALID_ARGUMENT;
  const TileGrid tg = tile_grid(width, height);
  const int n_tiles = tg.tx * tg.ty;
  const dim3 tiles((unsigned)n_tiles), gauss((unsigned)((n_gauss + 255) / 256)), block(256);
  float* partial = (float*)ws;
  hipStream_t st = (hipStream_t)stream;
  if (n_tile_pairs > 0) {
    hipLaunchKernelGGL(k_distort_bwd, tiles, block, 0, st, a, depth, tile_off, t_ckpt, a_n, b_n, grad_dist, (i64)n_tile_pairs, partial);
    GCP_HIP(hipGetLastError());
  }
  // without entries nothing is listed below the capacity 0: the reduce writes zeros
  hipLaunchKernelGGL(k_distort_reduce, gauss, block, 0, st, (const float*)partial, tile_off, tile_start, n_tiles, vinv, (i64)n_gauss,
                     (i64)n_tile_pairs, grad_mean, grad_vinv, grad_opacity, grad_depth);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

}  // extern "C"
