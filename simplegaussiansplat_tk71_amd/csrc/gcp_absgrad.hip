// gcp_absgrad.hip — the absolute screen-space gradient of one camera (AbsGS; gsplat's absgrad): per Gaussian the sums, over
// the pixels of its box, of |dL/dmu_x(p)| and |dL/dmu_y(p)|, where the blend backward (gcp_blend.hip) returns the signed sums
// — per-pixel gradients of a large splat that is too bright on one side and too dark on the other cancel there.
//
//   Per splat-pixel pair (k, p) the backward counts:   m(k,p) = T_k o_k g_k (c_k - R_k) Λ_k (p - mu_k)
//   with the terms as blend_bwd_tile forms them: c_k = (dL/dI . l_k) (+ dL/dD z_k), the suffix recursion
//   R_{k-1} = R_k + a_k (c_k - R_k) from R = 0 behind the list (depth variant: dL/dI . bg - dL/dA where T_N != 0), m = 0
//   outside the box clamped to the frame and for a dropped pair (inclusive product exactly 0), and
//   Λ (p - mu) = (A dx + C dy, B dx + D dy) with the raw vinv entries, as grad_reduce expands its moments.
//   grad_mean[k] of the backward is sum_p m(k,p);  absgrad[k] = (sum_p |m_x(k,p)|, sum_p |m_y(k,p)|).
//
//   k_absgrad_tile    one 256-thread block per 16x16 tile, one pixel per lane, the tile's list BACK TO FRONT in chunks of
//                     kStageBwd entries from the forward's transmittance checkpoints, T_k by the backward's own rule (the
//                     quotient T_{k+1} / (1 - a_k); front to back from the chunk's start checkpoint where a pixel of the strip
//                     underflows in the chunk; nothing at all where every pixel enters the chunk behind an exact zero) — so the
//                     pair set and T_k are the backward's.  Per entry two 16-lane row sums (DPP), parked in LDS at
//                     [entry][pixel row][2]; after every chunk one thread per entry adds the rows in fixed order into the
//                     entry's Gaussian-major slot (the slot k_blend_bwd writes its partial sums to), 2 floats per slot.
//   k_absgrad_reduce  one thread per Gaussian: the in-order sums of its slots; a Gaussian with 128 slots or more is taken by
//                     its whole wave, as in k_grad_reduce.
// No float atomics: every sum is taken in a fixed order => the same bits on every run.
// gcp_blend.hip is not touched: the staging record and the front-to-back factor are copied here (the record also carries the
// raw Λ, and the parked values are two per row instead of eight).

#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>

#include "gcp_tiles.hpp"

namespace {
using namespace gcp;

constexpr int kStageBwd = 32;     // entries per chunk = the forward's checkpoint interval (gcp_blend.hip: kStageBwd == kCkpt)
constexpr int kCkpt = kStageBwd;
constexpr int kReduceWide = 128;  // tile slots from which a Gaussian is summed by the wave

// sum over each 16-lane DPP row (= one pixel row of the tile); valid in lanes 15, 31, 47, 63
__device__ __forceinline__ float row_sum16(float v) {
  v += dpp_f<0x111, 0xf>(0.0f, v);
  v += dpp_f<0x112, 0xf>(0.0f, v);
  v += dpp_f<0x114, 0xf>(0.0f, v);
  v += dpp_f<0x118, 0xf>(0.0f, v);
  return v;
}

struct AbsDepthArgs {
  const float* z;           // [N] camera-space depth of every Gaussian
  const float* bg;          // float[3] background colour, or nullptr (black)
  const float* grad_depth;  // dL/d(depth map), or nullptr (zero)
  const float* grad_alpha;  // dL/d(alpha map), or nullptr (zero)
};

struct AbsStaged {
  int4 box[kStageBwd];    // x0, y0, x1-x0, y1-y0 (clamped to the image)
  float4 geo[kStageBwd];  // mx, my, opacity, box mask as bits (0-15: tile columns inside the box, 16-31: tile rows)
  float4 vin[kStageBwd];  // Λ' = -0.5*log2(e) * Λ as a, b + c, d, - (the backward's form)
  float4 col[kStageBwd];  // l0 l1 l2, z (depth variant; 0 otherwise)
  float4 raw[kStageBwd];  // Λ itself: A B C D
  unsigned long long hits[4];  // hits[w]: bit j set = staged entry j reaches into the four pixel rows of wave w
};

template <bool DEPTH>
__device__ __forceinline__ void stage_abs(const BlendArgs& a, AbsStaged& s, int first, int cnt, int tile_x0, int tile_y0, const float* z) {
  for (int j = threadIdx.x; j < cnt; j += blockDim.x) {  // cnt <= 32: part of wave 0
    const i64 g = a.tile_list[first + j];
    Box b;
    load_box(a.start, a.end, g, a.W, a.H, b);
    s.box[j] = make_int4(b.x0, b.y0, b.x1 - b.x0, b.y1 - b.y0);
    const int c0 = max(b.x0 - tile_x0, 0), c1 = min(b.x1 - tile_x0, kTile - 1);
    const int r0 = max(b.y0 - tile_y0, 0), r1 = min(b.y1 - tile_y0, kTile - 1);
    const unsigned cm = (c1 >= c0) ? ((2u << c1) - (1u << c0)) : 0u;
    const unsigned rm = (r1 >= r0) ? ((2u << r1) - (1u << r0)) : 0u;
#pragma unroll
    for (int w2 = 0; w2 < 4; ++w2) {
      const unsigned long long touched = __ballot(((rm >> (4 * w2)) & 0xfu) != 0u);
      if ((threadIdx.x & 63) == 0) s.hits[w2] = touched;
    }
    s.geo[j] = make_float4(a.mean[2 * g], a.mean[2 * g + 1], a.opacity[g], __uint_as_float(cm | (rm << 16)));
    constexpr float kS = -0.5f * 1.44269504088896341f;  // the backward's pre-scaling, product by product
    const float A = a.vinv[4 * g], B = a.vinv[4 * g + 1], C = a.vinv[4 * g + 2], D = a.vinv[4 * g + 3];
    s.vin[j] = make_float4(kS * A, kS * B + kS * C, kS * D, 0.0f);
    s.raw[j] = make_float4(A, B, C, D);
    s.col[j] = make_float4(a.l_d[3 * g], a.l_d[3 * g + 1], a.l_d[3 * g + 2], DEPTH ? z[g] : 0.0f);
  }
}

__device__ __forceinline__ i64 ckpt_slot0(int first, int tile) { return (i64)(first / kCkpt) + 2 * (i64)tile; }

// T behind staged entry j for this lane's pixel, given T in front of it (gcp_blend.hip: slow_factor)
__device__ __forceinline__ float slow_factor(const AbsStaged& s, int j, float fx, float fy, unsigned lane_bits, float T) {
  const float4 gj = s.geo[j];
  const float4 vj = s.vin[j];
  const float dxj = fx - gj.x, dyj = fy - gj.y;
  const float g_j = __builtin_amdgcn_exp2f(dxj * (vj.x * dxj + vj.y * dyj) + (vj.z * dyj) * dyj);
  return ((__float_as_uint(gj.w) & lane_bits) == lane_bits) ? T * (1.0f - gj.z * g_j) : T;
}

// [entry][pixel row of the tile * 2 + axis]; one word of padding per entry: the fold reads with one thread per entry, and a
// stride of 32 words would put all of them on one LDS bank
constexpr int kPartStride = 16 * 2 + 1;

template <bool DEPTH>
__device__ __forceinline__ void absgrad_tile(const BlendArgs& a, const int* __restrict__ tile_off, const float* __restrict__ t_ckpt,
                                             const float* __restrict__ grad_image, i64 n_slots, float2* __restrict__ slot,
                                             const AbsDepthArgs& da) {
#pragma clang fp contract(fast)  // the backward's arithmetic, contraction included: T_k and the pair set are its own
  __shared__ AbsStaged s;
  __shared__ float s_part[kStageBwd][kPartStride];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave id in an SGPR
  const int tile = blockIdx.x;
  const int ttx = tile % a.tiles_x, tty = tile / a.tiles_x;
  const int px = ttx * kTile + (lane & 15);
  const int py = tty * kTile + w * 4 + (lane >> 4);
  const float fx = (float)px, fy = (float)py;
  const int first = a.tile_start[tile], last = a.tile_start[tile + 1];
  float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
  if (px <= a.W && py <= a.H) {
    const i64 o = ((i64)py * (a.W + 1) + px) * 3;
    g0 = grad_image[o]; g1 = grad_image[o + 1]; g2 = grad_image[o + 2];
  }
  const unsigned lane_bits = (1u << (lane & 15)) | (1u << (16 + w * 4 + (lane >> 4)));
  float* const row_slot = &s_part[0][(w * 4 + (lane >> 4)) * 2];
  const float* const ck = t_ckpt + ckpt_slot0(first, tile) * 256 + threadIdx.x;
  const int nchunks = (last - first + kStageBwd - 1) / kStageBwd;
  float R = 0.0f;   // R_k of the deepest entry handled so far (the suffix behind the end of the list is empty)
  float gz = 0.0f;  // dL/dD of this pixel (depth variant)
  if (DEPTH) {
    if (nchunks == 0) return;  // (block-uniform)
    const float T_N = ck[(i64)nchunks * 256];
    float ga = 0.0f;
    if (px <= a.W && py <= a.H) {
      const i64 p = (i64)py * (a.W + 1) + px;
      if (da.grad_depth) gz = da.grad_depth[p];
      if (da.grad_alpha) ga = da.grad_alpha[p];
    }
    const float cb = da.bg ? g0 * da.bg[0] + g1 * da.bg[1] + g2 * da.bg[2] : 0.0f;
    R = (T_N != 0.0f) ? cb - ga : 0.0f;  // the absorbing layer behind the list
  }
  for (int q = nchunks - 1; q >= 0; --q) {
    const int base = first + q * kStageBwd;
    const int cnt = __builtin_amdgcn_readfirstlane(min(kStageBwd, last - base));  // scalar loop bound
    const float T_end = ck[(i64)(q + 1) * 256];
    const float T_start = (q > 0) ? ck[(i64)q * 256] : 1.0f;
    __syncthreads();
    stage_abs<DEPTH>(a, s, base, cnt, ttx * kTile, tty * kTile, da.z);
    __syncthreads();
    // only the entries whose rows reach this wave, deepest first (the fold skips this wave's rows for the others)
    const unsigned hits = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)s.hits[w]);
    // wave-uniform: some pixel of the strip underflows inside this chunk — quotients cannot be trusted for it
    const bool slow = __ballot(T_end < 1.17549435e-38f && T_start != 0.0f) != 0ull;
    float Tn = T_end;  // transmittance behind the entry in hand
    float T_group = T_start;
    int slow_group = -1;
    auto walk_chunk = [&](auto slow_tag) {
      constexpr bool kSlow = decltype(slow_tag)::value;
      unsigned h = hits;
      while (h) {
        const int k = 31 - __builtin_clz(h);
        h &= ~(1u << k);
        // straight-line for all 64 lanes; lanes outside the box / dropped pairs are zeroed with selects
        const float4 ge = s.geo[k];
        const float4 vi = s.vin[k];
        const float4 co = s.col[k];
        const float4 ra = s.raw[k];
        const bool in = (__float_as_uint(ge.w) & lane_bits) == lane_bits;
        const float dx = fx - ge.x, dy = fy - ge.y;
        const float gv = __builtin_amdgcn_exp2f(dx * (vi.x * dx + vi.y * dy) + (vi.z * dy) * dy);
        const float og = ge.z * gv;
        const float anti = 1.0f - og;
        float Tk, incl;
        if (!kSlow) {
          incl = Tn;  // what the forward pass left behind this pair
          Tk = (Tn == 0.0f) ? 0.0f : Tn * __builtin_amdgcn_rcpf(anti);
        } else {
          // T_k front to back from the chunk's start checkpoint, the product up to the entry's group of eight formed once per
          // group (gcp_blend.hip: blend_bwd_tile)
          const unsigned below_group = (1u << (k & ~7)) - 1u;
          if ((k & ~7) != slow_group) {  // wave-uniform
            slow_group = k & ~7;
            T_group = T_start;
            for (unsigned hh = hits & below_group; hh; hh &= hh - 1) T_group = slow_factor(s, __builtin_ctz(hh), fx, fy, lane_bits, T_group);
          }
          Tk = T_group;
          for (unsigned hh = hits & ((1u << k) - 1u) & ~below_group; hh; hh &= hh - 1) Tk = slow_factor(s, __builtin_ctz(hh), fx, fy, lane_bits, Tk);
          incl = Tk * anti;
        }
        const bool keep = in & (incl != 0.0f);  // dropped when the inclusive product is exactly 0
        Tn = in ? Tk : Tn;
        const float tg = keep ? Tk * gv : 0.0f;
        float c = g0 * co.x + g1 * co.y + g2 * co.z;  // dL/dI . l
        if (DEPTH) c += gz * co.w;                    // + dL/dD z
        const float d = c - R;
        const float r_c = (tg * ge.z) * d;            // T o g (c - R): the backward's "common" factor
        R = keep ? R + og * d : R;                    // R_{k-1} = R_k + a_k (c_k - R_k)
        const float ax = row_sum16(fabsf(r_c * (ra.x * dx + ra.z * dy)));  // |m_x|: Λ (p - mu) with the raw entries
        const float ay = row_sum16(fabsf(r_c * (ra.y * dx + ra.w * dy)));  // |m_y|
        if ((lane & 15) == 15) {
          row_slot[k * kPartStride] = ax;
          row_slot[k * kPartStride + 1] = ay;
        }
      }
    };
    if (__ballot(T_start != 0.0f) == 0ull) {
      // every pixel of the strip enters the chunk behind an exact zero: T_k = 0 throughout, every term is 0 and R does not move
      if ((lane & 15) == 15)
        for (unsigned hz = hits; hz; hz &= hz - 1) {
          row_slot[__builtin_ctz(hz) * kPartStride] = 0.0f;
          row_slot[__builtin_ctz(hz) * kPartStride + 1] = 0.0f;
        }
    } else if (slow) {
      walk_chunk(std::true_type{});
    } else {
      walk_chunk(std::false_type{});
    }
    __syncthreads();
    // one thread per entry: add the 16 pixel rows in fixed order, write the entry's Gaussian-major slot
    for (int j = threadIdx.x; j < cnt; j += 256) {
      const i64 g = a.tile_list[base + j];
      const int4 bx = s.box[j];
      const int ntx = ((bx.x + bx.z) >> 4) - (bx.x >> 4) + 1;
      const i64 e = (i64)tile_off[g] + (i64)(tty - (bx.y >> 4)) * ntx + (ttx - (bx.x >> 4));
      float sx = 0.0f, sy = 0.0f;
#pragma unroll
      for (int wv = 0; wv < 4; ++wv) {
        if (!((s.hits[wv] >> j) & 1ull)) continue;  // that wave never wrote its rows for this entry
#pragma unroll
        for (int r = 4 * wv; r < 4 * wv + 4; ++r) {
          sx += s_part[j][2 * r];
          sy += s_part[j][2 * r + 1];
        }
      }
      if (e >= 0 && e < n_slots) slot[e] = make_float2(sx, sy);  // (a listed entry always is: the binning lists whole Gaussians)
    }
  }
}

__global__ __launch_bounds__(256) void k_absgrad_tile(const BlendArgs a, const int* __restrict__ tile_off,
                                                      const float* __restrict__ t_ckpt, const float* __restrict__ grad_image,
                                                      i64 n_slots, float2* __restrict__ slot) {
  absgrad_tile<false>(a, tile_off, t_ckpt, grad_image, n_slots, slot, AbsDepthArgs{});
}

__global__ __launch_bounds__(256) void k_absgrad_tile_depth(const BlendArgs a, const AbsDepthArgs da, const int* __restrict__ tile_off,
                                                            const float* __restrict__ t_ckpt, const float* __restrict__ grad_image,
                                                            i64 n_slots, float2* __restrict__ slot) {
  absgrad_tile<true>(a, tile_off, t_ckpt, grad_image, n_slots, slot, da);
}

// per Gaussian: the in-order sums of its tile slots.  Only slots k_absgrad_tile wrote are read — the rule of k_grad_reduce
// (gcp_blend.hip): a Gaussian's entries [tile_off[g], tile_off[g+1]) count iff they lie inside what the binning LISTED
// (tile_start[n_tiles] entries, at most the capacity); offsets that wrapped or are inverted give zeros.  A Gaussian with
// kReduceWide slots or more is taken by its whole wave: lane l adds slots e0 + l, e0 + l + 64, ... in order and the 64 partial
// sums meet in a fixed butterfly.  Which Gaussians go that way depends on their slot count alone.
__global__ __launch_bounds__(256) void k_absgrad_reduce(const float2* __restrict__ slot, const int* __restrict__ tile_off,
                                                        const int* __restrict__ tile_start, int n_tiles, i64 n, i64 capacity,
                                                        float* __restrict__ absgrad /*[n][2]*/) {
  const i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const i64 listed = min((i64)tile_start[n_tiles], capacity);
  i64 e0 = 0, e1 = 0;
  if (g < n) {
    e0 = tile_off[g];
    e1 = tile_off[g + 1];
    if (e0 < 0 || e1 < e0 || e1 > listed) e1 = e0 < 0 ? 0 : e0;
    if (e0 < 0) e0 = 0;
  }
  float sx = 0.0f, sy = 0.0f;
  const bool wide = e1 - e0 >= kReduceWide;
  if (!wide) {
    for (i64 e = e0; e < e1; ++e) {
      const float2 p = slot[e];
      sx += p.x;
      sy += p.y;
    }
  }
  for (unsigned long long todo = __ballot(wide); todo; todo &= todo - 1ull) {  // wave-uniform: one wide Gaussian at a time
    const int owner = __builtin_ctzll(todo);
    const i64 f0 = (i64)__builtin_amdgcn_readlane((int)e0, owner), f1 = (i64)__builtin_amdgcn_readlane((int)e1, owner);  // (entries < 2^31)
    float px = 0.0f, py = 0.0f;
    for (i64 e = f0 + lane; e < f1; e += 64) {
      const float2 p = slot[e];
      px += p.x;
      py += p.y;
    }
    for (int o = 32; o > 0; o >>= 1) {  // a fixed butterfly: every lane ends with the same pair
      px += __shfl_xor(px, o);
      py += __shfl_xor(py, o);
    }
    if (lane == owner) { sx = px; sy = py; }
  }
  if (g >= n) return;
  absgrad[2 * g] = sx;
  absgrad[2 * g + 1] = sy;
}

int blend_absgrad(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv, const float* opacity,
                  const float* l_d, int64_t n_gauss, int32_t width, int32_t height, const int32_t* tile_off, int64_t n_tile_pairs,
                  const int32_t* tile_start, const int32_t* tile_list, const float* t_ckpt, const float* grad_image, float* absgrad,
                  const AbsDepthArgs* da, void* ws, size_t ws_bytes, hipStream_t stream) {
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
  AbsDepthArgs da{};
  da.z = depth; da.bg = background; da.grad_depth = grad_depth_map; da.grad_alpha = grad_alpha_map;
  return blend_absgrad(start_xy, end_xy, mean_xy, vinv, opacity, l_d, n_gauss, width, height, tile_off, n_tile_pairs, tile_start,
                       tile_list, t_ckpt, grad_image, absgrad, &da, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
