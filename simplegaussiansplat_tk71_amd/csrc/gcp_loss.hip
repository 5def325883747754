// gcp_loss.hip — the training loss of the caller, fused.
//
// reference: gs_control.py:180-182
//     loss = (1 - lambda) * l1_loss(images, targets) + lambda * (1 - kornia.metrics.ssim(images, targets, 11).mean())
// As PyTorch ops that is five depthwise 11x11 Gaussian blurs per direction and ~40 element-wise kernels over the
// image batch: 6.3 ms forward + backward for one 1920x1080 frame, against 3 ms for projection + rasterisation.
// Here: one kernel per direction.  A 256-thread block owns a 32x16 pixel tile of one (image, channel) plane, stages
// the tile plus a 5-pixel halo in LDS (reflect padding, as kornia's filter2d), blurs separably (rows, then columns)
// and keeps everything else in registers.
//   forward : sum of the SSIM map and sum of |a - b| per block (deterministic: no atomics; the host adds the block
//             sums) and, for backward, the three maps dm/dmu1, dm/dE[a^2], dm/dE[ab];
//   backward: dL/da = s_ssim * (blur^T(dm/dmu1) + 2a blur^T(dm/dE11) + b blur^T(dm/dE12)) + s_l1 * sign(a - b),
//             with blur^T the exact adjoint of the reflect-padded blur (border pixels collect the mirrored taps).
// HBM bound: forward reads 8 B and writes 12 B per pixel-channel, backward reads 20 B and writes 4 B.
// The four forward kernels (loss / evaluation metrics, each plain or with a per-camera exposure) are instantiations of
// one body, ssim_tile; the two backward kernels share the staging of the maps and both passes of the adjoint blur.
#include "gcp_device.hpp"
#include "grouped_cumprod_hip.h"

namespace {

using gcp::i64;

constexpr int kTW = 32, kTH = 16, kR = 5, kTaps = 2 * kR + 1;
constexpr int kHW = kTW + 2 * kR, kHH = kTH + 2 * kR;  // 42 x 26 halo tile
constexpr int kThreads = 256;

struct Window {
  float w[kTaps];
};

__device__ __forceinline__ int reflect(int u, int n) { return u < 0 ? -u : (u >= n ? 2 * (n - 1) - u : u); }

__device__ __forceinline__ float block_sum(float v, float* s_red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// Three block sums behind one barrier, each with the association of block_sum; s_red: float[3][4].
__device__ __forceinline__ void block_sum3(float& a, float& b, float& c, float (*s_red)[4]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64), b += __shfl_down(b, off, 64), c += __shfl_down(c, off, 64);
  }
  if ((threadIdx.x & 63) == 0) s_red[0][threadIdx.x >> 6] = a, s_red[1][threadIdx.x >> 6] = b, s_red[2][threadIdx.x >> 6] = c;
  __syncthreads();
  a = (s_red[0][0] + s_red[0][1]) + (s_red[0][2] + s_red[0][3]);
  b = (s_red[1][0] + s_red[1][1]) + (s_red[1][2] + s_red[1][3]);
  c = (s_red[2][0] + s_red[2][1]) + (s_red[2][2] + s_red[2][3]);
}

// ---- per-camera exposure compensation -------------------------------------------------------------------
// One learned 3 x 4 colour affine per image, applied to the render before the loss: y_c = E[c][0] x_0 + E[c][1] x_1 +
// E[c][2] x_2 + E[c][3].  y is never written to memory: it is formed as the tile is staged (reflect padding commutes with a
// pointwise map), and the backward forms it again from x.

// THE compensated value: three fused multiply-adds in this order, wherever y is needed (forward staging, the backward's
// 2 y g1 and sign(y - b), the metrics), so that all of them see the same bits.  Exact for E = [I | 0]: 1 * x_c + 0 + 0 + 0.
__device__ __forceinline__ float exposure_apply(const float* __restrict__ e, float x0, float x1, float x2) {
  return __fmaf_rn(e[0], x0, __fmaf_rn(e[1], x1, __fmaf_rn(e[2], x2, e[3])));
}

// y_c at offset o of an image whose three planes are `stride` floats apart; e: row c of the image's matrix.
__device__ __forceinline__ float exposure_stage(const float* __restrict__ x, i64 stride, i64 o, const float* __restrict__ e) {
  const float x0 = x[o], x1 = x[o + stride], x2 = x[o + 2 * stride];
  return exposure_apply(e, x0, x1, x2);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
// The one body of the four forward kernels: block = plane * tiles + tile (with an exposure plane = 3 * image + c), so the host
// and k_metrics_fold add the block sums in one order whatever the variant.
//   EXPOSURE: y_c is staged in place of img1 (exposure_stage on the image's three planes; row c of the image's matrix at
//             12 image + 4 c = 4 plane).  The two extra channel loads per halo position re-read lines the blocks of the sibling
//             planes fetch too.
//   METRICS : evaluation — no gradient, no maps, three sums per block (the SSIM map, |a - b| and (a - b)^2) at
//             partial[3 * block ..].  clamp: img1 (the render, compensated first; never the photograph) is clamped to [0, 1]
//             as it is staged, so that all three terms see the clamped value (NaN stays NaN).  8 B read per pixel-channel.
//   else    : the loss — two sums per block (the SSIM map, |a - b|) at partial[2 * block ..] and, unless dm_dmu1 is NULL, the
//             three maps for the backward.
template <bool EXPOSURE, bool METRICS>
__device__ __forceinline__ void ssim_tile(const float* __restrict__ img1, const float* __restrict__ img2,
                                          const float* __restrict__ exposure, int height, int width, int tiles_x, int tiles_y,
                                          const Window& win, float c1, float c2, int clamp, float* __restrict__ dm_dmu1,
                                          float* __restrict__ dm_de11, float* __restrict__ dm_de12, float* __restrict__ partial) {
  __shared__ float s_a[kHH][kHW + 1], s_b[kHH][kHW + 1];
  __shared__ float s_h[5][kHH][kTW + 1];
  __shared__ float s_red[METRICS ? 3 : 1][4];
  const int tile = blockIdx.x % (tiles_x * tiles_y), plane = blockIdx.x / (tiles_x * tiles_y);
  const int x0 = (tile % tiles_x) * kTW, y0 = (tile / tiles_x) * kTH;
  const i64 stride = (i64)height * width;
  const float* a = img1 + (i64)(EXPOSURE ? plane / 3 * 3 : plane) * stride;  // with an exposure: the image's first plane
  const float* b = img2 + (i64)plane * stride;
  const float lo = clamp ? 0.f : -__builtin_inff(), hi = clamp ? 1.f : __builtin_inff();
  for (int i = threadIdx.x; i < kHH * kHW; i += kThreads) {
    const int r = i / kHW, c = i % kHW;
    // rows / columns past the image edge of a partial tile are clamped: their results are never used
    const int y = reflect(min(y0 + r - kR, height - 1 + kR), height), x = reflect(min(x0 + c - kR, width - 1 + kR), width);
    const i64 o = (i64)y * width + x;
    float va, vb = b[o];
    if constexpr (EXPOSURE) va = exposure_stage(a, stride, o, exposure + 4 * (i64)plane);  // row c of image i: 12 i + 4 c
    else va = a[o];
    // all loads first, then two selects against uniform bounds (+-inf without the clamp: the identity): a branch on the
    // loaded value would hold the later loads back until the first has returned
    if constexpr (METRICS) va = va < lo ? lo : (va > hi ? hi : va);
    s_a[r][c] = va;
    s_b[r][c] = vb;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kHH * kTW; i += kThreads) {  // blur along the row
    const int r = i / kTW, c = i % kTW;
    float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float va = s_a[r][c + k], vb = s_b[r][c + k], w = win.w[k];
      m1 += w * va, m2 += w * vb, e11 += w * (va * va), e22 += w * (vb * vb), e12 += w * (va * vb);
    }
    s_h[0][r][c] = m1, s_h[1][r][c] = m2, s_h[2][r][c] = e11, s_h[3][r][c] = e22, s_h[4][r][c] = e12;
  }
  __syncthreads();
  float sum_ssim = 0.f, sum_l1 = 0.f, sum_sq = 0.f;
  const int c = threadIdx.x % kTW;
#pragma unroll
  for (int half = 0; half < 2; ++half) {  // blur along the column, two pixels per thread
    const int r = threadIdx.x / kTW + half * (kTH / 2);
    const int x = x0 + c, y = y0 + r;
    float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float w = win.w[k];
      mu1 += w * s_h[0][r + k][c], mu2 += w * s_h[1][r + k][c], e11 += w * s_h[2][r + k][c], e22 += w * s_h[3][r + k][c],
          e12 += w * s_h[4][r + k][c];
    }
    if (x < width && y < height) {
      const float s1 = e11 - mu1 * mu1, s2 = e22 - mu2 * mu2, s12 = e12 - mu1 * mu2;
      const float A = 2.f * mu1 * mu2 + c1, B = 2.f * s12 + c2, C = mu1 * mu1 + mu2 * mu2 + c1, D = s1 + s2 + c2;
      const float den = C * D + 1e-12f, m = A * B / den;
      const float d = s_a[r + kR][c + kR] - s_b[r + kR][c + kR];
      sum_ssim += m;
      sum_l1 += fabsf(d);
      if constexpr (METRICS) {
        sum_sq += d * d;
      } else if (dm_dmu1) {
        const i64 o = ((i64)plane * height + y) * width + x;
        const float m_den = m / den;  // A B / den^2
        dm_dmu1[o] = (2.f * mu2 * (B - A)) / den - m_den * (2.f * mu1 * (D - C));
        dm_de11[o] = -m_den * C;
        dm_de12[o] = 2.f * A / den;
      }
    }
  }
  if constexpr (METRICS) {
    block_sum3(sum_ssim, sum_l1, sum_sq, s_red);
    if (threadIdx.x == 0) {
      float* p = partial + 3 * (i64)blockIdx.x;
      p[0] = sum_ssim, p[1] = sum_l1, p[2] = sum_sq;
    }
  } else {
    const float t_ssim = block_sum(sum_ssim, s_red[0]);
    __syncthreads();
    const float t_l1 = block_sum(sum_l1, s_red[0]);
    if (threadIdx.x == 0) partial[2 * (i64)blockIdx.x] = t_ssim, partial[2 * (i64)blockIdx.x + 1] = t_l1;
  }
}

__global__ __launch_bounds__(kThreads) void k_ssim_l1_fwd(const float* __restrict__ img1, const float* __restrict__ img2,
                                                         int height, int width, int tiles_x, int tiles_y, Window win, float c1,
                                                         float c2, float* __restrict__ dm_dmu1, float* __restrict__ dm_de11,
                                                         float* __restrict__ dm_de12, float* __restrict__ partial) {
  ssim_tile<false, false>(img1, img2, nullptr, height, width, tiles_x, tiles_y, win, c1, c2, 0, dm_dmu1, dm_de11, dm_de12, partial);
}

__global__ __launch_bounds__(kThreads) void k_image_metrics(const float* __restrict__ img1, const float* __restrict__ img2,
                                                           int height, int width, int tiles_x, int tiles_y, Window win, float c1,
                                                           float c2, int clamp, float* __restrict__ partial) {
  ssim_tile<false, true>(img1, img2, nullptr, height, width, tiles_x, tiles_y, win, c1, c2, clamp, nullptr, nullptr, nullptr, partial);
}

__global__ __launch_bounds__(kThreads) void k_ssim_l1_fwd_exposure(const float* __restrict__ img1, const float* __restrict__ img2,
                                                                  const float* __restrict__ exposure, int height, int width,
                                                                  int tiles_x, int tiles_y, Window win, float c1, float c2,
                                                                  float* __restrict__ dm_dmu1, float* __restrict__ dm_de11,
                                                                  float* __restrict__ dm_de12, float* __restrict__ partial) {
  ssim_tile<true, false>(img1, img2, exposure, height, width, tiles_x, tiles_y, win, c1, c2, 0, dm_dmu1, dm_de11, dm_de12, partial);
}

__global__ __launch_bounds__(kThreads) void k_image_metrics_exposure(const float* __restrict__ img1, const float* __restrict__ img2,
                                                                    const float* __restrict__ exposure, int height, int width,
                                                                    int tiles_x, int tiles_y, Window win, float c1, float c2, int clamp,
                                                                    float* __restrict__ partial) {
  ssim_tile<true, true>(img1, img2, exposure, height, width, tiles_x, tiles_y, win, c1, c2, clamp, nullptr, nullptr, nullptr, partial);
}

// One block per image: its channels x tiles partials of k_image_metrics lie next to each other (block = plane * tiles +
// tile, plane = image * channels + c).  Added in double in a fixed order — strided per thread, then a fixed LDS tree, no
// atomics — and divided by the image's element count: out[image] = (mean (a-b)^2, mean |a-b|, mean SSIM).
__global__ __launch_bounds__(kThreads) void k_metrics_fold(const float* __restrict__ partial, i64 per_image, double count,
                                                          double* __restrict__ out) {
  __shared__ double s_acc[3][kThreads];
  const float* p = partial + 3 * per_image * (i64)blockIdx.x;
  double ssim = 0.0, l1 = 0.0, sq = 0.0;
  i64 i = threadIdx.x;
  for (; i + 7 * kThreads < per_image; i += 8 * kThreads) {  // eight loads in flight; added in the order of the plain loop
    float v[8][3];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float* q = p + 3 * (i + u * kThreads);
      v[u][0] = q[0], v[u][1] = q[1], v[u][2] = q[2];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) ssim += (double)v[u][0], l1 += (double)v[u][1], sq += (double)v[u][2];
  }
  for (; i < per_image; i += kThreads) ssim += (double)p[3 * i], l1 += (double)p[3 * i + 1], sq += (double)p[3 * i + 2];
  s_acc[0][threadIdx.x] = sq, s_acc[1][threadIdx.x] = l1, s_acc[2][threadIdx.x] = ssim;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s_acc[k][threadIdx.x] += s_acc[k][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) out[3 * (i64)blockIdx.x + threadIdx.x] = s_acc[threadIdx.x][0] / count;
}

// ---- backward --------------------------------------------------------------------------------------------------------------
// Weight of map pixel q in the adjoint at image pixel p along one axis of length n: the direct tap plus the taps
// that reached p through the reflection at either edge.
__device__ __forceinline__ float adjoint_weight(const Window& win, int p, int q, int n) {
  const int d = q - p;
  float w = win.w[d + kR];
  const int sl = p + q, sr = 2 * (n - 1) - p - q;
  if (p >= 1 && q >= 0 && sl <= kR) w += win.w[sl + kR];
  if (p <= n - 2 && q <= n - 1 && sr <= kR) w += win.w[sr + kR];
  return w;
}

// OPAQUE: the pixel index is made opaque to the compiler.  Only k_ssim_l1_bwd_exposure sets it, whose channel loop calls both
// passes below three times: the adjoint_weight values do not depend on the channel, and left alone the compiler hoists all of
// them out of the loop and keeps them live (215 VGPRs, profiles/r28_exposure.md).  Opaque per channel, the edge weights are
// formed again, as k_ssim_l1_bwd forms them once.  The weights are the same expressions either way: the same bits.
template <bool OPAQUE>
__device__ __forceinline__ void opaque(int& v) {
  if constexpr (OPAQUE) asm volatile("" : "+v"(v));
}

// The halo tile of the three maps of the plane at `base` into s_m.
__device__ __forceinline__ void stage_maps(float (*s_m)[kHH][kHW + 1], const float* __restrict__ dm_dmu1,
                                           const float* __restrict__ dm_de11, const float* __restrict__ dm_de12, i64 base, int x0,
                                           int y0, int height, int width) {
  for (int i = threadIdx.x; i < kHH * kHW; i += kThreads) {
    const int r = i / kHW, c = i % kHW;
    const int y = y0 + r - kR, x = x0 + c - kR;
    const bool in = y >= 0 && y < height && x >= 0 && x < width;  // the maps are zero outside the image
    const i64 o = base + (i64)y * width + x;
    s_m[0][r][c] = in ? dm_dmu1[o] : 0.f;
    s_m[1][r][c] = in ? dm_de11[o] : 0.f;
    s_m[2][r][c] = in ? dm_de12[o] : 0.f;
  }
}

// Row pass of the adjoint blur: s_m -> s_h.
template <bool OPAQUE>
__device__ __forceinline__ void adjoint_rows(const float (*s_m)[kHH][kHW + 1], float (*s_h)[kHH][kTW + 1], const Window& win, int x0,
                                             int width) {
  const bool edge_x = x0 < kR + 1 || x0 + kTW + kR + 1 >= width;
  for (int i = threadIdx.x; i < kHH * kTW; i += kThreads) {
    const int r = i / kTW, c = i % kTW;
    int p = x0 + c;
    opaque<OPAQUE>(p);
    float h0 = 0.f, h1 = 0.f, h2 = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float w = edge_x ? adjoint_weight(win, p, p + k - kR, width) : win.w[k];
      h0 += w * s_m[0][r][c + k], h1 += w * s_m[1][r][c + k], h2 += w * s_m[2][r][c + k];
    }
    s_h[0][r][c] = h0, s_h[1][r][c] = h1, s_h[2][r][c] = h2;
  }
}

// Column pass of the adjoint blur at tile pixel (r, c), image row y (made opaque in place): s_h -> g[0..2].
template <bool OPAQUE>
__device__ __forceinline__ void adjoint_column(const float (*s_h)[kHH][kTW + 1], const Window& win, int r, int c, int& y, int y0,
                                               int height, float (&g)[3]) {
  const bool edge_y = y0 < kR + 1 || y0 + kTH + kR + 1 >= height;
  opaque<OPAQUE>(y);
  g[0] = g[1] = g[2] = 0.f;
#pragma unroll
  for (int k = 0; k < kTaps; ++k) {
    const float w = edge_y ? adjoint_weight(win, y, y + k - kR, height) : win.w[k];
    g[0] += w * s_h[0][r + k][c], g[1] += w * s_h[1][r + k][c], g[2] += w * s_h[2][r + k][c];
  }
}

__global__ __launch_bounds__(kThreads) void k_ssim_l1_bwd(const float* __restrict__ img1, const float* __restrict__ img2,
                                                         const float* __restrict__ dm_dmu1, const float* __restrict__ dm_de11,
                                                         const float* __restrict__ dm_de12, int height, int width, int tiles_x,
                                                         int tiles_y, Window win, const float* __restrict__ scales,
                                                         float* __restrict__ grad) {
  __shared__ float s_m[3][kHH][kHW + 1];
  __shared__ float s_h[3][kHH][kTW + 1];
  const int tile = blockIdx.x % (tiles_x * tiles_y), plane = blockIdx.x / (tiles_x * tiles_y);
  const int x0 = (tile % tiles_x) * kTW, y0 = (tile / tiles_x) * kTH;
  const i64 base = (i64)plane * height * width;
  stage_maps(s_m, dm_dmu1, dm_de11, dm_de12, base, x0, y0, height, width);
  __syncthreads();
  adjoint_rows<false>(s_m, s_h, win, x0, width);
  __syncthreads();
  const float s_ssim = scales[0], s_l1 = scales[1];
  const int c = threadIdx.x % kTW;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int r = threadIdx.x / kTW + half * (kTH / 2);
    const int x = x0 + c;
    int y = y0 + r;
    float g[3];
    adjoint_column<false>(s_h, win, r, c, y, y0, height, g);
    if (x < width && y < height) {
      const i64 o = base + (i64)y * width + x;
      const float a = img1[o], b = img2[o];
      const float sgn = a > b ? 1.f : (a < b ? -1.f : 0.f);
      grad[o] = s_ssim * (g[0] + 2.f * a * g[1] + b * g[2]) + s_l1 * sgn;
    }
  }
}

// One block per (image, tile), looping c = 0..2 over the LDS buffers of k_ssim_l1_bwd: g_c = dL/dy_c at the thread's two
// pixels as k_ssim_l1_bwd forms it (with a := y_c, recomputed from x), then grad_x_k += E[c][k] g_c in six registers and the
// channel's four products g_c x_k, g_c in per-thread sums, reduced per wave at once into a 12 x 4 LDS table (twelve live
// accumulators would cost an occupancy step).  The twelve block sums (association of block_sum) share the one barrier after
// the loop and go to partial_e[12 * block ..]; k_exposure_fold adds them per image.  grad (dL/dx) or partial_e may be NULL:
// that output is skipped.  20 B read and 4 B written per pixel-channel, as the plain backward, plus 48 B per block.
__global__ __launch_bounds__(kThreads) void k_ssim_l1_bwd_exposure(const float* __restrict__ img1, const float* __restrict__ img2,
                                                                  const float* __restrict__ exposure,
                                                                  const float* __restrict__ dm_dmu1, const float* __restrict__ dm_de11,
                                                                  const float* __restrict__ dm_de12, int height, int width, int tiles_x,
                                                                  int tiles_y, Window win, const float* __restrict__ scales,
                                                                  float* __restrict__ grad, float* __restrict__ partial_e) {
  __shared__ float s_m[3][kHH][kHW + 1];
  __shared__ float s_h[3][kHH][kTW + 1];
  __shared__ float s_red[12][4];
  const int tile = blockIdx.x % (tiles_x * tiles_y), image = blockIdx.x / (tiles_x * tiles_y);
  const int x0 = (tile % tiles_x) * kTW, y0 = (tile / tiles_x) * kTH;
  const i64 stride = (i64)height * width, base = (i64)image * 3 * stride;
  const float* e = exposure + 12 * (i64)image;
  const float s_ssim = scales[0], s_l1 = scales[1];
  const int c = threadIdx.x % kTW;
  float px[2][3], gx[2][3];
  bool inside[2];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int x = x0 + c, y = y0 + threadIdx.x / kTW + half * (kTH / 2);
    inside[half] = x < width && y < height;
    const i64 o = base + (i64)y * width + x;
#pragma unroll
    for (int k = 0; k < 3; ++k) px[half][k] = inside[half] ? img1[o + k * stride] : 0.f, gx[half][k] = 0.f;
  }
#pragma unroll 1  // one channel's registers at a time: unrolled, the three bodies overlap and cost an occupancy step
  for (int ch = 0; ch < 3; ++ch) {
    const i64 pbase = base + ch * stride;
    stage_maps(s_m, dm_dmu1, dm_de11, dm_de12, pbase, x0, y0, height, width);
    __syncthreads();
    adjoint_rows<true>(s_m, s_h, win, x0, width);
    __syncthreads();  // also: every read of s_m is done before the next channel is staged
    float ge[4] = {0.f, 0.f, 0.f, 0.f};  // this thread's share of dL/dE[ch][0..3]
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int r = threadIdx.x / kTW + half * (kTH / 2);
      int y = y0 + r;
      float g3[3];
      adjoint_column<true>(s_h, win, r, c, y, y0, height, g3);
      if (inside[half]) {
        const float a = exposure_apply(e + 4 * ch, px[half][0], px[half][1], px[half][2]);
        const float b = img2[pbase + (i64)y * width + x0 + c];
        const float sgn = a > b ? 1.f : (a < b ? -1.f : 0.f);
        const float g = s_ssim * (g3[0] + 2.f * a * g3[1] + b * g3[2]) + s_l1 * sgn;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          gx[half][k] = __fmaf_rn(e[4 * ch + k], g, gx[half][k]);
          ge[k] = __fmaf_rn(g, px[half][k], ge[k]);
        }
        ge[3] += g;
      }
    }
    if (partial_e) {  // the wave's four sums of this channel; read after the barrier below the loop
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float v = ge[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) s_red[4 * ch + k][threadIdx.x >> 6] = v;
      }
    }
    // the next channel's row blur writes s_h only after the barrier that follows its staging: every read above is done by then
  }
  if (grad) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if (inside[half]) {
        const i64 o = base + (i64)(y0 + threadIdx.x / kTW + half * (kTH / 2)) * width + x0 + c;
#pragma unroll
        for (int k = 0; k < 3; ++k) grad[o + k * stride] = gx[half][k];
      }
    }
  }
  if (partial_e) {
    __syncthreads();
    if (threadIdx.x < 12) {
      const float* s = s_red[threadIdx.x];
      partial_e[12 * (i64)blockIdx.x + threadIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
    }
  }
}

// One block per image, in the pattern of k_metrics_fold: the image's `tiles` partials of k_ssim_l1_bwd_exposure (twelve floats
// each, next to each other) added in double in a fixed order — strided per thread, then a fixed LDS tree, no atomics — and
// rounded once: grad_exposure[image][12].  Every entry is written.
__global__ __launch_bounds__(kThreads) void k_exposure_fold(const float* __restrict__ partial_e, i64 tiles, float* __restrict__ grad_exposure) {
  __shared__ double s_acc[12][kThreads];
  const float* p = partial_e + 12 * tiles * (i64)blockIdx.x;
  double acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.0;
  for (i64 i = threadIdx.x; i < tiles; i += kThreads) {
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] += (double)p[12 * i + k];
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) s_acc[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
#pragma unroll
      for (int k = 0; k < 12; ++k) s_acc[k][threadIdx.x] += s_acc[k][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x < 12) grad_exposure[12 * (i64)blockIdx.x + threadIdx.x] = (float)s_acc[threadIdx.x][0];
}

// ---- host ------------------------------------------------------------------------------------------------------------------
constexpr int tiles_of(int n, int t) { return (n + t - 1) / t; }

// What every entry point needs before it looks at a pointer: the window by value, the tile grid and the block count of
// `images` x `per_image` planes (or whatever a block stands for).
struct Launch {
  Window win;
  int tx, ty;
  int64_t blocks;  // 0: an empty batch, nothing to launch
};

// GCP_OK with `l` filled, or GCP_ERR_INVALID_ARGUMENT: a negative batch, an image smaller than the reflect padding allows,
// no window, or more blocks than one grid holds.
int launch_geometry(int64_t images, int64_t per_image, int32_t height, int32_t width, const float* window11_host, Launch& l) {
  if (images < 0 || per_image <= 0 || height < kR + 1 || width < kR + 1 || !window11_host) return GCP_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < kTaps; ++k) l.win.w[k] = window11_host[k];
  l.tx = tiles_of(width, kTW), l.ty = tiles_of(height, kTH), l.blocks = 0;
  if (images == 0) return GCP_OK;
  if (images > 0x7fffffff / per_image) return GCP_ERR_INVALID_ARGUMENT;  // the plane count alone is past one grid
  if ((int64_t)l.tx * l.ty > 0x7fffffff / (images * per_image)) return GCP_ERR_INVALID_ARGUMENT;
  l.blocks = images * per_image * l.tx * l.ty;
  return GCP_OK;
}

// One launch of `grid` blocks on the entry point's `stream`; returns the HIP failure from the entry point.
#define GCP_LOSS_LAUNCH(kernel, grid, ...)                                                                   \
  do {                                                                                                       \
    hipLaunchKernelGGL(kernel, dim3((unsigned)(grid)), dim3(kThreads), 0, (hipStream_t)stream, __VA_ARGS__); \
    GCP_HIP(hipGetLastError());                                                                              \
  } while (0)

bool all_or_none(const float* a, const float* b, const float* c) { return (a != nullptr) == (b != nullptr) && (a != nullptr) == (c != nullptr); }

}  // namespace

extern "C" {

int64_t gcp_ssim_blocks(int64_t planes, int32_t height, int32_t width) {
  if (planes < 0 || height <= 0 || width <= 0) return 0;
  return planes * (int64_t)tiles_of(width, kTW) * (int64_t)tiles_of(height, kTH);
}

int64_t gcp_exposure_blocks(int64_t images, int32_t height, int32_t width) { return gcp_ssim_blocks(images, height, width); }

int gcp_ssim_l1_forward(const float* img1, const float* img2, int64_t planes, int32_t height, int32_t width,
                        const float* window11_host, float c1, float c2, float* dm_dmu1, float* dm_de11, float* dm_de12,
                        float* partial, void* stream) {
  Launch l;
  if (const int st = launch_geometry(planes, 1, height, width, window11_host, l); st != GCP_OK || l.blocks == 0) return st;
  if (!img1 || !img2 || !partial || !all_or_none(dm_dmu1, dm_de11, dm_de12)) return GCP_ERR_INVALID_ARGUMENT;
  GCP_LOSS_LAUNCH(k_ssim_l1_fwd, l.blocks, img1, img2, (int)height, (int)width, l.tx, l.ty, l.win, c1, c2, dm_dmu1, dm_de11, dm_de12, partial);
  return GCP_OK;
}

int gcp_ssim_l1_forward_exposure(const float* img, const float* ref, const float* exposure, int64_t images, int32_t height,
                                 int32_t width, const float* window11_host, float c1, float c2, float* dm_dmu1, float* dm_de11,
                                 float* dm_de12, float* partial, void* stream) {
  Launch l;
  if (const int st = launch_geometry(images, 3, height, width, window11_host, l); st != GCP_OK || l.blocks == 0) return st;
  if (!img || !ref || !exposure || !partial || !all_or_none(dm_dmu1, dm_de11, dm_de12)) return GCP_ERR_INVALID_ARGUMENT;
  GCP_LOSS_LAUNCH(k_ssim_l1_fwd_exposure, l.blocks, img, ref, exposure, (int)height, (int)width, l.tx, l.ty, l.win, c1, c2, dm_dmu1, dm_de11,
                  dm_de12, partial);
  return GCP_OK;
}

int gcp_ssim_l1_backward(const float* img1, const float* img2, const float* dm_dmu1, const float* dm_de11, const float* dm_de12,
                         int64_t planes, int32_t height, int32_t width, const float* window11_host, const float* scales,
                         float* grad_img1, void* stream) {
  Launch l;
  if (const int st = launch_geometry(planes, 1, height, width, window11_host, l); st != GCP_OK || l.blocks == 0) return st;
  if (!img1 || !img2 || !dm_dmu1 || !dm_de11 || !dm_de12 || !scales || !grad_img1) return GCP_ERR_INVALID_ARGUMENT;
  GCP_LOSS_LAUNCH(k_ssim_l1_bwd, l.blocks, img1, img2, dm_dmu1, dm_de11, dm_de12, (int)height, (int)width, l.tx, l.ty, l.win, scales, grad_img1);
  return GCP_OK;
}

int gcp_ssim_l1_backward_exposure(const float* img, const float* ref, const float* exposure, const float* dm_dmu1,
                                  const float* dm_de11, const float* dm_de12, int64_t images, int32_t height, int32_t width,
                                  const float* window11_host, const float* scales, float* grad_img, float* partial_e,
                                  float* grad_exposure, void* stream) {
  Launch l;  // a block per (image, tile)
  if (const int st = launch_geometry(images, 1, height, width, window11_host, l); st != GCP_OK || l.blocks == 0) return st;
  if (!img || !ref || !exposure || !dm_dmu1 || !dm_de11 || !dm_de12 || !scales) return GCP_ERR_INVALID_ARGUMENT;
  if ((!grad_img && !grad_exposure) || (grad_exposure && !partial_e)) return GCP_ERR_INVALID_ARGUMENT;
  GCP_LOSS_LAUNCH(k_ssim_l1_bwd_exposure, l.blocks, img, ref, exposure, dm_dmu1, dm_de11, dm_de12, (int)height, (int)width, l.tx, l.ty, l.win,
                  scales, grad_img, grad_exposure ? partial_e : nullptr);
  if (grad_exposure) GCP_LOSS_LAUNCH(k_exposure_fold, images, (const float*)partial_e, (i64)l.tx * l.ty, grad_exposure);
  return GCP_OK;
}

int gcp_image_metrics(const float* img, const float* ref, int64_t images, int32_t channels, int32_t height, int32_t width,
                      const float* window11_host, float c1, float c2, int32_t flags, float* partial, double* out, void* stream) {
  Launch l;
  if (flags & ~GCP_METRICS_CLAMP) return GCP_ERR_INVALID_ARGUMENT;
  if (const int st = launch_geometry(images, channels, height, width, window11_host, l); st != GCP_OK || l.blocks == 0) return st;
  if (!img || !ref || !partial || !out) return GCP_ERR_INVALID_ARGUMENT;
  GCP_LOSS_LAUNCH(k_image_metrics, l.blocks, img, ref, (int)height, (int)width, l.tx, l.ty, l.win, c1, c2, (int)(flags & GCP_METRICS_CLAMP), partial);
  GCP_LOSS_LAUNCH(k_metrics_fold, images, (const float*)partial, (i64)channels * l.tx * l.ty, (double)channels * (double)height * (double)width, out);
  return GCP_OK;
}

int gcp_image_metrics_exposure(const float* img, const float* ref, const float* exposure, int64_t images, int32_t height,
                               int32_t width, const float* window11_host, float c1, float c2, int32_t flags, float* partial,
                               double* out, void* stream) {
  Launch l;
  if (flags & ~GCP_METRICS_CLAMP) return GCP_ERR_INVALID_ARGUMENT;
  if (const int st = launch_geometry(images, 3, height, width, window11_host, l); st != GCP_OK || l.blocks == 0) return st;
  if (!img || !ref || !exposure || !partial || !out) return GCP_ERR_INVALID_ARGUMENT;
  GCP_LOSS_LAUNCH(k_image_metrics_exposure, l.blocks, img, ref, exposure, (int)height, (int)width, l.tx, l.ty, l.win, c1, c2,
                  (int)(flags & GCP_METRICS_CLAMP), partial);
  GCP_LOSS_LAUNCH(k_metrics_fold, images, (const float*)partial, (i64)3 * l.tx * l.ty, 3.0 * (double)height * (double)width, out);
  return GCP_OK;
}

}  // extern "C"
