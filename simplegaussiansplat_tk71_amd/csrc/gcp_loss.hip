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

__global__ __launch_bounds__(kThreads) void k_ssim_l1_fwd(const float* __restrict__ img1, const float* __restrict__ img2,
                                                         int height, int width, int tiles_x, int tiles_y, Window win, float c1,
                                                         float c2, float* __restrict__ dm_dmu1, float* __restrict__ dm_de11,
                                                         float* __restrict__ dm_de12, float* __restrict__ partial) {
  __shared__ float s_a[kHH][kHW + 1], s_b[kHH][kHW + 1];
  __shared__ float s_h[5][kHH][kTW + 1];
  __shared__ float s_red[4];
  const int tile = blockIdx.x % (tiles_x * tiles_y), plane = blockIdx.x / (tiles_x * tiles_y);
  const int x0 = (tile % tiles_x) * kTW, y0 = (tile / tiles_x) * kTH;
  const float* a = img1 + (i64)plane * height * width;
  const float* b = img2 + (i64)plane * height * width;
  for (int i = threadIdx.x; i < kHH * kHW; i += kThreads) {
    const int r = i / kHW, c = i % kHW;
    // rows / columns past the image edge of a partial tile are clamped: their results are never used
    const int y = reflect(min(y0 + r - kR, height - 1 + kR), height), x = reflect(min(x0 + c - kR, width - 1 + kR), width);
    s_a[r][c] = a[(i64)y * width + x];
    s_b[r][c] = b[(i64)y * width + x];
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
  float sum_ssim = 0.f, sum_l1 = 0.f;
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
      sum_ssim += m;
      sum_l1 += fabsf(s_a[r + kR][c + kR] - s_b[r + kR][c + kR]);
      if (dm_dmu1) {
        const i64 o = ((i64)plane * height + y) * width + x;
        const float m_den = m / den;  // A B / den^2
        dm_dmu1[o] = (2.f * mu2 * (B - A)) / den - m_den * (2.f * mu1 * (D - C));
        dm_de11[o] = -m_den * C;
        dm_de12[o] = 2.f * A / den;
      }
    }
  }
  const float t_ssim = block_sum(sum_ssim, s_red);
  __syncthreads();
  const float t_l1 = block_sum(sum_l1, s_red);
  if (threadIdx.x == 0) partial[2 * (i64)blockIdx.x] = t_ssim, partial[2 * (i64)blockIdx.x + 1] = t_l1;
}

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
  for (int i = threadIdx.x; i < kHH * kHW; i += kThreads) {
    const int r = i / kHW, c = i % kHW;
    const int y = y0 + r - kR, x = x0 + c - kR;
    const bool in = y >= 0 && y < height && x >= 0 && x < width;  // the maps are zero outside the image
    const i64 o = base + (i64)y * width + x;
    s_m[0][r][c] = in ? dm_dmu1[o] : 0.f;
    s_m[1][r][c] = in ? dm_de11[o] : 0.f;
    s_m[2][r][c] = in ? dm_de12[o] : 0.f;
  }
  __syncthreads();
  const bool edge_x = x0 < kR + 1 || x0 + kTW + kR + 1 >= width;
  for (int i = threadIdx.x; i < kHH * kTW; i += kThreads) {
    const int r = i / kTW, c = i % kTW;
    const int p = x0 + c;
    float h0 = 0.f, h1 = 0.f, h2 = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float w = edge_x ? adjoint_weight(win, p, p + k - kR, width) : win.w[k];
      h0 += w * s_m[0][r][c + k], h1 += w * s_m[1][r][c + k], h2 += w * s_m[2][r][c + k];
    }
    s_h[0][r][c] = h0, s_h[1][r][c] = h1, s_h[2][r][c] = h2;
  }
  __syncthreads();
  const bool edge_y = y0 < kR + 1 || y0 + kTH + kR + 1 >= height;
  const float s_ssim = scales[0], s_l1 = scales[1];
  const int c = threadIdx.x % kTW;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int r = threadIdx.x / kTW + half * (kTH / 2);
    const int x = x0 + c, y = y0 + r;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
      const float w = edge_y ? adjoint_weight(win, y, y + k - kR, height) : win.w[k];
      g0 += w * s_h[0][r + k][c], g1 += w * s_h[1][r + k][c], g2 += w * s_h[2][r + k][c];
    }
    if (x < width && y < height) {
      const i64 o = base + (i64)y * width + x;
      const float a = img1[o], b = img2[o];
      const float sgn = a > b ? 1.f : (a < b ? -1.f : 0.f);
      grad[o] = s_ssim * (g0 + 2.f * a * g1 + b * g2) + s_l1 * sgn;
    }
  }
}

// Evaluation (no gradient, no maps): the tiling, staging and blurs of k_ssim_l1_fwd, with three sums per block — the SSIM
// map, |a - b| and (a - b)^2 — at partial[3 * block ..].  clamp: img1 (the render; never the photograph) is clamped to
// [0, 1] as it is staged, so that all three terms see the clamped value (NaN stays NaN).  8 B read per pixel-channel.
__global__ __launch_bounds__(kThreads) void k_image_metrics(const float* __restrict__ img1, const float* __restrict__ img2,
                                                           int height, int width, int tiles_x, int tiles_y, Window win, float c1,
                                                           float c2, int clamp, float* __restrict__ partial) {
  __shared__ float s_a[kHH][kHW + 1], s_b[kHH][kHW + 1];
  __shared__ float s_h[5][kHH][kTW + 1];
  __shared__ float s_red[3][4];
  const int tile = blockIdx.x % (tiles_x * tiles_y), plane = blockIdx.x / (tiles_x * tiles_y);
  const int x0 = (tile % tiles_x) * kTW, y0 = (tile / tiles_x) * kTH;
  const float* a = img1 + (i64)plane * height * width;
  const float* b = img2 + (i64)plane * height * width;
  const float lo = clamp ? 0.f : -__builtin_inff(), hi = clamp ? 1.f : __builtin_inff();
  for (int i = threadIdx.x; i < kHH * kHW; i += kThreads) {
    const int r = i / kHW, c = i % kHW;
    // rows / columns past the image edge of a partial tile are clamped: their results are never used
    const int y = reflect(min(y0 + r - kR, height - 1 + kR), height), x = reflect(min(x0 + c - kR, width - 1 + kR), width);
    // both loads first, then two selects against uniform bounds (+-inf without the clamp: the identity): a branch on the
    // loaded value would hold the second load back until the first has returned
    const float va = a[(i64)y * width + x], vb = b[(i64)y * width + x];
    s_a[r][c] = va < lo ? lo : (va > hi ? hi : va);
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
      const float d = s_a[r + kR][c + kR] - s_b[r + kR][c + kR];
      sum_ssim += A * B / (C * D + 1e-12f);
      sum_l1 += fabsf(d);
      sum_sq += d * d;
    }
  }
  block_sum3(sum_ssim, sum_l1, sum_sq, s_red);
  if (threadIdx.x == 0) {
    float* p = partial + 3 * (i64)blockIdx.x;
    p[0] = sum_ssim, p[1] = sum_l1, p[2] = sum_sq;
  }
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

// ---- per-camera exposure compensation -------------------------------------------------------------------
// One learned 3 x 4 colour affine per image, applied to the render before the loss: y_c = E[c][0] x_0 + E[c][1] x_1 +
// E[c][2] x_2 + E[c][3].  y is never written to memory: it is formed as the tile is staged (reflect padding commutes with a
// pointwise map), and the backward forms it again from x.  Siblings of the kernels above, whose text stays as it is.

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

// k_ssim_l1_fwd with y staged in place of img1: grid, tile, LDS layout and partial index are its own (block = plane * tiles +
// tile, plane = 3 * image + c), so the host adds the block sums in the same order.  The two extra channel loads per halo
// position re-read lines the blocks of the sibling planes fetch too.
__global__ __launch_bounds__(kThreads) void k_ssim_l1_fwd_exposure(const float* __restrict__ img1, const float* __restrict__ img2,
                                                                  const float* __restrict__ exposure, int height, int width,
                                                                  int tiles_x, int tiles_y, Window win, float c1, float c2,
                                                                  float* __restrict__ dm_dmu1, float* __restrict__ dm_de11,
                                                                  float* __restrict__ dm_de12, float* __restrict__ partial) {
  __shared__ float s_a[kHH][kHW + 1], s_b[kHH][kHW + 1];
  __shared__ float s_h[5][kHH][kTW + 1];
  __shared__ float s_red[4];
  const int tile = blockIdx.x % (tiles_x * tiles_y), plane = blockIdx.x / (tiles_x * tiles_y);
  const int x0 = (tile % tiles_x) * kTW, y0 = (tile / tiles_x) * kTH;
  const i64 stride = (i64)height * width;
  const float* a = img1 + (i64)(plane / 3) * 3 * stride;  // the image's three planes
  const float* b = img2 + (i64)plane * stride;
  const float* e = exposure + 4 * (i64)plane;  // row c of image i: 12 i + 4 c
  for (int i = threadIdx.x; i < kHH * kHW; i += kThreads) {
    const int r = i / kHW, c = i % kHW;
    // rows / columns past the image edge of a partial tile are clamped: their results are never used
    const int y = reflect(min(y0 + r - kR, height - 1 + kR), height), x = reflect(min(x0 + c - kR, width - 1 + kR), width);
    s_a[r][c] = exposure_stage(a, stride, (i64)y * width + x, e);
    s_b[r][c] = b[(i64)y * width + x];
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
  float sum_ssim = 0.f, sum_l1 = 0.f;
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
      sum_ssim += m;
      sum_l1 += fabsf(s_a[r + kR][c + kR] - s_b[r + kR][c + kR]);
      if (dm_dmu1) {
        const i64 o = ((i64)plane * height + y) * width + x;
        const float m_den = m / den;  // A B / den^2
        dm_dmu1[o] = (2.f * mu2 * (B - A)) / den - m_den * (2.f * mu1 * (D - C));
        dm_de11[o] = -m_den * C;
        dm_de12[o] = 2.f * A / den;
      }
    }
  }
  const float t_ssim = block_sum(sum_ssim, s_red);
  __syncthreads();
  const float t_l1 = block_sum(sum_l1, s_red);
  if (threadIdx.x == 0) partial[2 * (i64)blockIdx.x] = t_ssim, partial[2 * (i64)blockIdx.x + 1] = t_l1;
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
  const bool edge_x = x0 < kR + 1 || x0 + kTW + kR + 1 >= width;
  const bool edge_y = y0 < kR + 1 || y0 + kTH + kR + 1 >= height;
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
    for (int i = threadIdx.x; i < kHH * kHW; i += kThreads) {
      const int r = i / kHW, cc = i % kHW;
      const int y = y0 + r - kR, x = x0 + cc - kR;
      const bool in = y >= 0 && y < height && x >= 0 && x < width;  // the maps are zero outside the image
      const i64 o = pbase + (i64)y * width + x;
      s_m[0][r][cc] = in ? dm_dmu1[o] : 0.f;
      s_m[1][r][cc] = in ? dm_de11[o] : 0.f;
      s_m[2][r][cc] = in ? dm_de12[o] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kHH * kTW; i += kThreads) {
      const int r = i / kTW, cc = i % kTW;
      int p = x0 + cc;
      asm volatile("" : "+v"(p));  // opaque per channel: the edge weights are formed again, not kept in registers across the loop
      float h0 = 0.f, h1 = 0.f, h2 = 0.f;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) {
        const float w = edge_x ? adjoint_weight(win, p, p + k - kR, width) : win.w[k];
        h0 += w * s_m[0][r][cc + k], h1 += w * s_m[1][r][cc + k], h2 += w * s_m[2][r][cc + k];
      }
      s_h[0][r][cc] = h0, s_h[1][r][cc] = h1, s_h[2][r][cc] = h2;
    }
    __syncthreads();  // also: every read of s_m is done before the next channel is staged
    float ge[4] = {0.f, 0.f, 0.f, 0.f};  // this thread's share of dL/dE[ch][0..3]
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int r = threadIdx.x / kTW + half * (kTH / 2);
      int y = y0 + r;
      asm volatile("" : "+v"(y));  // as p above
      float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
      for (int k = 0; k < kTaps; ++k) {
        const float w = edge_y ? adjoint_weight(win, y, y + k - kR, height) : win.w[k];
        g0 += w * s_h[0][r + k][c], g1 += w * s_h[1][r + k][c], g2 += w * s_h[2][r + k][c];
      }
      if (inside[half]) {
        const float a = exposure_apply(e + 4 * ch, px[half][0], px[half][1], px[half][2]);
        const float b = img2[pbase + (i64)y * width + x0 + c];
        const float sgn = a > b ? 1.f : (a < b ? -1.f : 0.f);
        const float g = s_ssim * (g0 + 2.f * a * g1 + b * g2) + s_l1 * sgn;
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

// k_image_metrics on y: compensated as it is staged (exposure_stage), clamped after — the clamp applies to y.  The partials
// and k_metrics_fold are those of k_image_metrics (three channels).
__global__ __launch_bounds__(kThreads) void k_image_metrics_exposure(const float* __restrict__ img1, const float* __restrict__ img2,
                                                                    const float* __restrict__ exposure, int height, int width,
                                                                    int tiles_x, int tiles_y, Window win, float c1, float c2, int clamp,
                                                                    float* __restrict__ partial) {
  __shared__ float s_a[kHH][kHW + 1], s_b[kHH][kHW + 1];
  __shared__ float s_h[5][kHH][kTW + 1];
  __shared__ float s_red[3][4];
  const int tile = blockIdx.x % (tiles_x * tiles_y), plane = blockIdx.x / (tiles_x * tiles_y);
  const int x0 = (tile % tiles_x) * kTW, y0 = (tile / tiles_x) * kTH;
  const i64 stride = (i64)height * width;
  const float* a = img1 + (i64)(plane / 3) * 3 * stride;
  const float* b = img2 + (i64)plane * stride;
  const float* e = exposure + 4 * (i64)plane;
  const float lo = clamp ? 0.f : -__builtin_inff(), hi = clamp ? 1.f : __builtin_inff();
  for (int i = threadIdx.x; i < kHH * kHW; i += kThreads) {
    const int r = i / kHW, c = i % kHW;
    // rows / columns past the image edge of a partial tile are clamped: their results are never used
    const int y = reflect(min(y0 + r - kR, height - 1 + kR), height), x = reflect(min(x0 + c - kR, width - 1 + kR), width);
    // all four loads first, then two selects against uniform bounds (+-inf without the clamp: the identity)
    const float va = exposure_stage(a, stride, (i64)y * width + x, e), vb = b[(i64)y * width + x];
    s_a[r][c] = va < lo ? lo : (va > hi ? hi : va);
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
      const float d = s_a[r + kR][c + kR] - s_b[r + kR][c + kR];
      sum_ssim += A * B / (C * D + 1e-12f);
      sum_l1 += fabsf(d);
      sum_sq += d * d;
    }
  }
  block_sum3(sum_ssim, sum_l1, sum_sq, s_red);
  if (threadIdx.x == 0) {
    float* p = partial + 3 * (i64)blockIdx.x;
    p[0] = sum_ssim, p[1] = sum_l1, p[2] = sum_sq;
  }
}

bool make_window(const float* window11_host, Window& w) {
  if (!window11_host) return false;
  for (int k = 0; k < kTaps; ++k) w.w[k] = window11_host[k];
  return true;
}

}  // namespace

extern "C" {

int64_t gcp_ssim_blocks(int64_t planes, int32_t height, int32_t width) {
  if (planes < 0 || height <= 0 || width <= 0) return 0;
  return planes * (int64_t)((width + kTW - 1) / kTW) * (int64_t)((height + kTH - 1) / kTH);
}

int gcp_ssim_l1_forward(const float* img1, const float* img2, int64_t planes, int32_t height, int32_t width,
                        const float* window11_host, float c1, float c2, float* dm_dmu1, float* dm_de11, float* dm_de12,
                        float* partial, void* stream) {
  Window win;
  if (planes < 0 || height < kR + 1 || width < kR + 1 || !make_window(window11_host, win)) return GCP_ERR_INVALID_ARGUMENT;
  const int64_t blocks = gcp_ssim_blocks(planes, height, width);
  if (blocks == 0) return GCP_OK;
  if (blocks > 0x7fffffff || !img1 || !img2 || !partial) return GCP_ERR_INVALID_ARGUMENT;
  if ((dm_dmu1 != nullptr) != (dm_de11 != nullptr) || (dm_dmu1 != nullptr) != (dm_de12 != nullptr)) return GCP_ERR_INVALID_ARGUMENT;
  const int tx = (width + kTW - 1) / kTW, ty = (height + kTH - 1) / kTH;
  hipLaunchKernelGGL(k_ssim_l1_fwd, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, img1, img2, (int)height,
                     (int)width, tx, ty, win, c1, c2, dm_dmu1, dm_de11, dm_de12, partial);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int gcp_ssim_l1_backward(const float* img1, const float* img2, const float* dm_dmu1, const float* dm_de11, const float* dm_de12,
                         int64_t planes, int32_t height, int32_t width, const float* window11_host, const float* scales,
                         float* grad_img1, void* stream) {
  Window win;
  if (planes < 0 || height < kR + 1 || width < kR + 1 || !make_window(window11_host, win)) return GCP_ERR_INVALID_ARGUMENT;
  const int64_t blocks = gcp_ssim_blocks(planes, height, width);
  if (blocks == 0) return GCP_OK;
  if (blocks > 0x7fffffff || !img1 || !img2 || !dm_dmu1 || !dm_de11 || !dm_de12 || !scales || !grad_img1) return GCP_ERR_INVALID_ARGUMENT;
  const int tx = (width + kTW - 1) / kTW, ty = (height + kTH - 1) / kTH;
  hipLaunchKernelGGL(k_ssim_l1_bwd, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, img1, img2, dm_dmu1, dm_de11,
                     dm_de12, (int)height, (int)width, tx, ty, win, scales, grad_img1);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int gcp_image_metrics(const float* img, const float* ref, int64_t images, int32_t channels, int32_t height, int32_t width,
                      const float* window11_host, float c1, float c2, int32_t flags, float* partial, double* out, void* stream) {
  Window win;
  if (images < 0 || channels <= 0 || height < kR + 1 || width < kR + 1 || (flags & ~GCP_METRICS_CLAMP) || !make_window(window11_host, win))
    return GCP_ERR_INVALID_ARGUMENT;
  if (images == 0) return GCP_OK;
  if (images > 0x7fffffff / channels) return GCP_ERR_INVALID_ARGUMENT;  // the plane count alone is past one grid
  const int64_t blocks = gcp_ssim_blocks(images * channels, height, width);
  if (blocks > 0x7fffffff || !img || !ref || !partial || !out) return GCP_ERR_INVALID_ARGUMENT;
  const int tx = (width + kTW - 1) / kTW, ty = (height + kTH - 1) / kTH;
  hipLaunchKernelGGL(k_image_metrics, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, img, ref, (int)height, (int)width,
                     tx, ty, win, c1, c2, (int)(flags & GCP_METRICS_CLAMP), partial);
  GCP_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_metrics_fold, dim3((unsigned)images), dim3(kThreads), 0, (hipStream_t)stream, (const float*)partial,
                     (i64)channels * tx * ty, (double)channels * (double)height * (double)width, out);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int64_t gcp_exposure_blocks(int64_t images, int32_t height, int32_t width) { return gcp_ssim_blocks(images, height, width); }

int gcp_ssim_l1_forward_exposure(const float* img, const float* ref, const float* exposure, int64_t images, int32_t height,
                                 int32_t width, const float* window11_host, float c1, float c2, float* dm_dmu1, float* dm_de11,
                                 float* dm_de12, float* partial, void* stream) {
  Window win;
  if (images < 0 || height < kR + 1 || width < kR + 1 || !make_window(window11_host, win)) return GCP_ERR_INVALID_ARGUMENT;
  if (images == 0) return GCP_OK;
  if (images > 0x7fffffff / 3) return GCP_ERR_INVALID_ARGUMENT;  // the plane count alone is past one grid
  const int64_t blocks = gcp_ssim_blocks(3 * images, height, width);
  if (blocks > 0x7fffffff || !img || !ref || !exposure || !partial) return GCP_ERR_INVALID_ARGUMENT;
  if ((dm_dmu1 != nullptr) != (dm_de11 != nullptr) || (dm_dmu1 != nullptr) != (dm_de12 != nullptr)) return GCP_ERR_INVALID_ARGUMENT;
  const int tx = (width + kTW - 1) / kTW, ty = (height + kTH - 1) / kTH;
  hipLaunchKernelGGL(k_ssim_l1_fwd_exposure, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, img, ref, exposure,
                     (int)height, (int)width, tx, ty, win, c1, c2, dm_dmu1, dm_de11, dm_de12, partial);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int gcp_ssim_l1_backward_exposure(const float* img, const float* ref, const float* exposure, const float* dm_dmu1,
                                  const float* dm_de11, const float* dm_de12, int64_t images, int32_t height, int32_t width,
                                  const float* window11_host, const float* scales, float* grad_img, float* partial_e,
                                  float* grad_exposure, void* stream) {
  Window win;
  if (images < 0 || height < kR + 1 || width < kR + 1 || !make_window(window11_host, win)) return GCP_ERR_INVALID_ARGUMENT;
  if (images == 0) return GCP_OK;
  const int64_t blocks = gcp_exposure_blocks(images, height, width);
  if (blocks > 0x7fffffff || !img || !ref || !exposure || !dm_dmu1 || !dm_de11 || !dm_de12 || !scales) return GCP_ERR_INVALID_ARGUMENT;
  if ((!grad_img && !grad_exposure) || (grad_exposure && !partial_e)) return GCP_ERR_INVALID_ARGUMENT;
  const int tx = (width + kTW - 1) / kTW, ty = (height + kTH - 1) / kTH;
  hipLaunchKernelGGL(k_ssim_l1_bwd_exposure, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, img, ref, exposure, dm_dmu1,
                     dm_de11, dm_de12, (int)height, (int)width, tx, ty, win, scales, grad_img, grad_exposure ? partial_e : nullptr);
  GCP_HIP(hipGetLastError());
  if (grad_exposure) {
    hipLaunchKernelGGL(k_exposure_fold, dim3((unsigned)images), dim3(kThreads), 0, (hipStream_t)stream, (const float*)partial_e,
                       (i64)tx * ty, grad_exposure);
    GCP_HIP(hipGetLastError());
  }
  return GCP_OK;
}

int gcp_image_metrics_exposure(const float* img, const float* ref, const float* exposure, int64_t images, int32_t height,
                               int32_t width, const float* window11_host, float c1, float c2, int32_t flags, float* partial,
                               double* out, void* stream) {
  Window win;
  if (images < 0 || height < kR + 1 || width < kR + 1 || (flags & ~GCP_METRICS_CLAMP) || !make_window(window11_host, win))
    return GCP_ERR_INVALID_ARGUMENT;
  if (images == 0) return GCP_OK;
  if (images > 0x7fffffff / 3) return GCP_ERR_INVALID_ARGUMENT;  // the plane count alone is past one grid
  const int64_t blocks = gcp_ssim_blocks(images * 3, height, width);
  if (blocks > 0x7fffffff || !img || !ref || !exposure || !partial || !out) return GCP_ERR_INVALID_ARGUMENT;
  const int tx = (width + kTW - 1) / kTW, ty = (height + kTH - 1) / kTH;
  hipLaunchKernelGGL(k_image_metrics_exposure, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, img, ref, exposure,
                     (int)height, (int)width, tx, ty, win, c1, c2, (int)(flags & GCP_METRICS_CLAMP), partial);
  GCP_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_metrics_fold, dim3((unsigned)images), dim3(kThreads), 0, (hipStream_t)stream, (const float*)partial,
                     (i64)3 * tx * ty, 3.0 * (double)height * (double)width, out);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

}  // extern "C"
