// gcp_filter3d.hip — Mip-Splatting's 3-D smoothing filter (Yu et al., CVPR 2024) as a stage in front of the projection: every
// Gaussian is low-pass filtered in world space by an isotropic Gaussian whose size phi comes from the highest rate at which a
// training camera samples it (focal / depth), and its opacity is scaled so that it keeps its mass.
//
// Three kernels, one thread per Gaussian in a grid-stride loop, 256 threads, at most 4096 blocks:
//   k_filter3d_rate      every ~100 iterations: rate[i] = max over the cameras that see Gaussian i of max(fx, fy) / depth
//   k_filter3d_apply     every step: (log scale, opacity logit, phi) -> the filtered log scale and opacity logit; 36 B per row
//   k_filter3d_backward  every step: their gradients, every intermediate recomputed, nothing saved; 52 B per row
// No atomics: every output word has exactly one writer and a thread's arithmetic does not depend on its position, so the
// results are the same bits whatever the launch shape.  Nothing reads anything back to the host or waits for the stream.
// The cameras are NOT staged in LDS: the camera index is the loop counter of every thread, so a camera's 12 + 4 + 2 words are
// read through wave-uniform addresses (scalar loads, once per wave and camera) and there is no chunk size.
#include <math.h>

#include "gcp_device.hpp"
#include "grouped_cumprod_hip.h"

namespace {

using gcp::i64;

constexpr int kThreads = 256;
constexpr i64 kMaxBlocks = 4096;  // the grid cap: 16 blocks per CU of 256; beyond 2^20 rows a thread takes several

inline unsigned grid_for(i64 n) {
  const i64 b = (n + kThreads - 1) / kThreads;
  return (unsigned)(b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b));
}

// t = P_c [mean; 1] with every sum left to right, u = fx t.x / t.z + cx, v = fy t.y / t.z + cy.  The camera sees the Gaussian
// iff t.z > near and u, v lie within the image widened by `margin` of its size on every side; a NaN anywhere is "not seen".
__global__ __launch_bounds__(kThreads) void k_filter3d_rate(const float* __restrict__ mean, const float* __restrict__ P, const float* __restrict__ K,
                                                             const int* __restrict__ wh, i64 N, int C, float near_z, float margin,
                                                             float* __restrict__ rate) {
  for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < N; i += (i64)gridDim.x * kThreads) {
    const float x = mean[3 * i], y = mean[3 * i + 1], z = mean[3 * i + 2];
    float best = 0.0f;
    for (int c = 0; c < C; ++c) {
      const float* p = P + 12 * (i64)c;
      const float* k = K + 9 * (i64)c;
      const float tz = p[8] * x + p[9] * y + p[10] * z + p[11];
      if (!(tz > near_z)) continue;
      const float tx = p[0] * x + p[1] * y + p[2] * z + p[3];
      const float ty = p[4] * x + p[5] * y + p[6] * z + p[7];
      const float fx = k[0], fy = k[4], cx = k[2], cy = k[5];
      const float W = (float)wh[2 * c], H = (float)wh[2 * c + 1];
      const float u = fx * tx / tz + cx, v = fy * ty / tz + cy;
      if (u >= -margin * W && u <= (1.0f + margin) * W && v >= -margin * H && v <= (1.0f + margin) * H) best = fmaxf(best, fmaxf(fx, fy) / tz);
    }
    rate[i] = best;
  }
}

// What forward and backward share, per axis j: r_j = phi^2 e^(-2 v_j) (at most 1.2e30 at phi = 1e2, v = -30) and log1p(r_j).
struct Filtered {
  float r[3], l[3];
  float log_c;       // -1/2 sum_j log1p(r_j): c = sqrt(prod s^2 / prod (s^2 + phi^2)) in (0, 1]
  float one_minus_c; // -expm1(log c): exact where c -> 1, 1 where c underflows
};

__device__ __forceinline__ Filtered filtered(float phi, float v0, float v1, float v2) {
  Filtered f;
  const float phi2 = phi * phi;
  f.r[0] = phi2 * expf(-2.0f * v0);
  f.r[1] = phi2 * expf(-2.0f * v1);
  f.r[2] = phi2 * expf(-2.0f * v2);
  f.l[0] = log1pf(f.r[0]);
  f.l[1] = log1pf(f.r[1]);
  f.l[2] = log1pf(f.r[2]);
  f.log_c = -0.5f * ((f.l[0] + f.l[1]) + f.l[2]);
  f.one_minus_c = -expm1f(f.log_c);
  return f;
}

// v'_j = v_j + 1/2 log1p(r_j)  (s'^2 = s^2 + phi^2);  x' = x + log c - log1p(e^x (1 - c))  (sigmoid(x') = sigmoid(x) c).
// A row with phi == 0 is copied: the same bits, a signed zero included.
__global__ __launch_bounds__(kThreads) void k_filter3d_apply(const float* __restrict__ log_scale, const float* __restrict__ opacity_logit,
                                                              const float* __restrict__ filter, i64 N, float* __restrict__ log_scale_out,
                                                              float* __restrict__ opacity_out) {
  for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < N; i += (i64)gridDim.x * kThreads) {
    const float phi = filter[i], x = opacity_logit[i];
    const float v0 = log_scale[3 * i], v1 = log_scale[3 * i + 1], v2 = log_scale[3 * i + 2];
    if (phi == 0.0f) {
      log_scale_out[3 * i] = v0;
      log_scale_out[3 * i + 1] = v1;
      log_scale_out[3 * i + 2] = v2;
      opacity_out[i] = x;
      continue;
    }
    const Filtered f = filtered(phi, v0, v1, v2);
    log_scale_out[3 * i] = v0 + 0.5f * f.l[0];
    log_scale_out[3 * i + 1] = v1 + 0.5f * f.l[1];
    log_scale_out[3 * i + 2] = v2 + 0.5f * f.l[2];
    const float u = expf(x) * f.one_minus_c;
    opacity_out[i] = (x + f.log_c) - log1pf(u);
  }
}

// With u = e^x (1 - c):  g_x = g_x' / (1 + u);  g_logc = g_x' (1 + e^x) / (1 + u);
// g_v_j = g_v'_j / (1 + r_j) + g_logc (r_j / (1 + r_j)) — the quotient first: g_logc r_j alone leaves float32 at r = 1e30.
// phi carries no gradient.  A row with phi == 0 passes the gradients through, the same bits.
__global__ __launch_bounds__(kThreads) void k_filter3d_backward(const float* __restrict__ log_scale, const float* __restrict__ opacity_logit,
                                                                 const float* __restrict__ filter, const float* __restrict__ g_log_scale_out,
                                                                 const float* __restrict__ g_opacity_out, i64 N, float* __restrict__ g_log_scale,
                                                                 float* __restrict__ g_opacity) {
  for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < N; i += (i64)gridDim.x * kThreads) {
    const float phi = filter[i], gx = g_opacity_out[i];
    const float g0 = g_log_scale_out[3 * i], g1 = g_log_scale_out[3 * i + 1], g2 = g_log_scale_out[3 * i + 2];
    if (phi == 0.0f) {
      g_log_scale[3 * i] = g0;
      g_log_scale[3 * i + 1] = g1;
      g_log_scale[3 * i + 2] = g2;
      g_opacity[i] = gx;
      continue;
    }
    const Filtered f = filtered(phi, log_scale[3 * i], log_scale[3 * i + 1], log_scale[3 * i + 2]);
    const float ex = expf(opacity_logit[i]);
    const float denom = 1.0f + ex * f.one_minus_c;
    const float g_logc = gx * (1.0f + ex) / denom;
    g_log_scale[3 * i] = g0 / (1.0f + f.r[0]) + g_logc * (f.r[0] / (1.0f + f.r[0]));
    g_log_scale[3 * i + 1] = g1 / (1.0f + f.r[1]) + g_logc * (f.r[1] / (1.0f + f.r[1]));
    g_log_scale[3 * i + 2] = g2 / (1.0f + f.r[2]) + g_logc * (f.r[2] / (1.0f + f.r[2]));
    g_opacity[i] = gx / denom;
  }
}

}  // namespace

extern "C" int gcp_filter3d_rate(const float* mean, const float* P, const float* K, const int32_t* wh, int64_t n_gauss, int64_t n_cams, float near_z,
                                 float margin, float* rate, void* stream) {
  if (n_gauss < 0 || n_gauss > INT32_MAX || n_cams < 0 || n_cams > INT32_MAX) return GCP_ERR_INVALID_ARGUMENT;
  if (!std::isfinite(near_z) || !std::isfinite(margin) || margin < 0.0f) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0 || n_cams == 0) return GCP_OK;
  if (!mean || !P || !K || !wh || !rate) return GCP_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_filter3d_rate, dim3(grid_for(n_gauss)), dim3(kThreads), 0, (hipStream_t)stream, mean, P, K, (const int*)wh, (i64)n_gauss,
                     (int)n_cams, near_z, margin, rate);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

extern "C" int gcp_filter3d_apply(const float* log_scale, const float* opacity_logit, const float* filter, int64_t n_gauss, float* log_scale_out,
                                  float* opacity_out, void* stream) {
  if (n_gauss < 0 || n_gauss > INT32_MAX) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0) return GCP_OK;
  if (!log_scale || !opacity_logit || !filter || !log_scale_out || !opacity_out) return GCP_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_filter3d_apply, dim3(grid_for(n_gauss)), dim3(kThreads), 0, (hipStream_t)stream, log_scale, opacity_logit, filter,
                     (i64)n_gauss, log_scale_out, opacity_out);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

extern "C" int gcp_filter3d_apply_backward(const float* log_scale, const float* opacity_logit, const float* filter, const float* g_log_scale_out,
                                           const float* g_opacity_out, int64_t n_gauss, float* g_log_scale, float* g_opacity, void* stream) {
  if (n_gauss < 0 || n_gauss > INT32_MAX) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0) return GCP_OK;
  if (!log_scale || !opacity_logit || !filter || !g_log_scale_out || !g_opacity_out || !g_log_scale || !g_opacity) return GCP_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_filter3d_backward, dim3(grid_for(n_gauss)), dim3(kThreads), 0, (hipStream_t)stream, log_scale, opacity_logit, filter,
                     g_log_scale_out, g_opacity_out, (i64)n_gauss, g_log_scale, g_opacity);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}
