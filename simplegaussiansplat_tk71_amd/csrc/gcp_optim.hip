// gcp_optim.hip — Adam update of one parameter tensor (the optimiser step of the caller).
//
// reference: gs_model.py:43-47, :64-67 (torch.optim.Adam with one learning rate per parameter tensor; default betas,
// eps, no weight decay, no amsgrad).  torch's fused multi-tensor Adam takes 0.38 ms per step for the 38 floats of 10^6
// Gaussians; the update is a pure stream — read p, g, m, v, write p, m, v (28 B per element) — so one float4-wide
// grid-stride kernel per tensor does it in ~0.2 ms.  Same arithmetic as torch:
//   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
#include "gcp_device.hpp"
#include "grouped_cumprod_hip.h"

namespace {

using gcp::i64;

struct AdamArgs {
  float lr_over_bc1, inv_sqrt_bc2, beta1, beta2, one_minus_beta1, one_minus_beta2, eps;  // rounded once, from doubles
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamArgs& a) {
  m = a.beta1 * m + a.one_minus_beta1 * g;
  v = a.beta2 * v + a.one_minus_beta2 * (g * g);
  const float denom = sqrtf(v) * a.inv_sqrt_bc2 + a.eps;
  p -= a.lr_over_bc1 * (m / denom);
}

__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, i64 n, AdamArgs a) {
  const i64 n4 = n >> 2;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n4; i += (i64)gridDim.x * 256) {
    float4 pp = reinterpret_cast<float4*>(p)[i], mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    adam_one(pp.x, gg.x, mm.x, vv.x, a);
    adam_one(pp.y, gg.y, mm.y, vv.y, a);
    adam_one(pp.z, gg.z, mm.z, vv.z, a);
    adam_one(pp.w, gg.w, mm.w, vv.w, a);
    reinterpret_cast<float4*>(p)[i] = pp, reinterpret_cast<float4*>(m)[i] = mm, reinterpret_cast<float4*>(v)[i] = vv;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {  // tail
    const i64 i = (n4 << 2) + threadIdx.x;
    adam_one(p[i], g[i], m[i], v[i], a);
  }
}

// ---- several tensors in one launch, step counts and rates on the device, optional row mask (gcp_adam_step_multi) ----
constexpr int MAX_T = GCP_ADAM_MAX_TENSORS;
constexpr i64 MAX_BLOCKS = 16384;  // per tensor, as k_adam: beyond it the blocks of a tensor grid-stride

struct AdamTensors {
  float* p[MAX_T];
  const float* g[MAX_T];
  float* m[MAX_T];
  float* v[MAX_T];
  i64 n[MAX_T];          // elements
  int width[MAX_T];
  int block_end[MAX_T];  // blocks of tensors 0..t; the unused entries hold the grid size
  float beta1, beta2, one_minus_beta1, one_minus_beta2, eps;
};

struct AdamSteps {
  int* step[MAX_T];
};

// One thread per tensor: the step count advances on the device, and the two scalars gcp_adam_step rounds on the host are
// formed from it here, in double, rounded once in the same places.
__global__ __launch_bounds__(64) void k_adam_prologue(AdamSteps s, const float* __restrict__ lr, float* __restrict__ scal, double beta1,
                                                      double beta2, int n_tensors) {
  const int t = threadIdx.x;
  if (t >= n_tensors) return;
  int* counter = s.step[0];
#pragma unroll
  for (int k = 1; k < MAX_T; ++k) counter = t == k ? s.step[k] : counter;
  const int step = *counter + 1;
  *counter = step;
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  scal[2 * t] = (float)((double)lr[t] / bc1);
  scal[2 * t + 1] = (float)(1.0 / sqrt(bc2));
}

// The row of element e and its position in that row; 32-bit division where the tensor's size allows (wave-uniform choice).
__device__ __forceinline__ void row_of(i64 e, int width, bool small, i64& row, int& col) {
  if (small) {
    const unsigned q = (unsigned)e / (unsigned)width;
    row = q, col = (int)((unsigned)e - q * (unsigned)width);
  } else {
    row = e / width, col = (int)(e - row * width);
  }
}

template <bool MASKED>
__global__ __launch_bounds__(256) void k_adam_multi(AdamTensors a, const float* __restrict__ scal, const uint8_t* __restrict__ visible) {
  // the block's tensor from the prefix values in the kernel arguments: scalar compares, the same for every wave of the block
  int t = 0;
#pragma unroll
  for (int k = 0; k < MAX_T - 1; ++k) t += (int)blockIdx.x >= a.block_end[k];
  const int first = t ? a.block_end[t - 1] : 0, blocks = a.block_end[t] - first, block = (int)blockIdx.x - first;
  float* __restrict__ p = a.p[t];
  const float* __restrict__ g = a.g[t];
  float* __restrict__ m = a.m[t];
  float* __restrict__ v = a.v[t];
  const i64 n = a.n[t], n4 = n >> 2;
  const int width = a.width[t];
  const bool small = n <= 0xffffffffLL;
  const AdamArgs c{scal[2 * t], scal[2 * t + 1], a.beta1, a.beta2, a.one_minus_beta1, a.one_minus_beta2, a.eps};
  for (i64 i = (i64)block * 256 + threadIdx.x; i < n4; i += (i64)blocks * 256) {
    bool on0 = true, on1 = true, on2 = true, on3 = true;
    if (MASKED) {
      // rows of the four elements: one division, then carries; with width >= 3 the inner two lie in the first or the last row
      i64 r0, r;
      int col;
      row_of(i << 2, width, small, r0, col);
      r = r0;
      const bool step1 = ++col == width;
      r += step1, col = step1 ? 0 : col;
      const i64 r1 = r;
      const bool step2 = ++col == width;
      r += step2, col = step2 ? 0 : col;
      const i64 r2 = r;
      r += ++col == width;
      const uint8_t v0 = visible[r0], v3 = visible[r];
      uint8_t v1 = r1 == r0 ? v0 : v3, v2 = r2 == r0 ? v0 : v3;
      if (width < 3) v1 = visible[r1], v2 = visible[r2];
      on0 = v0 != 0, on1 = v1 != 0, on2 = v2 != 0, on3 = v3 != 0;
      if (!(on0 || on1 || on2 || on3)) continue;  // nothing of this float4 is loaded or stored
    }
    float4 pp = reinterpret_cast<float4*>(p)[i], mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    if (on0) adam_one(pp.x, gg.x, mm.x, vv.x, c);
    if (on1) adam_one(pp.y, gg.y, mm.y, vv.y, c);
    if (on2) adam_one(pp.z, gg.z, mm.z, vv.z, c);
    if (on3) adam_one(pp.w, gg.w, mm.w, vv.w, c);
    reinterpret_cast<float4*>(p)[i] = pp, reinterpret_cast<float4*>(m)[i] = mm, reinterpret_cast<float4*>(v)[i] = vv;
  }
  if (block == 0 && threadIdx.x < (n & 3)) {  // tail
    const i64 i = (n4 << 2) + threadIdx.x;
    if (!MASKED || visible[i / width]) adam_one(p[i], g[i], m[i], v[i], c);
  }
}

bool beta_ok(double b) { return b >= 0.0 && b < 1.0; }

}  // namespace

extern "C" int gcp_adam_step_multi(int32_t n_tensors, float* const* param, const float* const* grad, float* const* exp_avg,
                                   float* const* exp_avg_sq, const int64_t* rows, const int32_t* width, int32_t* const* step,
                                   const float* lr, float* scal, const uint8_t* visible, double beta1, double beta2, double eps,
                                   void* stream) {
  if (n_tensors < 0 || n_tensors > MAX_T || !beta_ok(beta1) || !beta_ok(beta2)) return GCP_ERR_INVALID_ARGUMENT;
  if (n_tensors == 0) return GCP_OK;
  if (!param || !grad || !exp_avg || !exp_avg_sq || !rows || !width || !step || !lr || !scal) return GCP_ERR_INVALID_ARGUMENT;
  AdamTensors a{};
  AdamSteps s{};
  i64 total = 0;
  for (int t = 0; t < n_tensors; ++t) {
    if (width[t] < 1 || rows[t] < 0 || rows[t] > INT64_MAX / width[t] || !step[t]) return GCP_ERR_INVALID_ARGUMENT;
    if (visible && rows[t] != rows[0]) return GCP_ERR_INVALID_ARGUMENT;
    const i64 n = (i64)rows[t] * width[t];
    if (n && (!param[t] || !grad[t] || !exp_avg[t] || !exp_avg_sq[t] ||
              (((uintptr_t)param[t] | (uintptr_t)grad[t] | (uintptr_t)exp_avg[t] | (uintptr_t)exp_avg_sq[t]) & 15)))
      return GCP_ERR_INVALID_ARGUMENT;
    const i64 blocks = ((n >> 2) + 255) / 256;
    total += n == 0 ? 0 : (blocks < 1 ? 1 : (blocks > MAX_BLOCKS ? MAX_BLOCKS : blocks));
    a.p[t] = param[t], a.g[t] = grad[t], a.m[t] = exp_avg[t], a.v[t] = exp_avg_sq[t];
    a.n[t] = n, a.width[t] = width[t], a.block_end[t] = (int)total;
    s.step[t] = step[t];
  }
  for (int t = n_tensors; t < MAX_T; ++t) a.block_end[t] = (int)total, a.width[t] = 1;
  a.beta1 = (float)beta1, a.beta2 = (float)beta2, a.one_minus_beta1 = (float)(1.0 - beta1), a.one_minus_beta2 = (float)(1.0 - beta2);
  a.eps = (float)eps;
  hipLaunchKernelGGL(k_adam_prologue, dim3(1), dim3(64), 0, (hipStream_t)stream, s, lr, scal, beta1, beta2, (int)n_tensors);
  GCP_HIP(hipGetLastError());
  if (total == 0) return GCP_OK;  // every tensor empty: the steps advanced, nothing to update
  if (visible)
    hipLaunchKernelGGL(k_adam_multi<true>, dim3((unsigned)total), dim3(256), 0, (hipStream_t)stream, a, (const float*)scal, visible);
  else
    hipLaunchKernelGGL(k_adam_multi<false>, dim3((unsigned)total), dim3(256), 0, (hipStream_t)stream, a, (const float*)scal, visible);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

extern "C" int gcp_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1,
                             double beta2, double eps, int64_t step, void* stream) {
  if (n < 0 || step < 1 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return GCP_ERR_INVALID_ARGUMENT;
  if (n == 0) return GCP_OK;
  if (!param || !grad || !exp_avg || !exp_avg_sq || (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15))
    return GCP_ERR_INVALID_ARGUMENT;
  // bias corrections in double on the host, as torch computes them from the Python step count
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  AdamArgs a{(float)(lr / bc1), (float)(1.0 / sqrt(bc2)), (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps};
  const i64 blocks = ((n >> 2) + 255) / 256;
  hipLaunchKernelGGL(k_adam, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks))), dim3(256), 0, (hipStream_t)stream, param,
                     grad, exp_avg, exp_avg_sq, (i64)n, a);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}
