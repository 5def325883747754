// gcp_mcmc.hip — MCMC density control on the device (3DGS-MCMC, Kheradmand et al., NeurIPS 2024): dead Gaussians are
// relocated onto live ones drawn with probability proportional to opacity, the scene grows to a row count the HOST fixed,
// and every optimiser step is followed by an opacity-gated noise on the positions.
//
// Five small kernels around the library's int32 prefix sum and gcp_densify.hip's row gather:
//   k_mcmc_weights  one thread per Gaussian: integer weight from sigmoid(opacity), 0 when dead; gcp::launch_excl_scan -> cum[N+1]
//   k_mcmc_draw     one thread per output row: a slot (a new row, or a dead one) draws its source by binary search in cum
//   k_mcmc_kind     one thread per output row: survivor (moments carried) or fresh (moments 0.0)
//   k_mcmc_values   one thread per output row: opacity and log scale of a source drawn c times and of its c copies (float64)
//   k_mcmc_noise    one thread per Gaussian, after every optimiser step: mean += amount gate(opacity) Sigma z
// Every draw is a pure function of (seed, row).  The one atomic, in k_mcmc_draw, counts draws per source in an integer
// whose final value does not depend on order; every other output word has exactly one writer, so the results are the same
// bit for bit whatever the launch shape.  Nothing here reads anything back to the host or waits for the stream: the number
// of output rows is the caller's arithmetic, and the total weight is read from cum[N] on the device.
#include <math.h>

#include "gcp_philox.hpp"
#include "gcp_tiles.hpp"

namespace {

using gcp::i64;

constexpr int kThreads = 256;
constexpr int kMaxCopies = 51;  // n = min(c + 1, 51): the published code's cap on the binomial table
constexpr unsigned kNoiseDomain = 1u, kDrawDomain = 2u;  // the counter's last word; 0 is gcp_densify.hip's split children

inline unsigned grid_for(i64 n) {
  const i64 b = (n + kThreads - 1) / kThreads;
  return (unsigned)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(kThreads) void k_mcmc_weights(const float* __restrict__ opacity_logit, i64 N, float min_opacity, int w_max,
                                                            int* __restrict__ weight) {
  for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < N; i += (i64)gridDim.x * kThreads) {
    const float o = sigmoid_f(opacity_logit[i]);
    int w = 0;
    if (o > min_opacity) {  // NaN: dead
      w = (int)floorf(o * (float)w_max);
      w = w < 1 ? 1 : (w > w_max ? w_max : w);
    }
    weight[i] = w;
  }
}

// A slot is an output row that must draw a source: a new row (r >= N) or a dead one (weight 0: cum[r + 1] == cum[r]).
// t = floor(r0 T / 2^32) is uniform on [0, T) up to 2^-32 T; the source is the s with cum[s] <= t < cum[s + 1], the upper
// bound of t in cum[1..N] — never a dead row, whose interval is empty.
__global__ __launch_bounds__(kThreads) void k_mcmc_draw(const int* __restrict__ cum, i64 N, i64 M, unsigned seed_lo, unsigned seed_hi,
                                                         int* __restrict__ src_row, int* __restrict__ times) {
  const unsigned T = (unsigned)cum[N];
  for (i64 r = (i64)blockIdx.x * kThreads + threadIdx.x; r < M; r += (i64)gridDim.x * kThreads) {
    if (T == 0) {  // everything is dead: plain copies
      src_row[r] = (int)(r % N);
      continue;
    }
    if (r < N && cum[r + 1] != cum[r]) {
      src_row[r] = (int)r;
      continue;
    }
    unsigned rnd[4];
    gcp::philox4x32_10((unsigned)r, 0u, 0u, kDrawDomain, seed_lo, seed_hi, rnd);
    const int t = (int)(((unsigned long long)rnd[0] * T) >> 32);
    i64 lo = 0, hi = N - 1;  // the smallest s with cum[s + 1] > t; cum[N] = T > t, so s = N - 1 always qualifies
    while (lo < hi) {
      const i64 mid = (lo + hi) >> 1;
      if (cum[mid + 1] > t) hi = mid;
      else lo = mid + 1;
    }
    src_row[r] = (int)lo;
    atomicAdd(&times[lo], 1);  // an integer count: the same whatever the order
  }
}

__global__ __launch_bounds__(kThreads) void k_mcmc_kind(const int* __restrict__ src_row, const int* __restrict__ times, i64 N, i64 M,
                                                         unsigned char* __restrict__ kind) {
  for (i64 r = (i64)blockIdx.x * kThreads + threadIdx.x; r < M; r += (i64)gridDim.x * kThreads)
    kind[r] = (unsigned char)((r < N && src_row[r] == r && times[r] == 0) ? 0 : 1);
}

// The relocation rule (the paper's eq. 9, compute_relocation of its code) for a source p drawn c times, n = min(c + 1, 51)
// Gaussians in its place afterwards: every one of them gets opacity o' with (1 - o')^n = 1 - o and the scale that keeps
// the rendered contribution, s' = s o / D.  float64 from the arrays BEFORE the pass: in float32 the alternating binomial
// sum loses up to 1.5e-3 relative at o -> 1, n = 51.  The binomials C(i - 1, k) are a running product: no table.
__global__ __launch_bounds__(kThreads) void k_mcmc_values(const float* __restrict__ opacity_logit, const float* __restrict__ log_scale,
                                                           const int* __restrict__ src_row, const int* __restrict__ times, i64 N, i64 M,
                                                           float min_opacity, float* __restrict__ opacity_out, float* __restrict__ log_scale_out) {
  for (i64 r = (i64)blockIdx.x * kThreads + threadIdx.x; r < M; r += (i64)gridDim.x * kThreads) {
    const i64 p = src_row[r];
    if (p < 0 || p >= N) continue;
    const int c = times[p];
    if (c <= 0) continue;
    const int n = c + 1 < kMaxCopies ? c + 1 : kMaxCopies;
    const double o = 1.0 / (1.0 + exp(-(double)opacity_logit[p]));
    const double o_new = 1.0 - pow(1.0 - o, 1.0 / (double)n);
    double denom = 0.0;
    for (int i = 1; i <= n; ++i) {
      double binom = 1.0, power = o_new, sign = 1.0;  // C(i - 1, k), o'^(k + 1), (-1)^k
      for (int k = 0; k < i; ++k) {
        denom += binom * sign * power / sqrt((double)(k + 1));
        binom = binom * (double)(i - 1 - k) / (double)(k + 1);
        power *= o_new;
        sign = -sign;
      }
    }
    const double shift = log(o / denom);
    log_scale_out[3 * r] = (float)((double)log_scale[3 * p] + shift);
    log_scale_out[3 * r + 1] = (float)((double)log_scale[3 * p + 1] + shift);
    log_scale_out[3 * r + 2] = (float)((double)log_scale[3 * p + 2] + shift);
    const double hi = 1.0 - 1.1920928955078125e-07;  // 1 - 2^-23
    const double oc = o_new < (double)min_opacity ? (double)min_opacity : (o_new > hi ? hi : o_new);
    opacity_out[r] = (float)log(oc / (1.0 - oc));
  }
}

// 44 bytes read and 12 written per Gaussian.  The gate 1 / (1 + e^(-k (o0 - o))) is 1/2 at o = o0 and e^(-k (o - o0)) above
// it: only nearly transparent Gaussians move.
__global__ __launch_bounds__(kThreads) void k_mcmc_noise(float* __restrict__ mean, const float4* __restrict__ quat, const float* __restrict__ log_scale,
                                                          const float* __restrict__ opacity_logit, i64 N, float amount, float k, float o0,
                                                          unsigned seed_lo, unsigned seed_hi) {
  for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < N; i += (i64)gridDim.x * kThreads) {
    const float o = sigmoid_f(opacity_logit[i]);
    const float gate = 1.0f / (1.0f + expf(-k * (o0 - o)));
    unsigned rnd[4];
    gcp::philox4x32_10((unsigned)i, 0u, 0u, kNoiseDomain, seed_lo, seed_hi, rnd);
    // Box-Muller as in k_densify_split: z0, z1 from words 0 and 1, z2 from words 2 and 3
    const float ra = sqrtf(-2.0f * gcp::log_unit_open(rnd[0])), rb = sqrtf(-2.0f * gcp::log_unit_open(rnd[2]));
    float sa, ca, sb, cb;
    sincosf(6.283185307179586f * gcp::unit_open(rnd[1]), &sa, &ca);
    sincosf(6.283185307179586f * gcp::unit_open(rnd[3]), &sb, &cb);
    (void)sb;
    const float z[3] = {ra * ca, ra * sa, rb * cb};
    float rot[9];
    const float4 q = quat[i];
    gcp::quat_rotation(q.x, q.y, q.z, q.w, rot);
    const float sx = expf(log_scale[3 * i]), sy = expf(log_scale[3 * i + 1]), sz = expf(log_scale[3 * i + 2]);
    // Sigma z = R (s^2 (.) (R^T z))
    const float vx = (sx * sx) * (rot[0] * z[0] + rot[3] * z[1] + rot[6] * z[2]);
    const float vy = (sy * sy) * (rot[1] * z[0] + rot[4] * z[1] + rot[7] * z[2]);
    const float vz = (sz * sz) * (rot[2] * z[0] + rot[5] * z[1] + rot[8] * z[2]);
    const float a = amount * gate;
    mean[3 * i] += a * (rot[0] * vx + rot[1] * vy + rot[2] * vz);
    mean[3 * i + 1] += a * (rot[3] * vx + rot[4] * vy + rot[5] * vz);
    mean[3 * i + 2] += a * (rot[6] * vx + rot[7] * vy + rot[8] * vz);
  }
}

inline bool finite_f(float v) { return std::isfinite(v); }

// what the relocation entry points share: 0 <= n_gauss <= n_rows <= INT32_MAX, and no rows out of nothing
inline bool sizes_ok(int64_t n_gauss, int64_t n_rows) {
  return n_gauss >= 0 && n_rows >= n_gauss && n_rows <= INT32_MAX && !(n_gauss == 0 && n_rows > 0);
}

}  // namespace

extern "C" size_t gcp_mcmc_workspace_bytes(int64_t n_gauss) { return gcp_scan_i32_workspace_bytes(n_gauss > 0 ? n_gauss : 0); }

extern "C" int gcp_mcmc_weights(const float* opacity_logit, int64_t n_gauss, float min_opacity, int32_t w_max, int32_t* weight, int32_t* cum,
                                void* ws, size_t ws_bytes, void* stream) {
  if (n_gauss < 0 || !finite_f(min_opacity)) return GCP_ERR_INVALID_ARGUMENT;
  if (w_max < 1 || w_max > (1 << 16) || (w_max & (w_max - 1))) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss > (int64_t)INT32_MAX / w_max) return GCP_ERR_INVALID_ARGUMENT;  // the prefix sum is int32
  if (n_gauss == 0) return GCP_OK;
  if (!opacity_logit || !weight || !cum || !ws) return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < gcp_mcmc_workspace_bytes(n_gauss)) return GCP_ERR_WORKSPACE;
  hipLaunchKernelGGL(k_mcmc_weights, dim3(grid_for(n_gauss)), dim3(kThreads), 0, (hipStream_t)stream, opacity_logit, (i64)n_gauss, min_opacity,
                     (int)w_max, (int*)weight);
  GCP_HIP(hipGetLastError());
  return gcp::launch_excl_scan((const int*)weight, (int*)cum, n_gauss, (int*)ws, (hipStream_t)stream);
}

extern "C" int gcp_mcmc_draw(const int32_t* cum, int64_t n_gauss, int64_t n_rows, uint32_t seed_lo, uint32_t seed_hi, int32_t* src_row,
                             int32_t* times, uint8_t* kind, void* stream) {
  if (!sizes_ok(n_gauss, n_rows)) return GCP_ERR_INVALID_ARGUMENT;
  if (n_rows == 0) return GCP_OK;
  if (!cum || !src_row || !times || !kind) return GCP_ERR_INVALID_ARGUMENT;
  hipStream_t s = (hipStream_t)stream;
  GCP_HIP(hipMemsetAsync(times, 0, (size_t)n_gauss * sizeof(int), s));
  hipLaunchKernelGGL(k_mcmc_draw, dim3(grid_for(n_rows)), dim3(kThreads), 0, s, (const int*)cum, (i64)n_gauss, (i64)n_rows, (unsigned)seed_lo,
                     (unsigned)seed_hi, (int*)src_row, (int*)times);
  hipLaunchKernelGGL(k_mcmc_kind, dim3(grid_for(n_rows)), dim3(kThreads), 0, s, (const int*)src_row, (const int*)times, (i64)n_gauss, (i64)n_rows,
                     (unsigned char*)kind);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

extern "C" int gcp_mcmc_values(const float* opacity_logit, const float* log_scale, const int32_t* src_row, const int32_t* times, int64_t n_gauss,
                               int64_t n_rows, float min_opacity, float* opacity_out, float* log_scale_out, void* stream) {
  if (!sizes_ok(n_gauss, n_rows) || !finite_f(min_opacity)) return GCP_ERR_INVALID_ARGUMENT;
  if (n_rows == 0) return GCP_OK;
  if (!opacity_logit || !log_scale || !src_row || !times || !opacity_out || !log_scale_out) return GCP_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_mcmc_values, dim3(grid_for(n_rows)), dim3(kThreads), 0, (hipStream_t)stream, opacity_logit, log_scale, (const int*)src_row,
                     (const int*)times, (i64)n_gauss, (i64)n_rows, min_opacity, opacity_out, log_scale_out);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

extern "C" int gcp_mcmc_noise(float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit, int64_t n_gauss,
                              float amount, float k, float o0, uint32_t seed_lo, uint32_t seed_hi, void* stream) {
  if (n_gauss < 0 || n_gauss > INT32_MAX || !finite_f(amount) || !finite_f(k) || !finite_f(o0)) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0) return GCP_OK;
  if (!mean || !quat_xyzw || !log_scale || !opacity_logit || ((uintptr_t)quat_xyzw & 15)) return GCP_ERR_INVALID_ARGUMENT;  // rows are read as float4
  hipLaunchKernelGGL(k_mcmc_noise, dim3(grid_for(n_gauss)), dim3(kThreads), 0, (hipStream_t)stream, mean, (const float4*)quat_xyzw, log_scale,
                     opacity_logit, (i64)n_gauss, amount, k, o0, (unsigned)seed_lo, (unsigned)seed_hi);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}
