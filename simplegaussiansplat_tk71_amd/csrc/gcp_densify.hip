// gcp_densify.hip — density control on the device (the caller's densify / prune, gs_model.py:201-265).
//
// Five small kernels around the library's int32 prefix sum:
//   k_densify_accumulate  the screen-space statistic: per camera, |d loss / d centre| added to every listed Gaussian
//   k_densify_plan        one thread per Gaussian: split / clone / keep from the state BEFORE the pass, prune test on the
//                         rows the action writes -> count[N], action[N]; gcp::launch_excl_scan -> offset[N+1]
//   k_densify_fill        one thread per Gaussian: src_row / kind of its output rows (contiguous, in Gaussian order)
//   k_densify_rows        output-driven row gather of one tensor (parameters: copy; Adam moments: copy survivors, zero the rest)
//   k_densify_split       mean and log scale of the split children, Philox4x32-10 + Box-Muller per (seed, parent, child)
// Nothing here is ordered by timing: no atomics on values, every output word has exactly one writer, so the result is the
// same bit for bit whatever the launch shape.  The only device->host read of the whole operation is the caller's, of
// offset[N] (4 bytes).
#include <math.h>

#include "gcp_philox.hpp"
#include "gcp_tiles.hpp"

namespace {

using gcp::i64;

constexpr int kThreads = 256;
constexpr int kKeep = 0, kClone = 1, kSplit = 2;         // action[i]
constexpr int kSurvivor = 0, kFresh = 1, kChild = 2;     // kind[r]
constexpr int kNoSource = 255;                           // inside k_densify_rows: src_row[r] outside [0, N)

inline unsigned grid_for(i64 n) {
  const i64 b = (n + kThreads - 1) / kThreads;
  return (unsigned)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

// A Gaussian appears at most once in one camera's list (the projection emits each kept Gaussian once), so two entries of
// one call never share a destination: plain read-modify-write, no atomics, and the sums are reproducible.  An id outside
// [0, N) is never written through; it is counted in *n_bad where the caller asked for that.
__global__ __launch_bounds__(kThreads) void k_densify_accumulate(const float* __restrict__ grad_xy, const long long* __restrict__ index, i64 m,
                                                                  float scale_x, float scale_y, float* __restrict__ norm_acc,
                                                                  int* __restrict__ view_count, i64 N, int* __restrict__ n_bad) {
  for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < m; i += (i64)gridDim.x * kThreads) {
    const long long id = index[i];
    if (id < 0 || id >= N) {
      if (n_bad) atomicAdd(n_bad, 1);  // an integer count on the error path only
      continue;
    }
    if (!norm_acc) continue;  // the validation pass
    const float2 g = reinterpret_cast<const float2*>(grad_xy)[i];
    const float gx = g.x * scale_x, gy = g.y * scale_y;
    norm_acc[id] += sqrtf(gx * gx + gy * gy);
    view_count[id] += 1;
  }
}

struct PlanArgs {
  float grad_threshold, dense_extent, prune_extent, min_opacity, child_div;  // child_div = 0.8f * n_split
  int n_split;
};

__global__ __launch_bounds__(kThreads) void k_densify_plan(const float* __restrict__ norm_acc, const int* __restrict__ view_count,
                                                            const float* __restrict__ log_scale, const float* __restrict__ opacity_logit,
                                                            i64 N, PlanArgs a, int* __restrict__ count, unsigned char* __restrict__ action) {
  for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < N; i += (i64)gridDim.x * kThreads) {
    const int views = view_count[i];
    const float g = norm_acc[i] / (float)(views > 1 ? views : 1);
    const bool hot = views > 0 && g >= a.grad_threshold;
    const float s = fmaxf(fmaxf(expf(log_scale[3 * i]), expf(log_scale[3 * i + 1])), expf(log_scale[3 * i + 2]));
    int act = kKeep, rows = 1;
    float out_s = s;  // the largest scale of the rows the action writes
    if (hot && s > a.dense_extent) {
      act = kSplit, rows = a.n_split, out_s = s / a.child_div;
    } else if (hot) {
      act = kClone, rows = 2;
    }
    const float alpha = 1.0f / (1.0f + expf(-opacity_logit[i]));
    if (alpha < a.min_opacity || out_s > a.prune_extent) rows = 0;
    count[i] = rows;
    action[i] = (unsigned char)act;
  }
}

__global__ __launch_bounds__(kThreads) void k_densify_fill(const unsigned char* __restrict__ action, const int* __restrict__ offset, i64 N,
                                                            i64 M, int* __restrict__ src_row, unsigned char* __restrict__ kind) {
  for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < N; i += (i64)gridDim.x * kThreads) {
    const int r0 = offset[i];
    const i64 r1 = offset[i + 1] < M ? offset[i + 1] : M;  // an offset array that is not this plan's cannot write past the outputs
    const int act = action[i];
    for (int r = r0 < 0 ? 0 : r0; r < r1; ++r) {
      src_row[r] = (int)i;
      kind[r] = (unsigned char)(act == kSplit ? kChild : (act == kClone && r > r0 ? kFresh : kSurvivor));
    }
  }
}

// Output-driven: a block owns 256 consecutive output rows = one contiguous run of dst, written front to back by
// consecutive lanes.  VEC: W is a multiple of 4 and both arrays are 16-byte aligned, so every row of either side starts
// on a 16-byte boundary; otherwise (row widths 3, 27; a view at a 4-byte offset) single words.  MOMENTS: rows that are not
// survivors are written as 0.0f and their source is not read.
template <bool VEC, bool MOMENTS>
__global__ __launch_bounds__(kThreads) void k_densify_rows(const float* __restrict__ src, const int* __restrict__ src_row,
                                                            const unsigned char* __restrict__ kind, i64 N, i64 M, int W, float* __restrict__ dst) {
  __shared__ int s_src[kThreads];
  __shared__ unsigned char s_kind[kThreads];
  const i64 r0 = (i64)blockIdx.x * kThreads;
  const int rows = (int)(M - r0 < kThreads ? M - r0 : kThreads);
  if ((int)threadIdx.x < rows) {
    const int p = src_row[r0 + threadIdx.x];
    const bool ok = p >= 0 && p < N;  // a row without a source is written as zeros, never read
    s_src[threadIdx.x] = ok ? p : 0;
    s_kind[threadIdx.x] = ok ? kind[r0 + threadIdx.x] : (unsigned char)kNoSource;
  }
  __syncthreads();
  if (VEC) {
    const unsigned w4 = (unsigned)W >> 2, words = (unsigned)rows * w4;
    float4* d4 = reinterpret_cast<float4*>(dst) + r0 * w4;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    for (unsigned j = threadIdx.x; j < words; j += kThreads) {
      const unsigned r = j / w4, c = j - r * w4;
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (MOMENTS ? s_kind[r] == kSurvivor : s_kind[r] != kNoSource) v = s4[(i64)s_src[r] * w4 + c];
      d4[j] = v;
    }
  } else {
    const unsigned w = (unsigned)W, words = (unsigned)rows * w;
    float* d = dst + r0 * w;
    for (unsigned j = threadIdx.x; j < words; j += kThreads) {
      const unsigned r = j / w, c = j - r * w;
      float v = 0.0f;
      if (MOMENTS ? s_kind[r] == kSurvivor : s_kind[r] != kNoSource) v = src[(i64)s_src[r] * w + c];
      d[j] = v;
    }
  }
}

// One thread per output row; only split children do anything.  The child number is the row's place among its parent's
// rows (they are contiguous): r - offset[parent].  Every draw depends on (seed, parent, child) alone.
__global__ __launch_bounds__(kThreads) void k_densify_split(const float* __restrict__ mean, const float* __restrict__ quat,
                                                             const float* __restrict__ log_scale, const int* __restrict__ src_row,
                                                             const unsigned char* __restrict__ kind, const int* __restrict__ offset, i64 N, i64 M,
                                                             float child_div, unsigned seed_lo, unsigned seed_hi,
                                                             float* __restrict__ mean_out, float* __restrict__ log_scale_out) {
  for (i64 r = (i64)blockIdx.x * kThreads + threadIdx.x; r < M; r += (i64)gridDim.x * kThreads) {
    if (kind[r] != kChild) continue;
    const i64 p = src_row[r];
    if (p < 0 || p >= N) continue;
    const unsigned child = (unsigned)((int)r - offset[p]);
    unsigned rnd[4];
    gcp::philox4x32_10((unsigned)p, child, 0u, 0u, seed_lo, seed_hi, rnd);
    const float ra = sqrtf(-2.0f * gcp::log_unit_open(rnd[0])), rb = sqrtf(-2.0f * gcp::log_unit_open(rnd[2]));
    float sa, ca, sb, cb;
    sincosf(6.283185307179586f * gcp::unit_open(rnd[1]), &sa, &ca);
    sincosf(6.283185307179586f * gcp::unit_open(rnd[3]), &sb, &cb);
    (void)sb;
    const float sx = expf(log_scale[3 * p]), sy = expf(log_scale[3 * p + 1]), sz = expf(log_scale[3 * p + 2]);
    const float vx = sx * (ra * ca), vy = sy * (ra * sa), vz = sz * (rb * cb);  // sigma (.) z
    float rot[9];
    gcp::quat_rotation(quat[4 * p], quat[4 * p + 1], quat[4 * p + 2], quat[4 * p + 3], rot);
    mean_out[3 * r] = mean[3 * p] + (rot[0] * vx + rot[1] * vy + rot[2] * vz);
    mean_out[3 * r + 1] = mean[3 * p + 1] + (rot[3] * vx + rot[4] * vy + rot[5] * vz);
    mean_out[3 * r + 2] = mean[3 * p + 2] + (rot[6] * vx + rot[7] * vy + rot[8] * vz);
    log_scale_out[3 * r] = logf(sx / child_div);
    log_scale_out[3 * r + 1] = logf(sy / child_div);
    log_scale_out[3 * r + 2] = logf(sz / child_div);
  }
}

inline bool finite_f(float v) { return std::isfinite(v); }

}  // namespace

extern "C" int gcp_densify_accumulate(const float* grad_xy, const int64_t* index, int64_t m, float scale_x, float scale_y, float* norm_acc,
                                      int32_t* view_count, int64_t n_gauss, int32_t* n_bad, void* stream) {
  if (m < 0 || n_gauss < 0 || !finite_f(scale_x) || !finite_f(scale_y)) return GCP_ERR_INVALID_ARGUMENT;
  if (m == 0) return GCP_OK;
  const bool check_only = !norm_acc && !view_count && n_bad;  // count the ids outside [0, n_gauss), write nothing else
  if (!index || (!check_only && (!grad_xy || !norm_acc || !view_count))) return GCP_ERR_INVALID_ARGUMENT;
  if (!check_only && ((uintptr_t)grad_xy & 7)) return GCP_ERR_INVALID_ARGUMENT;  // rows are read as float2
  hipLaunchKernelGGL(k_densify_accumulate, dim3(grid_for(m)), dim3(kThreads), 0, (hipStream_t)stream, grad_xy, (const long long*)index, (i64)m,
                     scale_x, scale_y, norm_acc, (int*)view_count, (i64)n_gauss, (int*)n_bad);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

extern "C" size_t gcp_densify_plan_workspace_bytes(int64_t n_gauss) { return gcp_scan_i32_workspace_bytes(n_gauss > 0 ? n_gauss : 0); }

extern "C" int gcp_densify_plan(const float* norm_acc, const int32_t* view_count, const float* log_scale, const float* opacity_logit,
                                int64_t n_gauss, float grad_threshold, float dense_extent, float prune_extent, float min_opacity,
                                int32_t n_split, int32_t* count, uint8_t* action, int32_t* offset, void* ws, size_t ws_bytes, void* stream) {
  if (n_gauss < 0 || n_split < 1 || !finite_f(grad_threshold) || !finite_f(dense_extent) || !finite_f(prune_extent) || !finite_f(min_opacity))
    return GCP_ERR_INVALID_ARGUMENT;
  // the prefix sum is int32: refuse whatever COULD exceed it (a Gaussian writes at most max(n_split, 2) rows)
  if (n_gauss > (int64_t)INT32_MAX / (n_split > 2 ? n_split : 2)) return GCP_ERR_INVALID_ARGUMENT;
  if (!offset) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss > 0) {
    if (!norm_acc || !view_count || !log_scale || !opacity_logit || !count || !action || !ws) return GCP_ERR_INVALID_ARGUMENT;
    if (ws_bytes < gcp_densify_plan_workspace_bytes(n_gauss)) return GCP_ERR_WORKSPACE;
    const PlanArgs a{grad_threshold, dense_extent, prune_extent, min_opacity, 0.8f * (float)n_split, n_split};
    hipLaunchKernelGGL(k_densify_plan, dim3(grid_for(n_gauss)), dim3(kThreads), 0, (hipStream_t)stream, norm_acc, (const int*)view_count, log_scale,
                       opacity_logit, (i64)n_gauss, a, (int*)count, (unsigned char*)action);
    GCP_HIP(hipGetLastError());
  }
  return gcp::launch_excl_scan((const int*)count, (int*)offset, n_gauss, (int*)ws, (hipStream_t)stream);  // n_gauss == 0: offset[0] = 0
}

extern "C" int gcp_densify_fill(const uint8_t* action, const int32_t* offset, int64_t n_gauss, int64_t n_rows, int32_t* src_row, uint8_t* kind,
                                void* stream) {
  if (n_gauss < 0 || n_rows < 0 || n_rows > INT32_MAX) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0 || n_rows == 0) return GCP_OK;
  if (!action || !offset || !src_row || !kind) return GCP_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_densify_fill, dim3(grid_for(n_gauss)), dim3(kThreads), 0, (hipStream_t)stream, (const unsigned char*)action,
                     (const int*)offset, (i64)n_gauss, (i64)n_rows, (int*)src_row, (unsigned char*)kind);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

extern "C" int gcp_densify_rows(const float* src, int64_t n_src_rows, const int32_t* src_row, const uint8_t* kind, int64_t n_rows,
                                int32_t width, int32_t mode, float* dst, void* stream) {
  if (n_src_rows < 0 || n_rows < 0 || n_rows > INT32_MAX || width < 0 || width > (1 << 20) || (mode != 0 && mode != 1)) return GCP_ERR_INVALID_ARGUMENT;
  if (n_rows == 0 || width == 0) return GCP_OK;
  if (!src || !src_row || !kind || !dst || (((uintptr_t)src | (uintptr_t)dst) & 3)) return GCP_ERR_INVALID_ARGUMENT;
  const bool vec = (width & 3) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  const dim3 grid((unsigned)((n_rows + kThreads - 1) / kThreads)), block(kThreads);
  hipStream_t s = (hipStream_t)stream;
  const int* rows = (const int*)src_row;
  const unsigned char* k = (const unsigned char*)kind;
  if (vec && mode) hipLaunchKernelGGL((k_densify_rows<true, true>), grid, block, 0, s, src, rows, k, (i64)n_src_rows, (i64)n_rows, width, dst);
  else if (vec) hipLaunchKernelGGL((k_densify_rows<true, false>), grid, block, 0, s, src, rows, k, (i64)n_src_rows, (i64)n_rows, width, dst);
  else if (mode) hipLaunchKernelGGL((k_densify_rows<false, true>), grid, block, 0, s, src, rows, k, (i64)n_src_rows, (i64)n_rows, width, dst);
  else hipLaunchKernelGGL((k_densify_rows<false, false>), grid, block, 0, s, src, rows, k, (i64)n_src_rows, (i64)n_rows, width, dst);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

extern "C" int gcp_densify_split(const float* mean, const float* quat_xyzw, const float* log_scale, const int32_t* src_row, const uint8_t* kind,
                                 const int32_t* offset, int64_t n_gauss, int64_t n_rows, int32_t n_split, uint32_t seed_lo, uint32_t seed_hi, float* mean_out,
                                 float* log_scale_out, void* stream) {
  if (n_gauss < 0 || n_rows < 0 || n_rows > INT32_MAX || n_split < 1) return GCP_ERR_INVALID_ARGUMENT;
  if (n_rows == 0 || n_gauss == 0) return GCP_OK;
  if (!mean || !quat_xyzw || !log_scale || !src_row || !kind || !offset || !mean_out || !log_scale_out) return GCP_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_densify_split, dim3(grid_for(n_rows)), dim3(kThreads), 0, (hipStream_t)stream, mean, quat_xyzw, log_scale, (const int*)src_row,
                     (const unsigned char*)kind, (const int*)offset, (i64)n_gauss, (i64)n_rows, 0.8f * (float)n_split, (unsigned)seed_lo, (unsigned)seed_hi,
                     mean_out, log_scale_out);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}
