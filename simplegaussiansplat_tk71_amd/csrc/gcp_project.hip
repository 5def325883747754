// gcp_project.hip — the caller's per-Gaussian camera projection, fused.
//
// reference: gs_model.py:277-425 (GS_model_with_param.forward up to the Function call): ~150 small PyTorch
// kernels, batched 3x3 matmuls and a CPU round trip for torch.linalg.eigh per step.  At N = 1e6 Gaussians that
// is 64 ms forward + 110 ms backward around a 1.8 ms rasterise-and-blend.  Here one thread owns one Gaussian:
// k_project_fwd writes, in the Gaussians' own order, everything the Function needs of it for one camera;
// k_project_bwd recomputes the chain in registers and turns (dL/dSigma'^-1, dL/dopacity, dL/dl_d) into the
// gradients of (mean, quaternion, log-scale, opacity logit, SH coefficients).  HBM bound: 152 B in, 77 B out per
// Gaussian forward at 9 SH coefficients; no cross-lane traffic.  Depth order: the forward also emits a 31-bit sort key
// per Gaussian (bits of the positive depth; culled last) for gcp_sort_pairs_u32, and k_project_gather unpacks the
// kept records in that order.
//
// Appearance: real spherical harmonics up to degree 3 in the usual 3DGS order and sign, evaluated on the direction
// -t/|t| in camera coordinates (the reference's call site, gs_model.py:335-338; the default) or on the world-space unit
// vector from the camera centre to the Gaussian, W^T t/|t| (sh_frame 1).  Both are compile-time: a 256-thread block
// stages 10 + 3 n_basis floats per Gaussian in LDS, 37 888 B at 9 coefficients (four blocks per CU, 4 waves per SIMD,
// <= 128 VGPRs) and 59 392 B at 16 (two blocks per CU, 2 waves per SIMD, <= 256 VGPRs) — so degree <= 2 in the camera
// frame runs the kernels it always ran (k_project_fwd, k_project_bwd, k_project_bwd_depth) and only degree 3 pays for the
// sixteen-term basis in registers (k_project_fwd_sh<3, *>, k_project_bwd_sh<3, *, *>).
//
// The arithmetic follows the reference's order of operations (matrix products accumulated left to right, k
// ascending, no FMA contraction: the library is built with -ffp-contract=off) so that the integer boxes that come
// out of float -> int32 truncation agree with the reference's.
#include "gcp_project.hpp"
#include "grouped_cumprod_hip.h"

namespace {

// Per Gaussian, one 64-byte record (what the gather reads back in one piece), the sort key of its depth and the cull flag.
//   record words: 0-3 box x0 y0 x1 y1 | 4-5 pixel mean | 6-9 Sigma'^-1 | 10 opacity | 11-13 colour | 14 camera depth | 15 unused

// MAXDEG: the highest SH degree the instantiation can evaluate (sh_degree <= MAXDEG is the caller's to ensure).
template <int MAXDEG, bool WORLD>
__device__ __forceinline__ void project_fwd(
    const float* __restrict__ mean, const float* __restrict__ q, const float* __restrict__ log_scale,
    const float* __restrict__ opacity, const float* __restrict__ color, const float* __restrict__ cam_P,
    const float* __restrict__ cam_K, i64 n, int sh_degree, int n_basis, int width, int height, float box_clamp,
    float4* __restrict__ record, int* __restrict__ sort_key, uint8_t* __restrict__ keep, int* __restrict__ row_of) {
  extern __shared__ float s_stage[];
  const ParamTile tile = param_tile(s_stage, n_basis);
  const Camera cam = load_camera(cam_P, cam_K);
  for (i64 base = (i64)blockIdx.x * kThreads; base < n; base += (i64)gridDim.x * kThreads) {
    const int cnt = (int)min((i64)kThreads, n - base);
    __syncthreads();  // the previous chunk's rows are no longer read
    load_param_tile(tile, mean, q, log_scale, color, base, cnt, n_basis);
    __syncthreads();
    const i64 i = base + threadIdx.x;
    if (i >= n) continue;
    Projected p;
    project_one(cam, tile.mean, tile.q, tile.ls, threadIdx.x, p);
    float hx, hy;
    box_halfsize(p.a, p.c, p.d, hx, hy);
    const float ilim = 2147483647.f / 1000.f;
    const int mx = trunc_i32(clampf(p.px, -ilim, ilim)), my = trunc_i32(clampf(p.py, -ilim, ilim));
    const int bw = trunc_i32(fminf(hx, box_clamp)), bh = trunc_i32(fminf(hy, box_clamp));
    const bool k = p.t[2] > 0.f && bw != 0 && mx - bw < width && mx + bw > 0 && my - bh < height && my + bh > 0;
    const int x0 = min(max(mx - bw, 0), width), y0 = min(max(my - bh, 0), height);
    const int x1 = min(max(mx + bw, 0), width), y1 = min(max(my + bh, 0), height);
    keep[i] = k ? 1 : 0;
    row_of[i] = -1;
    // kept depths are positive floats: their bit patterns sort like the values; culled Gaussians sort last
    sort_key[i] = k ? __float_as_int(p.t[2]) : 0x7fffffff;
    const float* sh = tile.sh + threadIdx.x * n_basis * 3;
    float dir[3];
    sh_direction<WORLD>(cam.P, p.view, dir);
    const float x = dir[0], y = dir[1], z = dir[2];
    float l[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) l[ch] = sh_colour<MAXDEG>(sh, ch, sh_degree, x, y, z);
    const float alpha = 1.f / (1.f + expf(-opacity[i]));
    float4* rec = record + 4 * i;
    rec[0] = make_float4(__int_as_float(x0), __int_as_float(y0), __int_as_float(x1), __int_as_float(y1));
    rec[1] = make_float4(__int_as_float(mx), __int_as_float(my), p.d / p.det, -p.b / p.det);
    rec[2] = make_float4(-p.c / p.det, p.a / p.det, alpha, l[0]);
    rec[3] = make_float4(l[1], l[2], p.t[2], 0.f);
  }
}

#define GCP_PROJECT_FWD_PARAMS                                                                                              \
  const float *__restrict__ mean, const float *__restrict__ q, const float *__restrict__ log_scale,                        \
      const float *__restrict__ opacity, const float *__restrict__ color, const float *__restrict__ cam_P,                 \
      const float *__restrict__ cam_K, i64 n, int sh_degree, int n_basis, int width, int height, float box_clamp,          \
      float4 *__restrict__ record, int *__restrict__ sort_key, uint8_t *__restrict__ keep, int *__restrict__ row_of
#define GCP_PROJECT_FWD_ARGS \
  mean, q, log_scale, opacity, color, cam_P, cam_K, n, sh_degree, n_basis, width, height, box_clamp, record, sort_key, keep, row_of

// degree <= 2 on the camera-frame direction: what every call ran before degree 3 and the world frame existed
__global__ __launch_bounds__(kThreads) void k_project_fwd(GCP_PROJECT_FWD_PARAMS) { project_fwd<2, false>(GCP_PROJECT_FWD_ARGS); }

// <2, true>: degree <= 2, world frame; <3, false> and <3, true>: degree 3
template <int MAXDEG, bool WORLD>
__global__ __launch_bounds__(kThreads) void k_project_fwd_sh(GCP_PROJECT_FWD_PARAMS) {
  project_fwd<MAXDEG, WORLD>(GCP_PROJECT_FWD_ARGS);
}

// Row r of the depth-ordered list is Gaussian perm[r]: unpack its record into the Function's argument arrays (DEPTH: and its
// camera depth, 0 for a culled one).
template <bool DEPTH>
__device__ __forceinline__ void project_gather(
    const float4* __restrict__ record, const int* __restrict__ perm, i64 m, int* __restrict__ start_xy,
    int* __restrict__ end_xy, int* __restrict__ mean_xy, i64* __restrict__ boxsize, float* __restrict__ vinv,
    float* __restrict__ alpha, float* __restrict__ l_d, float* __restrict__ depth, i64* __restrict__ index, int* __restrict__ row_of,
    const unsigned char* __restrict__ keep) {
  for (i64 r = (i64)blockIdx.x * kThreads + threadIdx.x; r < m; r += (i64)gridDim.x * kThreads) {
    const int i = perm[r];
    const float4* rec = record + 4 * (i64)i;
    const float4 a = rec[0], b = rec[1], c = rec[2], d = rec[3];
    int x0 = __float_as_int(a.x), y0 = __float_as_int(a.y), x1 = __float_as_int(a.z), y1 = __float_as_int(a.w);
    // `keep` given (the list holds ALL Gaussians, no kept count was read back): a culled one stays in the list behind
    // the kept ones with an EMPTY box — binned into no tile, blended nowhere, zero gradients (its row_of stays -1)
    const bool culled = keep != nullptr && keep[i] == 0;
    if (culled) { x0 = 1; y0 = 1; x1 = 0; y1 = 0; }
    reinterpret_cast<int2*>(start_xy)[r] = make_int2(x0, y0);
    reinterpret_cast<int2*>(end_xy)[r] = make_int2(x1, y1);
    reinterpret_cast<int2*>(mean_xy)[r] = make_int2(__float_as_int(b.x), __float_as_int(b.y));
    boxsize[r] = (i64)(x1 - x0 + 1) * (i64)(y1 - y0 + 1);
    reinterpret_cast<float4*>(vinv)[r] = make_float4(b.z, b.w, c.x, c.y);
    alpha[r] = c.z;
    l_d[3 * r] = c.w, l_d[3 * r + 1] = d.x, l_d[3 * r + 2] = d.y;
    if (DEPTH) depth[r] = culled ? 0.f : d.z;
    index[r] = i;
    if (!culled) row_of[i] = (int)r;
  }
}

__global__ __launch_bounds__(kThreads) void k_project_gather(
    const float4* __restrict__ record, const int* __restrict__ perm, i64 m, int* __restrict__ start_xy,
    int* __restrict__ end_xy, int* __restrict__ mean_xy, i64* __restrict__ boxsize, float* __restrict__ vinv,
    float* __restrict__ alpha, float* __restrict__ l_d, i64* __restrict__ index, int* __restrict__ row_of,
    const unsigned char* __restrict__ keep) {
  project_gather<false>(record, perm, m, start_xy, end_xy, mean_xy, boxsize, vinv, alpha, l_d, nullptr, index, row_of, keep);
}

__global__ __launch_bounds__(kThreads) void k_project_gather_depth(
    const float4* __restrict__ record, const int* __restrict__ perm, i64 m, int* __restrict__ start_xy,
    int* __restrict__ end_xy, int* __restrict__ mean_xy, i64* __restrict__ boxsize, float* __restrict__ vinv,
    float* __restrict__ alpha, float* __restrict__ l_d, float* __restrict__ depth, i64* __restrict__ index, int* __restrict__ row_of,
    const unsigned char* __restrict__ keep) {
  project_gather<true>(record, perm, m, start_xy, end_xy, mean_xy, boxsize, vinv, alpha, l_d, depth, index, row_of, keep);
}

#define GCP_PROJECT_BWD_PARAMS                                                                                              \
  const float *__restrict__ mean, const float *__restrict__ q, const float *__restrict__ log_scale,                        \
      const float *__restrict__ opacity, const float *__restrict__ color, const float *__restrict__ cam_P,                 \
      const float *__restrict__ cam_K, i64 n, int sh_degree, int n_basis, const int *__restrict__ row_of,                  \
      const float *__restrict__ g_vinv, const float *__restrict__ g_alpha, const float *__restrict__ g_ld
#define GCP_PROJECT_BWD_GRADS                                                                                               \
  float *__restrict__ grad_mean, float *__restrict__ grad_q, float *__restrict__ grad_log_scale,                           \
      float *__restrict__ grad_opacity, float *__restrict__ grad_color
#define GCP_PROJECT_BWD_ARGS mean, q, log_scale, opacity, color, cam_P, cam_K, n, sh_degree, n_basis, row_of, g_vinv, g_alpha, g_ld
#define GCP_PROJECT_BWD_GRAD_ARGS grad_mean, grad_q, grad_log_scale, grad_opacity, grad_color

// degree <= 2 on the camera-frame direction, without and with the depth gradient
__global__ __launch_bounds__(kThreads) void k_project_bwd(GCP_PROJECT_BWD_PARAMS, GCP_PROJECT_BWD_GRADS) {
  project_bwd<2, false, false>(GCP_PROJECT_BWD_ARGS, nullptr, GCP_PROJECT_BWD_GRAD_ARGS);
}

__global__ __launch_bounds__(kThreads) void k_project_bwd_depth(GCP_PROJECT_BWD_PARAMS, const float* __restrict__ g_depth,
                                                                GCP_PROJECT_BWD_GRADS) {
  project_bwd<2, false, true>(GCP_PROJECT_BWD_ARGS, g_depth, GCP_PROJECT_BWD_GRAD_ARGS);
}

// <2, true, *>: degree <= 2, world frame; <3, *, *>: degree 3
template <int MAXDEG, bool WORLD, bool DEPTH>
__global__ __launch_bounds__(kThreads) void k_project_bwd_sh(GCP_PROJECT_BWD_PARAMS, const float* __restrict__ g_depth,
                                                             GCP_PROJECT_BWD_GRADS) {
  project_bwd<MAXDEG, WORLD, DEPTH>(GCP_PROJECT_BWD_ARGS, g_depth, GCP_PROJECT_BWD_GRAD_ARGS);
}

int project_forward_call(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                         const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                         int32_t n_basis, int32_t sh_frame, int32_t width, int32_t height, float box_clamp, float* record,
                         int32_t* sort_key, uint8_t* keep, int32_t* row_of, void* stream) {
  if (n_gauss < 0 || n_gauss > 0x7fffffff || !sh_arguments_valid(sh_degree, n_basis, sh_frame) || width < 0 || height < 0)
    return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0) return GCP_OK;
  if (!mean || !quat_xyzw || !log_scale || !opacity_logit || !sh_coeff || !cam_P || !cam_K || !record || !sort_key || !keep ||
      !row_of || ((uintptr_t)record & 15))
    return GCP_ERR_INVALID_ARGUMENT;
  const size_t lds_fwd = (size_t)kThreads * (10 + 3 * (size_t)n_basis) * sizeof(float);
  if (lds_fwd > 64 * 1024) return GCP_ERR_INVALID_ARGUMENT;  // n_basis <= 18
  const bool deg3 = sh_degree > 2, world = sh_frame == 1;
  auto kernel = deg3 ? (world ? k_project_fwd_sh<3, true> : k_project_fwd_sh<3, false>) : (world ? k_project_fwd_sh<2, true> : k_project_fwd);
  hipLaunchKernelGGL(kernel, dim3(grid_for(n_gauss)), dim3(kThreads), lds_fwd, (hipStream_t)stream, mean, quat_xyzw, log_scale,
                     opacity_logit, sh_coeff, cam_P, cam_K, (i64)n_gauss, (int)sh_degree, (int)n_basis, (int)width, (int)height,
                     box_clamp, (float4*)record, sort_key, keep, row_of);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

}  // namespace

extern "C" {

int gcp_project_forward(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                        const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                        int32_t n_basis, int32_t width, int32_t height, float box_clamp, float* record, int32_t* sort_key,
                        uint8_t* keep, int32_t* row_of, void* stream) {
  return project_forward_call(mean, quat_xyzw, log_scale, opacity_logit, sh_coeff, cam_P, cam_K, n_gauss, sh_degree, n_basis, 0, width,
                              height, box_clamp, record, sort_key, keep, row_of, stream);
}

int gcp_project_forward_sh(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                           const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                           int32_t n_basis, int32_t sh_frame, int32_t width, int32_t height, float box_clamp, float* record,
                           int32_t* sort_key, uint8_t* keep, int32_t* row_of, void* stream) {
  return project_forward_call(mean, quat_xyzw, log_scale, opacity_logit, sh_coeff, cam_P, cam_K, n_gauss, sh_degree, n_basis, sh_frame,
                              width, height, box_clamp, record, sort_key, keep, row_of, stream);
}

}  // extern "C"

namespace {

int project_gather_call(const float* record, const int32_t* perm, int64_t n_kept, int32_t* start_xy, int32_t* end_xy,
                        int32_t* mean_xy, int64_t* boxsize, float* vinv, float* alpha, float* l_d, float* depth, bool with_depth,
                        int64_t* index, int32_t* row_of, const uint8_t* keep, void* stream) {
  if (n_kept < 0) return GCP_ERR_INVALID_ARGUMENT;
  if (n_kept == 0) return GCP_OK;
  if (!record || !perm || !start_xy || !end_xy || !mean_xy || !boxsize || !vinv || !alpha || !l_d || (with_depth && !depth) || !index ||
      !row_of || (((uintptr_t)record | (uintptr_t)vinv) & 15) || (((uintptr_t)start_xy | (uintptr_t)end_xy | (uintptr_t)mean_xy) & 7))
    return GCP_ERR_INVALID_ARGUMENT;
  if (with_depth)
    hipLaunchKernelGGL(k_project_gather_depth, dim3(grid_for(n_kept)), dim3(kThreads), 0, (hipStream_t)stream, (const float4*)record, perm,
                       (i64)n_kept, start_xy, end_xy, mean_xy, (i64*)boxsize, vinv, alpha, l_d, depth, (i64*)index, row_of,
                       (const unsigned char*)keep);
  else
    hipLaunchKernelGGL(k_project_gather, dim3(grid_for(n_kept)), dim3(kThreads), 0, (hipStream_t)stream, (const float4*)record, perm,
                       (i64)n_kept, start_xy, end_xy, mean_xy, (i64*)boxsize, vinv, alpha, l_d, (i64*)index, row_of,
                       (const unsigned char*)keep);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int project_backward_call(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                          const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                          int32_t n_basis, int32_t sh_frame, const int32_t* row_of, const float* grad_vinv, const float* grad_alpha,
                          const float* grad_l_d, const float* grad_depth, bool with_depth, float* grad_mean, float* grad_quat,
                          float* grad_log_scale, float* grad_opacity_logit, float* grad_sh_coeff, void* stream) {
  if (n_gauss < 0 || !sh_arguments_valid(sh_degree, n_basis, sh_frame)) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0) return GCP_OK;
  if (!mean || !quat_xyzw || !log_scale || !opacity_logit || !sh_coeff || !cam_P || !cam_K || !row_of || !grad_mean ||
      !grad_quat || !grad_log_scale || !grad_opacity_logit || !grad_sh_coeff)
    return GCP_ERR_INVALID_ARGUMENT;  // the upstream arrays may be NULL when no Gaussian was kept
  const size_t lds = (size_t)kThreads * (10 + 3 * (size_t)n_basis) * sizeof(float);
  if (lds > 64 * 1024) return GCP_ERR_INVALID_ARGUMENT;  // n_basis <= 18
  const dim3 grid(grid_for(n_gauss)), block(kThreads);
  const bool deg3 = sh_degree > 2, world = sh_frame == 1;
  if (!deg3 && !world) {
    if (with_depth)
      hipLaunchKernelGGL(k_project_bwd_depth, grid, block, lds, (hipStream_t)stream, mean, quat_xyzw, log_scale, opacity_logit, sh_coeff,
                         cam_P, cam_K, (i64)n_gauss, (int)sh_degree, (int)n_basis, row_of, grad_vinv, grad_alpha, grad_l_d, grad_depth,
                         grad_mean, grad_quat, grad_log_scale, grad_opacity_logit, grad_sh_coeff);
    else
      hipLaunchKernelGGL(k_project_bwd, grid, block, lds, (hipStream_t)stream, mean, quat_xyzw, log_scale, opacity_logit, sh_coeff, cam_P,
                         cam_K, (i64)n_gauss, (int)sh_degree, (int)n_basis, row_of, grad_vinv, grad_alpha, grad_l_d, grad_mean, grad_quat,
                         grad_log_scale, grad_opacity_logit, grad_sh_coeff);
  } else {
    auto kernel = deg3 ? (world ? (with_depth ? k_project_bwd_sh<3, true, true> : k_project_bwd_sh<3, true, false>)
                                : (with_depth ? k_project_bwd_sh<3, false, true> : k_project_bwd_sh<3, false, false>))
                       : (with_depth ? k_project_bwd_sh<2, true, true> : k_project_bwd_sh<2, true, false>);
    hipLaunchKernelGGL(kernel, grid, block, lds, (hipStream_t)stream, mean, quat_xyzw, log_scale, opacity_logit, sh_coeff, cam_P, cam_K,
                       (i64)n_gauss, (int)sh_degree, (int)n_basis, row_of, grad_vinv, grad_alpha, grad_l_d, grad_depth, grad_mean,
                       grad_quat, grad_log_scale, grad_opacity_logit, grad_sh_coeff);
  }
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

}  // namespace

extern "C" {

int gcp_project_gather(const float* record, const int32_t* perm, int64_t n_kept, int32_t* start_xy, int32_t* end_xy,
                       int32_t* mean_xy, int64_t* boxsize, float* vinv, float* alpha, float* l_d, int64_t* index,
                       int32_t* row_of, const uint8_t* keep, void* stream) {
  return project_gather_call(record, perm, n_kept, start_xy, end_xy, mean_xy, boxsize, vinv, alpha, l_d, nullptr, false, index, row_of,
                             keep, stream);
}

int gcp_project_gather_depth(const float* record, const int32_t* perm, int64_t n_kept, int32_t* start_xy, int32_t* end_xy,
                             int32_t* mean_xy, int64_t* boxsize, float* vinv, float* alpha, float* l_d, float* depth, int64_t* index,
                             int32_t* row_of, const uint8_t* keep, void* stream) {
  return project_gather_call(record, perm, n_kept, start_xy, end_xy, mean_xy, boxsize, vinv, alpha, l_d, depth, true, index, row_of,
                             keep, stream);
}

int gcp_project_backward(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                         const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                         int32_t n_basis, const int32_t* row_of, const float* grad_vinv, const float* grad_alpha,
                         const float* grad_l_d, float* grad_mean, float* grad_quat, float* grad_log_scale,
                         float* grad_opacity_logit, float* grad_sh_coeff, void* stream) {
  return project_backward_call(mean, quat_xyzw, log_scale, opacity_logit, sh_coeff, cam_P, cam_K, n_gauss, sh_degree, n_basis, 0, row_of,
                               grad_vinv, grad_alpha, grad_l_d, nullptr, false, grad_mean, grad_quat, grad_log_scale, grad_opacity_logit,
                               grad_sh_coeff, stream);
}

int gcp_project_backward_depth(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                               const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                               int32_t n_basis, const int32_t* row_of, const float* grad_vinv, const float* grad_alpha,
                               const float* grad_l_d, const float* grad_depth, float* grad_mean, float* grad_quat,
                               float* grad_log_scale, float* grad_opacity_logit, float* grad_sh_coeff, void* stream) {
  return project_backward_call(mean, quat_xyzw, log_scale, opacity_logit, sh_coeff, cam_P, cam_K, n_gauss, sh_degree, n_basis, 0, row_of,
                               grad_vinv, grad_alpha, grad_l_d, grad_depth, true, grad_mean, grad_quat, grad_log_scale,
                               grad_opacity_logit, grad_sh_coeff, stream);
}

int gcp_project_backward_sh(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                            const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                            int32_t n_basis, int32_t sh_frame, const int32_t* row_of, const float* grad_vinv, const float* grad_alpha,
                            const float* grad_l_d, const float* grad_depth, float* grad_mean, float* grad_quat,
                            float* grad_log_scale, float* grad_opacity_logit, float* grad_sh_coeff, void* stream) {
  return project_backward_call(mean, quat_xyzw, log_scale, opacity_logit, sh_coeff, cam_P, cam_K, n_gauss, sh_degree, n_basis, sh_frame,
                               row_of, grad_vinv, grad_alpha, grad_l_d, grad_depth, grad_depth != nullptr, grad_mean, grad_quat,
                               grad_log_scale, grad_opacity_logit, grad_sh_coeff, stream);
}

}  // extern "C"
