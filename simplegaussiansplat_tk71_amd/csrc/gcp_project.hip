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
//
// This file holds only the kernels and entry points.  The bodies (project_fwd, project_gather, project_bwd) and the checks
// the entry points share are in gcp_project.hpp, which gcp_splat.hip instantiates a second time with its SPLAT switch set.
#include "gcp_project.hpp"

namespace {

#define GCP_PROJECT_FWD_PARAMS                                                                                              \
  const float *__restrict__ mean, const float *__restrict__ q, const float *__restrict__ log_scale,                        \
      const float *__restrict__ opacity, const float *__restrict__ color, const float *__restrict__ cam_P,                 \
      const float *__restrict__ cam_K, i64 n, int sh_degree, int n_basis, int width, int height, float box_clamp,          \
      float4 *__restrict__ record, int *__restrict__ sort_key, uint8_t *__restrict__ keep, int *__restrict__ row_of
// project_fwd without SPLAT: 1e-6 on the covariance's diagonal, no offset, no colour clamp
#define GCP_PROJECT_FWD_ARGS                                                                                                 \
  mean, q, log_scale, opacity, color, cam_P, cam_K, n, sh_degree, n_basis, width, height, box_clamp, 1e-6f, 0.f, false, record, sort_key, \
      keep, row_of

// degree <= 2 on the camera-frame direction: what every call ran before degree 3 and the world frame existed
__global__ __launch_bounds__(kThreads) void k_project_fwd(GCP_PROJECT_FWD_PARAMS) { project_fwd<2, false, false>(GCP_PROJECT_FWD_ARGS); }

// <2, true>: degree <= 2, world frame; <3, false> and <3, true>: degree 3
template <int MAXDEG, bool WORLD>
__global__ __launch_bounds__(kThreads) void k_project_fwd_sh(GCP_PROJECT_FWD_PARAMS) {
  project_fwd<MAXDEG, WORLD, false>(GCP_PROJECT_FWD_ARGS);
}

__global__ __launch_bounds__(kThreads) void k_project_gather(
    const float4* __restrict__ record, const int* __restrict__ perm, i64 m, int* __restrict__ start_xy,
    int* __restrict__ end_xy, int* __restrict__ mean_xy, i64* __restrict__ boxsize, float* __restrict__ vinv,
    float* __restrict__ alpha, float* __restrict__ l_d, i64* __restrict__ index, int* __restrict__ row_of,
    const unsigned char* __restrict__ keep) {
  project_gather<int2, GatherDepth::no>(record, perm, m, start_xy, end_xy, reinterpret_cast<int2*>(mean_xy), boxsize, vinv, alpha, l_d,
                                        nullptr, index, row_of, keep);
}

__global__ __launch_bounds__(kThreads) void k_project_gather_depth(
    const float4* __restrict__ record, const int* __restrict__ perm, i64 m, int* __restrict__ start_xy,
    int* __restrict__ end_xy, int* __restrict__ mean_xy, i64* __restrict__ boxsize, float* __restrict__ vinv,
    float* __restrict__ alpha, float* __restrict__ l_d, float* __restrict__ depth, i64* __restrict__ index, int* __restrict__ row_of,
    const unsigned char* __restrict__ keep) {
  project_gather<int2, GatherDepth::yes>(record, perm, m, start_xy, end_xy, reinterpret_cast<int2*>(mean_xy), boxsize, vinv, alpha, l_d,
                                         depth, index, row_of, keep);
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
  const int rc = check_projection_call(n_gauss <= 0x7fffffff && width >= 0 && height >= 0,
                                       {mean, quat_xyzw, log_scale, opacity_logit, sh_coeff, cam_P, cam_K}, n_gauss, sh_degree, n_basis,
                                       sh_frame, {record, sort_key, keep, row_of});
  if (rc != kLaunch) return rc;
  if ((uintptr_t)record & 15) return GCP_ERR_INVALID_ARGUMENT;
  auto kernel = pick_kernel(sh_degree, sh_frame, k_project_fwd, k_project_fwd_sh<2, true>, k_project_fwd_sh<3, false>,
                            k_project_fwd_sh<3, true>);
  hipLaunchKernelGGL(kernel, dim3(grid_for(n_gauss)), dim3(kThreads), stage_bytes(n_basis), (hipStream_t)stream, mean, quat_xyzw,
                     log_scale, opacity_logit, sh_coeff, cam_P, cam_K, (i64)n_gauss, (int)sh_degree, (int)n_basis, (int)width,
                     (int)height, box_clamp, (float4*)record, sort_key, keep, row_of);
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
  // the upstream arrays may be NULL when no Gaussian was kept
  const int rc = check_projection_call(true, {mean, quat_xyzw, log_scale, opacity_logit, sh_coeff, cam_P, cam_K}, n_gauss, sh_degree,
                                       n_basis, sh_frame, {row_of, grad_mean, grad_quat, grad_log_scale, grad_opacity_logit, grad_sh_coeff});
  if (rc != kLaunch) return rc;
  const dim3 grid(grid_for(n_gauss)), block(kThreads);
  const size_t lds = stage_bytes(n_basis);
  if (sh_degree <= 2 && sh_frame == 0 && !with_depth) {  // the one kernel without the g_depth argument
    hipLaunchKernelGGL(k_project_bwd, grid, block, lds, (hipStream_t)stream, mean, quat_xyzw, log_scale, opacity_logit, sh_coeff, cam_P,
                       cam_K, (i64)n_gauss, (int)sh_degree, (int)n_basis, row_of, grad_vinv, grad_alpha, grad_l_d, grad_mean, grad_quat,
                       grad_log_scale, grad_opacity_logit, grad_sh_coeff);
  } else {
    auto kernel = pick_kernel(sh_degree, sh_frame, k_project_bwd_depth,  // degree <= 2, camera frame: here only with depth
                              with_depth ? k_project_bwd_sh<2, true, true> : k_project_bwd_sh<2, true, false>,
                              with_depth ? k_project_bwd_sh<3, false, true> : k_project_bwd_sh<3, false, false>,
                              with_depth ? k_project_bwd_sh<3, true, true> : k_project_bwd_sh<3, true, false>);
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
