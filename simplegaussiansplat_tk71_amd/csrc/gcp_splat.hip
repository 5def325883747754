// gcp_splat.hip — the camera projection of gcp_project.hip with the three things other 3DGS renderers do differently, each
// opt-in and each with its exact gradient:
//   * FLOAT pixel centres.  gcp_project.hip truncates the projected centre to an integer pixel (the reference,
//     gs_model.py:293-294), so the blend's dL/dcentre has nowhere to go.  Here the centre stays a float, the gather hands it
//     to the blend as float [n][2], and the backward chains its gradient through px = ph0 / pz, py = ph1 / pz, ph = K t.
//     Pixel i of the cropped image is frame pixel i + 1 (the model crops [1:, 1:] of the (H+1) x (W+1) frame) and, in the
//     COLMAP / 3DGS convention, its centre lies at i + 0.5 in the coordinates of K: a centre stored as px + mean_offset with
//     mean_offset = 0.5 makes the blend's dx = (i + 1) - (px + 0.5) = (i + 0.5) - px, what those renderers evaluate.
//   * The box goes around the float centre: with h = min(3 sigma half extent, box_clamp), columns ceil(cx - h) .. floor(cx + h),
//     rows likewise — every pixel within the clamped 3-sigma extent and no other.  (A box centred on trunc(px) would cut a
//     pixel 1.2 sigma from the centre of a one-pixel Gaussian.)
//   * cov_eps, a run-time float, replaces the 1e-6 on the diagonal of the pixel covariance (0.3: the usual screen-space
//     dilation); det = a d - b c + 1e-6 stays.  The box half extents come from the dilated covariance.
//   * clamp_colour: l = max(SH sum, 0) per channel; a channel whose sum is < 0 passes no gradient (a sum of exactly 0 does).
// This file holds only the kernels and entry points: the bodies are those of gcp_project.hpp (project_fwd, project_gather,
// project_bwd) with SPLAT set, the ones gcp_project.hip instantiates without it.  So the structure is the same: one thread per
// Gaussian, 256-thread blocks, the parameter rows staged in LDS (10 + 3 n_basis floats per Gaussian: 37 888 B at 9 coefficients, four blocks per
// CU; 59 392 B at 16, two), one 64-byte record per Gaussian, the library's stable radix sort on the depth key between
// k_splat_fwd and k_splat_gather, -ffp-contract=off arithmetic in project_one's association.  Degree and SH frame are
// compile-time, as there; depth gradient, centre gradient and colour clamp are run-time (uniform branches: the register
// report of tests/test_splat_cabi.py stays under that file's bounds without more instantiations).
#include "gcp_project.hpp"

#include <cmath>

namespace {

// project_fwd of gcp_project.hpp in its SPLAT form
template <int MAXDEG, bool WORLD>
__global__ __launch_bounds__(kThreads) void k_splat_fwd(
    const float* __restrict__ mean, const float* __restrict__ q, const float* __restrict__ log_scale,
    const float* __restrict__ opacity, const float* __restrict__ color, const float* __restrict__ cam_P,
    const float* __restrict__ cam_K, i64 n, int sh_degree, int n_basis, int width, int height, float box_clamp, float cov_eps,
    float mean_offset, int flags, float4* __restrict__ record, int* __restrict__ sort_key, uint8_t* __restrict__ keep,
    int* __restrict__ row_of) {
  project_fwd<MAXDEG, WORLD, true>(mean, q, log_scale, opacity, color, cam_P, cam_K, n, sh_degree, n_basis, width, height, box_clamp,
                                   cov_eps, mean_offset, (flags & GCP_SPLAT_CLAMP_COLOUR) != 0, record, sort_key, keep, row_of,
                                   (flags & GCP_SPLAT_ANTIALIAS) != 0);
}

// project_gather with the centre as two floats; `depth` may be NULL
__global__ __launch_bounds__(kThreads) void k_splat_gather(
    const float4* __restrict__ record, const int* __restrict__ perm, i64 m, int* __restrict__ start_xy, int* __restrict__ end_xy,
    float* __restrict__ mean_xy, i64* __restrict__ boxsize, float* __restrict__ vinv, float* __restrict__ alpha,
    float* __restrict__ l_d, float* __restrict__ depth, i64* __restrict__ index, int* __restrict__ row_of,
    const unsigned char* __restrict__ keep) {
  project_gather<float2, GatherDepth::if_given>(record, perm, m, start_xy, end_xy, reinterpret_cast<float2*>(mean_xy), boxsize, vinv,
                                                alpha, l_d, depth, index, row_of, keep);
}

// The backward chain of gcp_project.hpp in its SPLAT form: g_depth and g_mean_xy may be NULL.
template <int MAXDEG, bool WORLD>
__global__ __launch_bounds__(kThreads) void k_splat_bwd(
    const float* __restrict__ mean, const float* __restrict__ q, const float* __restrict__ log_scale,
    const float* __restrict__ opacity, const float* __restrict__ color, const float* __restrict__ cam_P,
    const float* __restrict__ cam_K, i64 n, int sh_degree, int n_basis, const int* __restrict__ row_of,
    const float* __restrict__ g_vinv, const float* __restrict__ g_alpha, const float* __restrict__ g_ld,
    const float* __restrict__ g_depth, float cov_eps, int flags, const float* __restrict__ g_mean_xy,
    float* __restrict__ grad_mean, float* __restrict__ grad_q, float* __restrict__ grad_log_scale, float* __restrict__ grad_opacity,
    float* __restrict__ grad_color) {
  project_bwd<MAXDEG, WORLD, false, true>(mean, q, log_scale, opacity, color, cam_P, cam_K, n, sh_degree, n_basis, row_of, g_vinv,
                                          g_alpha, g_ld, g_depth, grad_mean, grad_q, grad_log_scale, grad_opacity, grad_color, cov_eps,
                                          (flags & GCP_SPLAT_CLAMP_COLOUR) != 0, g_mean_xy, (flags & GCP_SPLAT_ANTIALIAS) != 0);
}

bool splat_arguments_valid(float cov_eps, int32_t flags) {
  return std::isfinite(cov_eps) && cov_eps >= 0.f && (flags & ~(GCP_SPLAT_CLAMP_COLOUR | GCP_SPLAT_ANTIALIAS)) == 0;
}

}  // namespace

extern "C" {

int gcp_splat_forward_flags(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                            const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                            int32_t n_basis, int32_t sh_frame, int32_t width, int32_t height, float box_clamp, float cov_eps,
                            float mean_offset, int32_t flags, float* record, int32_t* sort_key, uint8_t* keep, int32_t* row_of,
                            void* stream) {
  const int rc = check_projection_call(
      n_gauss <= 0x7fffffff && width >= 0 && height >= 0 && splat_arguments_valid(cov_eps, flags) && std::isfinite(mean_offset),
      {mean, quat_xyzw, log_scale, opacity_logit, sh_coeff, cam_P, cam_K}, n_gauss, sh_degree, n_basis, sh_frame,
      {record, sort_key, keep, row_of});
  if (rc != kLaunch) return rc;
  if ((uintptr_t)record & 15) return GCP_ERR_INVALID_ARGUMENT;
  const size_t lds = stage_bytes(n_basis);
  auto kernel = pick_kernel(sh_degree, sh_frame, k_splat_fwd<2, false>, k_splat_fwd<2, true>, k_splat_fwd<3, false>, k_splat_fwd<3, true>);
  hipLaunchKernelGGL(kernel, dim3(grid_for(n_gauss)), dim3(kThreads), lds, (hipStream_t)stream, mean, quat_xyzw, log_scale,
                     opacity_logit, sh_coeff, cam_P, cam_K, (i64)n_gauss, (int)sh_degree, (int)n_basis, (int)width, (int)height,
                     box_clamp, cov_eps, mean_offset, (int)flags, (float4*)record, sort_key, keep, row_of);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int gcp_splat_forward(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                      const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                      int32_t n_basis, int32_t sh_frame, int32_t width, int32_t height, float box_clamp, float cov_eps,
                      float mean_offset, int32_t clamp_colour, float* record, int32_t* sort_key, uint8_t* keep, int32_t* row_of,
                      void* stream) {
  if (clamp_colour != 0 && clamp_colour != 1) return GCP_ERR_INVALID_ARGUMENT;  // a switch here, not a set of flags
  return gcp_splat_forward_flags(mean, quat_xyzw, log_scale, opacity_logit, sh_coeff, cam_P, cam_K, n_gauss, sh_degree, n_basis, sh_frame,
                                 width, height, box_clamp, cov_eps, mean_offset, clamp_colour ? GCP_SPLAT_CLAMP_COLOUR : 0, record,
                                 sort_key, keep, row_of, stream);
}

int gcp_splat_gather(const float* record, const int32_t* perm, int64_t n_kept, int32_t* start_xy, int32_t* end_xy, float* mean_xy,
                     int64_t* boxsize, float* vinv, float* alpha, float* l_d, float* depth, int64_t* index, int32_t* row_of,
                     const uint8_t* keep, void* stream) {
  if (n_kept < 0) return GCP_ERR_INVALID_ARGUMENT;
  if (n_kept == 0) return GCP_OK;
  if (!record || !perm || !start_xy || !end_xy || !mean_xy || !boxsize || !vinv || !alpha || !l_d || !index || !row_of ||
      (((uintptr_t)record | (uintptr_t)vinv) & 15) || (((uintptr_t)start_xy | (uintptr_t)end_xy | (uintptr_t)mean_xy) & 7))
    return GCP_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_splat_gather, dim3(grid_for(n_kept)), dim3(kThreads), 0, (hipStream_t)stream, (const float4*)record, perm,
                     (i64)n_kept, start_xy, end_xy, mean_xy, (i64*)boxsize, vinv, alpha, l_d, depth, (i64*)index, row_of,
                     (const unsigned char*)keep);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int gcp_splat_backward_flags(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                             const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                             int32_t n_basis, int32_t sh_frame, const int32_t* row_of, const float* grad_vinv,
                             const float* grad_alpha, const float* grad_l_d, const float* grad_depth, float cov_eps, int32_t flags,
                             const float* grad_mean_xy, float* grad_mean, float* grad_quat, float* grad_log_scale,
                             float* grad_opacity_logit, float* grad_sh_coeff, void* stream) {
  // the upstream arrays may be NULL when no Gaussian was kept
  const int rc = check_projection_call(splat_arguments_valid(cov_eps, flags), {mean, quat_xyzw, log_scale, opacity_logit, sh_coeff, cam_P, cam_K},
                                       n_gauss, sh_degree, n_basis, sh_frame,
                                       {row_of, grad_mean, grad_quat, grad_log_scale, grad_opacity_logit, grad_sh_coeff});
  if (rc != kLaunch) return rc;
  const size_t lds = stage_bytes(n_basis);
  auto kernel = pick_kernel(sh_degree, sh_frame, k_splat_bwd<2, false>, k_splat_bwd<2, true>, k_splat_bwd<3, false>, k_splat_bwd<3, true>);
  hipLaunchKernelGGL(kernel, dim3(grid_for(n_gauss)), dim3(kThreads), lds, (hipStream_t)stream, mean, quat_xyzw, log_scale,
                     opacity_logit, sh_coeff, cam_P, cam_K, (i64)n_gauss, (int)sh_degree, (int)n_basis, row_of, grad_vinv, grad_alpha,
                     grad_l_d, grad_depth, cov_eps, (int)flags, grad_mean_xy, grad_mean, grad_quat, grad_log_scale,
                     grad_opacity_logit, grad_sh_coeff);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int gcp_splat_backward(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                       const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                       int32_t n_basis, int32_t sh_frame, const int32_t* row_of, const float* grad_vinv, const float* grad_alpha,
                       const float* grad_l_d, const float* grad_depth, float cov_eps, int32_t clamp_colour, const float* grad_mean_xy,
                       float* grad_mean, float* grad_quat, float* grad_log_scale, float* grad_opacity_logit, float* grad_sh_coeff,
                       void* stream) {
  if (clamp_colour != 0 && clamp_colour != 1) return GCP_ERR_INVALID_ARGUMENT;
  return gcp_splat_backward_flags(mean, quat_xyzw, log_scale, opacity_logit, sh_coeff, cam_P, cam_K, n_gauss, sh_degree, n_basis, sh_frame,
                                  row_of, grad_vinv, grad_alpha, grad_l_d, grad_depth, cov_eps, clamp_colour ? GCP_SPLAT_CLAMP_COLOUR : 0,
                                  grad_mean_xy, grad_mean, grad_quat, grad_log_scale, grad_opacity_logit, grad_sh_coeff, stream);
}

}  // extern "C"
