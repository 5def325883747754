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
// Same structure as gcp_project.hip, whose device code it shares (gcp_project.hpp): one thread per Gaussian, 256-thread
// blocks, the parameter rows staged in LDS (10 + 3 n_basis floats per Gaussian: 37 888 B at 9 coefficients, four blocks per
// CU; 59 392 B at 16, two), one 64-byte record per Gaussian, the library's stable radix sort on the depth key between
// k_splat_fwd and k_splat_gather, -ffp-contract=off arithmetic in project_one's association.  Degree and SH frame are
// compile-time, as there; depth gradient, centre gradient and colour clamp are run-time (uniform branches: the register
// report of tests/test_splat_cabi.py stays under that file's bounds without more instantiations).
#include "gcp_project.hpp"
#include "grouped_cumprod_hip.h"

#include <cmath>

namespace {

//   record words: 0-3 box x0 y0 x1 y1 | 4-5 pixel centre (float) | 6-9 Sigma'^-1 | 10 opacity | 11-13 colour | 14 camera depth | 15 unused
template <int MAXDEG, bool WORLD>
__global__ __launch_bounds__(kThreads) void k_splat_fwd(
    const float* __restrict__ mean, const float* __restrict__ q, const float* __restrict__ log_scale,
    const float* __restrict__ opacity, const float* __restrict__ color, const float* __restrict__ cam_P,
    const float* __restrict__ cam_K, i64 n, int sh_degree, int n_basis, int width, int height, float box_clamp, float cov_eps,
    float mean_offset, int clamp_colour, float4* __restrict__ record, int* __restrict__ sort_key, uint8_t* __restrict__ keep,
    int* __restrict__ row_of) {
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
    project_one(cam, tile.mean, tile.q, tile.ls, threadIdx.x, p, cov_eps);
    float hx, hy;
    box_halfsize(p.a, p.c, p.d, hx, hy);
    const float ilim = 2147483647.f / 1000.f;
    const float cx = clampf(p.px, -ilim, ilim) + mean_offset, cy = clampf(p.py, -ilim, ilim) + mean_offset;
    const float bw = fminf(hx, box_clamp), bh = fminf(hy, box_clamp);
    // clamped before conversion: every operand of the tests below is a valid int32 (a NaN extent clamps to +-ilim)
    const int bx0 = (int)ceilf(clampf(cx - bw, -ilim, ilim)), bx1 = (int)floorf(clampf(cx + bw, -ilim, ilim));
    const int by0 = (int)ceilf(clampf(cy - bh, -ilim, ilim)), by1 = (int)floorf(clampf(cy + bh, -ilim, ilim));
    const bool k = p.t[2] > 0.f && bx1 >= bx0 && by1 >= by0 && bx0 < width && bx1 > 0 && by0 < height && by1 > 0;
    const int x0 = min(max(bx0, 0), width), y0 = min(max(by0, 0), height);
    const int x1 = min(max(bx1, 0), width), y1 = min(max(by1, 0), height);
    keep[i] = k ? 1 : 0;
    row_of[i] = -1;
    // kept depths are positive floats: their bit patterns sort like the values; culled Gaussians sort last
    sort_key[i] = k ? __float_as_int(p.t[2]) : 0x7fffffff;
    const float* sh = tile.sh + threadIdx.x * n_basis * 3;
    float dir[3];
    sh_direction<WORLD>(cam.P, p.view, dir);
    float l[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      l[ch] = sh_colour<MAXDEG>(sh, ch, sh_degree, dir[0], dir[1], dir[2]);
      if (clamp_colour && l[ch] < 0.f) l[ch] = 0.f;  // the test the backward repeats on the same sum
    }
    const float alpha = 1.f / (1.f + expf(-opacity[i]));
    float4* rec = record + 4 * i;
    rec[0] = make_float4(__int_as_float(x0), __int_as_float(y0), __int_as_float(x1), __int_as_float(y1));
    rec[1] = make_float4(cx, cy, p.d / p.det, -p.b / p.det);
    rec[2] = make_float4(-p.c / p.det, p.a / p.det, alpha, l[0]);
    rec[3] = make_float4(l[1], l[2], p.t[2], 0.f);
  }
}

// Row r of the depth-ordered list is Gaussian perm[r]: unpack its record into the Function's argument arrays, the centre as
// two floats; `depth` (may be NULL): its camera depth too, 0 for a culled one.
__global__ __launch_bounds__(kThreads) void k_splat_gather(
    const float4* __restrict__ record, const int* __restrict__ perm, i64 m, int* __restrict__ start_xy, int* __restrict__ end_xy,
    float* __restrict__ mean_xy, i64* __restrict__ boxsize, float* __restrict__ vinv, float* __restrict__ alpha,
    float* __restrict__ l_d, float* __restrict__ depth, i64* __restrict__ index, int* __restrict__ row_of,
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
    reinterpret_cast<float2*>(mean_xy)[r] = make_float2(b.x, b.y);  // finite for every Gaussian: clamped before the offset
    boxsize[r] = (i64)(x1 - x0 + 1) * (i64)(y1 - y0 + 1);
    reinterpret_cast<float4*>(vinv)[r] = make_float4(b.z, b.w, c.x, c.y);
    alpha[r] = c.z;
    l_d[3 * r] = c.w, l_d[3 * r + 1] = d.x, l_d[3 * r + 2] = d.y;
    if (depth != nullptr) depth[r] = culled ? 0.f : d.z;
    index[r] = i;
    if (!culled) row_of[i] = (int)r;
  }
}

// The backward chain of gcp_project.hpp in its SPLAT form: g_depth and g_mean_xy may be NULL.
template <int MAXDEG, bool WORLD>
__global__ __launch_bounds__(kThreads) void k_splat_bwd(
    const float* __restrict__ mean, const float* __restrict__ q, const float* __restrict__ log_scale,
    const float* __restrict__ opacity, const float* __restrict__ color, const float* __restrict__ cam_P,
    const float* __restrict__ cam_K, i64 n, int sh_degree, int n_basis, const int* __restrict__ row_of,
    const float* __restrict__ g_vinv, const float* __restrict__ g_alpha, const float* __restrict__ g_ld,
    const float* __restrict__ g_depth, float cov_eps, int clamp_colour, const float* __restrict__ g_mean_xy,
    float* __restrict__ grad_mean, float* __restrict__ grad_q, float* __restrict__ grad_log_scale, float* __restrict__ grad_opacity,
    float* __restrict__ grad_color) {
  project_bwd<MAXDEG, WORLD, false, true>(mean, q, log_scale, opacity, color, cam_P, cam_K, n, sh_degree, n_basis, row_of, g_vinv,
                                          g_alpha, g_ld, g_depth, grad_mean, grad_q, grad_log_scale, grad_opacity, grad_color, cov_eps,
                                          clamp_colour != 0, g_mean_xy);
}

bool splat_arguments_valid(float cov_eps, int32_t clamp_colour) {
  return std::isfinite(cov_eps) && cov_eps >= 0.f && (clamp_colour == 0 || clamp_colour == 1);
}

size_t stage_bytes(int32_t n_basis) { return (size_t)kThreads * (10 + 3 * (size_t)n_basis) * sizeof(float); }

}  // namespace

extern "C" {

int gcp_splat_forward(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                      const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                      int32_t n_basis, int32_t sh_frame, int32_t width, int32_t height, float box_clamp, float cov_eps,
                      float mean_offset, int32_t clamp_colour, float* record, int32_t* sort_key, uint8_t* keep, int32_t* row_of,
                      void* stream) {
  if (n_gauss < 0 || n_gauss > 0x7fffffff || !sh_arguments_valid(sh_degree, n_basis, sh_frame) || width < 0 || height < 0 ||
      !splat_arguments_valid(cov_eps, clamp_colour) || !std::isfinite(mean_offset))
    return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0) return GCP_OK;
  if (!mean || !quat_xyzw || !log_scale || !opacity_logit || !sh_coeff || !cam_P || !cam_K || !record || !sort_key || !keep ||
      !row_of || ((uintptr_t)record & 15))
    return GCP_ERR_INVALID_ARGUMENT;
  const size_t lds = stage_bytes(n_basis);
  if (lds > 64 * 1024) return GCP_ERR_INVALID_ARGUMENT;  // n_basis <= 18
  const bool deg3 = sh_degree > 2, world = sh_frame == 1;
  auto kernel = deg3 ? (world ? k_splat_fwd<3, true> : k_splat_fwd<3, false>) : (world ? k_splat_fwd<2, true> : k_splat_fwd<2, false>);
  hipLaunchKernelGGL(kernel, dim3(grid_for(n_gauss)), dim3(kThreads), lds, (hipStream_t)stream, mean, quat_xyzw, log_scale,
                     opacity_logit, sh_coeff, cam_P, cam_K, (i64)n_gauss, (int)sh_degree, (int)n_basis, (int)width, (int)height,
                     box_clamp, cov_eps, mean_offset, (int)clamp_colour, (float4*)record, sort_key, keep, row_of);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
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

int gcp_splat_backward(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                       const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                       int32_t n_basis, int32_t sh_frame, const int32_t* row_of, const float* grad_vinv, const float* grad_alpha,
                       const float* grad_l_d, const float* grad_depth, float cov_eps, int32_t clamp_colour, const float* grad_mean_xy,
                       float* grad_mean, float* grad_quat, float* grad_log_scale, float* grad_opacity_logit, float* grad_sh_coeff,
                       void* stream) {
  if (n_gauss < 0 || !sh_arguments_valid(sh_degree, n_basis, sh_frame) || !splat_arguments_valid(cov_eps, clamp_colour))
    return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0) return GCP_OK;
  if (!mean || !quat_xyzw || !log_scale || !opacity_logit || !sh_coeff || !cam_P || !cam_K || !row_of || !grad_mean ||
      !grad_quat || !grad_log_scale || !grad_opacity_logit || !grad_sh_coeff)
    return GCP_ERR_INVALID_ARGUMENT;  // the upstream arrays may be NULL when no Gaussian was kept
  const size_t lds = stage_bytes(n_basis);
  if (lds > 64 * 1024) return GCP_ERR_INVALID_ARGUMENT;  // n_basis <= 18
  const bool deg3 = sh_degree > 2, world = sh_frame == 1;
  auto kernel = deg3 ? (world ? k_splat_bwd<3, true> : k_splat_bwd<3, false>) : (world ? k_splat_bwd<2, true> : k_splat_bwd<2, false>);
  hipLaunchKernelGGL(kernel, dim3(grid_for(n_gauss)), dim3(kThreads), lds, (hipStream_t)stream, mean, quat_xyzw, log_scale,
                     opacity_logit, sh_coeff, cam_P, cam_K, (i64)n_gauss, (int)sh_degree, (int)n_basis, row_of, grad_vinv, grad_alpha,
                     grad_l_d, grad_depth, cov_eps, (int)clamp_colour, grad_mean_xy, grad_mean, grad_quat, grad_log_scale,
                     grad_opacity_logit, grad_sh_coeff);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

}  // extern "C"
