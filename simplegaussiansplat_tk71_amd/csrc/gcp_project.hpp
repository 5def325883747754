// gcp_project.hpp — the per-Gaussian camera projection, written once for its two families of kernels: gcp_project.hip
// (integer centres, the reference's conventions) and gcp_splat.hip (float centres, covariance dilation, colour clamp).
// Device side: the camera, the chain of one Gaussian (project_one), the LDS staging of the parameter rows, the 3-sigma box,
// the SH colour, and the three bodies — project_fwd, project_gather, project_bwd — in which the compile-time switch SPLAT
// selects the few lines the families differ in.  Host side: the checks and the kernel pick their entry points share.
// Every function is inlined into the kernels and entry points of the including file; nothing here is a kernel.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "gcp_device.hpp"
#include "grouped_cumprod_hip.h"

namespace {

using gcp::i64;

constexpr int kThreads = 256;
constexpr float kShC0 = 0.28209479177387814f;
constexpr float kShC1 = 0.4886025119029199f;
constexpr float kShC2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f,
                            0.5462742152960396f};
constexpr float kShC3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                            -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f};

struct Camera {
  float P[12];  // world -> camera [R|t], row major 3x4
  float K[9];   // intrinsics, row major 3x3
};

__device__ __forceinline__ Camera load_camera(const float* __restrict__ P, const float* __restrict__ K) {
  Camera c;
#pragma unroll
  for (int i = 0; i < 12; ++i) c.P[i] = P[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) c.K[i] = K[i];
  return c;
}

// Everything between the parameters of one Gaussian and the arguments of the Function.  cov_eps: what is added to the
// diagonal of the pixel covariance (1e-6, the reference's; gcp_splat.hip passes the caller's dilation).
struct Projected {
  float t[3];        // mean in camera coordinates (gs_model.py:289-290)
  float px, py;      // pixel mean before truncation (:293-294)
  float qn[4], qlen; // unit quaternion (x, y, z, w) and the clamped norm (:297)
  float R[9];        // rotation (:299)
  float s[3];        // exp(log scale) (:302)
  float S[9];        // covariance, world (:307)
  float Sc[9];       // covariance, camera (:309)
  float J[6];        // 2x3 Jacobian (:311)
  float cov[4];      // pixel covariance before the clamp (:321)
  float a, b, c, d;  // pixel covariance after clamp + cov_eps I
  float det;         // a d - b c + 1e-6 (uitility.py:447-451)
  float view[3], tlen;  // direction towards the camera (:337)
};

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// Opacity compensation of the dilation (gcp_splat.hip, `antialias`): Sigma' = Sigma + cov_eps I spreads a Gaussian over more
// pixels than Sigma does, so its opacity is scaled by rho = sqrt(det Sigma / det Sigma') and the energy it paints,
// 2 pi alpha rho sqrt(det Sigma'), is that of the Gaussian before the dilation.  det0 = a0 d0 - b c on the clamped entries
// before cov_eps; the denominator is p.det, 1e-6 included: the determinant Sigma'^-1 = adj / det is formed with.
// det0 <= 0 (a covariance that underflowed, or lost its rank to rounding): rho = 0, and nothing passes through it.
struct Compensation {
  float a0, d0;     // clamped diagonal before cov_eps
  float rho;        // sqrt(max(det0, 0) / det)
  float rho_det0;   // rho / det0 = 1 / (sqrt(det0) sqrt(det)), finite for every positive det0; 0 where det0 <= 0
};

__device__ __forceinline__ Compensation compensation(const Projected& p) {
  const float lim = 3.4028234663852886e+38f / 1000.f;
  Compensation k;
  k.a0 = clampf(p.cov[0], -lim, lim);
  k.d0 = clampf(p.cov[3], -lim, lim);
  const float det0 = k.a0 * k.d0 - p.b * p.c;
  k.rho = sqrtf(fmaxf(det0, 0.f) / p.det);
  k.rho_det0 = det0 > 0.f ? 1.f / (sqrtf(det0) * sqrtf(p.det)) : 0.f;
  return k;
}

// The direction the SH basis is evaluated on.  Camera frame: `view` itself.  World frame: W = P[:, :3] is orthonormal and
// t = W (m - c), so the unit vector from the camera centre c to the Gaussian is W^T t / |t| = -W^T view.
template <bool WORLD>
__device__ __forceinline__ void sh_direction(const float* __restrict__ P, const float* __restrict__ view, float* __restrict__ dir) {
#pragma unroll
  for (int k = 0; k < 3; ++k) dir[k] = WORLD ? -((P[k] * view[0] + P[4 + k] * view[1]) + P[8 + k] * view[2]) : view[k];
}

__device__ __forceinline__ void project_one(const Camera& cam, const float* __restrict__ mean, const float* __restrict__ q,
                                            const float* __restrict__ log_scale, i64 i, Projected& o,
                                            float cov_eps = 1e-6f) {
  const float m0 = mean[3 * i], m1 = mean[3 * i + 1], m2 = mean[3 * i + 2];
#pragma unroll
  for (int j = 0; j < 3; ++j)
    o.t[j] = ((m0 * cam.P[4 * j] + m1 * cam.P[4 * j + 1]) + m2 * cam.P[4 * j + 2]) + cam.P[4 * j + 3];
  float ph[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) ph[j] = (o.t[0] * cam.K[3 * j] + o.t[1] * cam.K[3 * j + 1]) + o.t[2] * cam.K[3 * j + 2];
  const float pz = fmaxf(ph[2], 1e-2f);
  o.px = ph[0] / pz;
  o.py = ph[1] / pz;

  const float qx = q[4 * i], qy = q[4 * i + 1], qz = q[4 * i + 2], qw = q[4 * i + 3];
  o.qlen = fmaxf(sqrtf(((qx * qx + qy * qy) + qz * qz) + qw * qw), 1e-8f);
  const float x = qx / o.qlen, y = qy / o.qlen, z = qz / o.qlen, w = qw / o.qlen;
  o.qn[0] = x, o.qn[1] = y, o.qn[2] = z, o.qn[3] = w;
  float* R = o.R;
  R[0] = 1 - 2 * (y * y + z * z), R[1] = 2 * (x * y - w * z), R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z), R[4] = 1 - 2 * (x * x + z * z), R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y), R[7] = 2 * (y * z + w * x), R[8] = 1 - 2 * (x * x + y * y);
#pragma unroll
  for (int k = 0; k < 3; ++k) o.s[k] = expf(log_scale[3 * i + k]);
  // R diag(s) diag(s)^T R^T, left to right
  float B[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) B[3 * r + k] = (R[3 * r + k] * o.s[k]) * o.s[k];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) o.S[3 * r + c] = (B[3 * r] * R[3 * c] + B[3 * r + 1] * R[3 * c + 1]) + B[3 * r + 2] * R[3 * c + 2];
  // W S W^T with W = P[:, :3]
  float WS[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      WS[3 * r + c] = (cam.P[4 * r] * o.S[c] + cam.P[4 * r + 1] * o.S[3 + c]) + cam.P[4 * r + 2] * o.S[6 + c];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      o.Sc[3 * r + c] = (WS[3 * r] * cam.P[4 * c] + WS[3 * r + 1] * cam.P[4 * c + 1]) + WS[3 * r + 2] * cam.P[4 * c + 2];
  // Jacobian of the pinhole projection (uitility.py:257-287)
  const float fx = cam.K[0], fy = cam.K[4];
  const float zc = fmaxf(o.t[2], 1e-2f);
  float* J = o.J;
  J[0] = fx / zc, J[1] = 0.f, J[2] = -fx * o.t[0] / (zc * zc);
  J[3] = 0.f, J[4] = fy / zc, J[5] = -fy * o.t[1] / (zc * zc);
  float JS[6];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) JS[3 * r + c] = (J[3 * r] * o.Sc[c] + J[3 * r + 1] * o.Sc[3 + c]) + J[3 * r + 2] * o.Sc[6 + c];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c) o.cov[2 * r + c] = (JS[3 * r] * J[3 * c] + JS[3 * r + 1] * J[3 * c + 1]) + JS[3 * r + 2] * J[3 * c + 2];
  const float lim = 3.4028234663852886e+38f / 1000.f;
  o.a = clampf(o.cov[0], -lim, lim) + cov_eps;
  o.b = clampf(o.cov[1], -lim, lim);
  o.c = clampf(o.cov[2], -lim, lim);
  o.d = clampf(o.cov[3], -lim, lim) + cov_eps;
  o.det = (o.a * o.d - o.b * o.c) + 1e-6f;
  o.tlen = fmaxf(sqrtf((o.t[0] * o.t[0] + o.t[1] * o.t[1]) + o.t[2] * o.t[2]), 1e-8f);
#pragma unroll
  for (int k = 0; k < 3; ++k) o.view[k] = -o.t[k] / o.tlen;
}

// The parameter rows of a block's 256 consecutive Gaussians, copied into LDS with contiguous 16-byte loads: read
// straight from global memory they are 37 four-byte loads per thread, 12-108 bytes apart between neighbouring lanes.
// Layout: mean [256][3] | quaternion [256][4] | log scale [256][3] | SH [256][3 n_basis].
struct ParamTile {
  float *mean, *q, *ls, *sh;
};

__device__ __forceinline__ ParamTile param_tile(float* base, int n_basis) {
  ParamTile t;
  t.mean = base;
  t.q = t.mean + 3 * kThreads;
  t.ls = t.q + 4 * kThreads;
  t.sh = t.ls + 3 * kThreads;
  (void)n_basis;
  return t;
}

__device__ __forceinline__ void copy_rows(float* __restrict__ dst, const float* __restrict__ src, i64 first_word, int words) {
  // first_word is a multiple of 4 (256 rows per block): the run starts 16-byte aligned exactly when the array does.  The
  // caller's arrays need only 4-byte alignment (a view into a larger buffer); the test is the same for the whole block.
  // Unaligned: no 16-byte load is issued, the word loop below copies the whole run.
  const int wide = (reinterpret_cast<uintptr_t>(src + first_word) & 15) == 0 ? (words & ~3) : 0;
  const float4* s4 = reinterpret_cast<const float4*>(src + first_word);
  float4* d4 = reinterpret_cast<float4*>(dst);
  for (int j = threadIdx.x; j < (wide >> 2); j += kThreads) d4[j] = s4[j];
  for (int j = wide + threadIdx.x; j < words; j += kThreads) dst[j] = src[first_word + j];
}

__device__ __forceinline__ void load_param_tile(const ParamTile& t, const float* mean, const float* q, const float* log_scale,
                                                const float* color, i64 base, int cnt, int n_basis) {
  copy_rows(t.mean, mean, 3 * base, 3 * cnt);
  copy_rows(t.q, q, 4 * base, 4 * cnt);
  copy_rows(t.ls, log_scale, 3 * base, 3 * cnt);
  copy_rows(t.sh, color, 3 * (i64)n_basis * base, 3 * n_basis * cnt);
}

// 3 sqrt(V^2 |lambda|) of the symmetric matrix read from the lower triangle (gs_model.py:327-332)
__device__ __forceinline__ void box_halfsize(float a, float b, float c, float& hx, float& hy) {
  const float m = 0.5f * (a + c), d = 0.5f * (a - c);
  const float r = sqrtf(d * d + b * b);
  const float lo = m - r, hi = m + r;
  float ex = a, ey = c;
  if (!(lo >= 0.f)) {
    const float ratio = r > 0.f ? d / r : 0.f;
    const float w_hi = 0.5f * (1.f + ratio), w_lo = 0.5f * (1.f - ratio);
    ex = w_lo * fabsf(lo) + w_hi * fabsf(hi);
    ey = w_hi * fabsf(lo) + w_lo * fabsf(hi);
  }
  hx = 3.f * sqrtf(fabsf(ex));
  hy = 3.f * sqrtf(fabsf(ey));
}

__device__ __forceinline__ int trunc_i32(float v) { return (int)v; }

// Real spherical harmonics (the build's eval_sh; the reference's sh_utility is absent) on the unit direction (x, y, z):
// channel ch of sum_k B_k sh[3 k + ch], the degree-2 chain first.  MAXDEG: the highest degree the instantiation can evaluate.
template <int MAXDEG>
__device__ __forceinline__ float sh_colour(const float* sh, int ch, int sh_degree, const float x, const float y, const float z) {
  float v = kShC0 * sh[ch];
  if (sh_degree > 0) {
    v = ((v - kShC1 * y * sh[3 + ch]) + kShC1 * z * sh[6 + ch]) - kShC1 * x * sh[9 + ch];
    if (sh_degree > 1) {
      const float xx = x * x, yy = y * y, zz = z * z;
      v = ((((v + kShC2[0] * (x * y) * sh[12 + ch]) + kShC2[1] * (y * z) * sh[15 + ch]) +
            kShC2[2] * (2.f * zz - xx - yy) * sh[18 + ch]) + kShC2[3] * (x * z) * sh[21 + ch]) +
          kShC2[4] * (xx - yy) * sh[24 + ch];
    }
  }
  if (MAXDEG > 2 && sh_degree > 2) {  // after the degree-2 chain, which stays as it is: zero rows 9..15 add +-0, exactly
    const float xx = x * x, yy = y * y, zz = z * z;
    v = ((((((v + kShC3[0] * y * (3.f * xx - yy) * sh[27 + ch]) + kShC3[1] * (x * y * z) * sh[30 + ch]) +
            kShC3[2] * y * (4.f * zz - xx - yy) * sh[33 + ch]) + kShC3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy) * sh[36 + ch]) +
          kShC3[4] * x * (4.f * zz - xx - yy) * sh[39 + ch]) + kShC3[5] * z * (xx - yy) * sh[42 + ch]) +
        kShC3[6] * x * (xx - 3.f * yy) * sh[45 + ch];
  }
  return v;
}

// Forward, one thread per Gaussian.  Per Gaussian, one 64-byte record (what the gather reads back in one piece), the sort key
// of its depth and the cull flag.
//   record words: 0-3 box x0 y0 x1 y1 | 4-5 pixel centre (SPLAT: float, else int) | 6-9 Sigma'^-1 | 10 opacity | 11-13 colour |
//                 14 camera depth | 15 unused
// MAXDEG: the highest SH degree the instantiation can evaluate (sh_degree <= MAXDEG is the caller's to ensure).
// SPLAT (gcp_splat.hip; false: cov_eps, mean_offset and clamp_colour are not read): the centre stays a float, stored as
// px + mean_offset, and the box goes around it, ceil(c - h) .. floor(c + h); cov_eps replaces the 1e-6 on the covariance's
// diagonal; clamp_colour: l = max(SH sum, 0) per channel; antialias: the opacity word holds sigmoid(o) rho (`compensation`),
// every other word is what it is without it.
template <int MAXDEG, bool WORLD, bool SPLAT>
__device__ __forceinline__ void project_fwd(
    const float* __restrict__ mean, const float* __restrict__ q, const float* __restrict__ log_scale,
    const float* __restrict__ opacity, const float* __restrict__ color, const float* __restrict__ cam_P,
    const float* __restrict__ cam_K, i64 n, int sh_degree, int n_basis, int width, int height, float box_clamp, float cov_eps,
    float mean_offset, bool clamp_colour, float4* __restrict__ record, int* __restrict__ sort_key, uint8_t* __restrict__ keep,
    int* __restrict__ row_of, bool antialias = false) {
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
    project_one(cam, tile.mean, tile.q, tile.ls, threadIdx.x, p, SPLAT ? cov_eps : 1e-6f);
    float hx, hy;
    box_halfsize(p.a, p.c, p.d, hx, hy);
    const float ilim = 2147483647.f / 1000.f;
    bool k;                  // kept: in front of the camera, a box that is not empty and reaches into the frame
    int x0, y0, x1, y1;      // the box, cut to the frame
    float centre[2];         // words 4-5 of the record
    if constexpr (SPLAT) {
      const float cx = clampf(p.px, -ilim, ilim) + mean_offset, cy = clampf(p.py, -ilim, ilim) + mean_offset;
      const float bw = fminf(hx, box_clamp), bh = fminf(hy, box_clamp);
      // clamped before conversion: every operand of the tests below is a valid int32 (a NaN extent clamps to +-ilim)
      const int bx0 = (int)ceilf(clampf(cx - bw, -ilim, ilim)), bx1 = (int)floorf(clampf(cx + bw, -ilim, ilim));
      const int by0 = (int)ceilf(clampf(cy - bh, -ilim, ilim)), by1 = (int)floorf(clampf(cy + bh, -ilim, ilim));
      k = p.t[2] > 0.f && bx1 >= bx0 && by1 >= by0 && bx0 < width && bx1 > 0 && by0 < height && by1 > 0;
      x0 = min(max(bx0, 0), width), y0 = min(max(by0, 0), height);
      x1 = min(max(bx1, 0), width), y1 = min(max(by1, 0), height);
      centre[0] = cx, centre[1] = cy;  // finite for every Gaussian: clamped before the offset
    } else {
      const int mx = trunc_i32(clampf(p.px, -ilim, ilim)), my = trunc_i32(clampf(p.py, -ilim, ilim));
      const int bw = trunc_i32(fminf(hx, box_clamp)), bh = trunc_i32(fminf(hy, box_clamp));
      k = p.t[2] > 0.f && bw != 0 && mx - bw < width && mx + bw > 0 && my - bh < height && my + bh > 0;
      x0 = min(max(mx - bw, 0), width), y0 = min(max(my - bh, 0), height);
      x1 = min(max(mx + bw, 0), width), y1 = min(max(my + bh, 0), height);
      centre[0] = __int_as_float(mx), centre[1] = __int_as_float(my);
    }
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
      if constexpr (SPLAT)
        if (clamp_colour && l[ch] < 0.f) l[ch] = 0.f;  // the test the backward repeats on the same sum
    }
    float alpha = 1.f / (1.f + expf(-opacity[i]));
    if constexpr (SPLAT)
      if (antialias) alpha *= compensation(p).rho;
    float4* rec = record + 4 * i;
    rec[0] = make_float4(__int_as_float(x0), __int_as_float(y0), __int_as_float(x1), __int_as_float(y1));
    rec[1] = make_float4(centre[0], centre[1], p.d / p.det, -p.b / p.det);
    rec[2] = make_float4(-p.c / p.det, p.a / p.det, alpha, l[0]);
    rec[3] = make_float4(l[1], l[2], p.t[2], 0.f);
  }
}

// Gather: row r of the depth-ordered list is Gaussian perm[r]; unpack its record into the Function's argument arrays, the
// centre as the family's Centre (int2 or float2).  DEPTH: whether its camera depth is written too (0 for a culled one).
enum class GatherDepth { no, yes, if_given };  // if_given: where `depth` is not NULL, tested at run time
template <typename Centre, GatherDepth DEPTH>
__device__ __forceinline__ void project_gather(
    const float4* __restrict__ record, const int* __restrict__ perm, i64 m, int* __restrict__ start_xy,
    int* __restrict__ end_xy, Centre* __restrict__ mean_xy, i64* __restrict__ boxsize, float* __restrict__ vinv,
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
    if constexpr (std::is_same_v<Centre, int2>) mean_xy[r] = make_int2(__float_as_int(b.x), __float_as_int(b.y));
    else mean_xy[r] = make_float2(b.x, b.y);
    boxsize[r] = (i64)(x1 - x0 + 1) * (i64)(y1 - y0 + 1);
    reinterpret_cast<float4*>(vinv)[r] = make_float4(b.z, b.w, c.x, c.y);
    alpha[r] = c.z;
    l_d[3 * r] = c.w, l_d[3 * r + 1] = d.x, l_d[3 * r + 2] = d.y;
    if (DEPTH == GatherDepth::yes || (DEPTH == GatherDepth::if_given && depth != nullptr)) depth[r] = culled ? 0.f : d.z;
    index[r] = i;
    if (!culled) row_of[i] = (int)r;
  }
}

// Backward, one thread per Gaussian, in the Gaussians' own order (coalesced parameter reads and gradient writes); the only
// scattered reads are the 8 upstream gradient words of its row `row_of[i]` in the depth-ordered list.  Culled
// Gaussians (row -1) get zeros: every gradient row is written, nothing needs clearing first.
// SPLAT (gcp_splat.hip; false leaves the chain of gcp_project.hip as it is): cov_eps replaces the 1e-6 on the covariance's
// diagonal; g_depth is tested at run time instead of DEPTH; g_mean_xy (may be NULL) is dL/d(float pixel centre) in list
// order, chained through px = ph0 / pz, py = ph1 / pz, ph = K t, pz = max(ph2, 1e-2) into dL/dt (zero where the centre was
// clamped at +-ilim); clamp_colour: a channel whose SH sum is < 0 was clamped to 0 by the forward and passes no gradient;
// antialias: g_alpha is dL/d(sigmoid(o) rho) — the logit gets g_alpha rho s (1 - s), and dL/drho = g_alpha s reaches the
// covariance through both determinants of rho = sqrt(det0 / det), added to dL/dA before the clamped entries are zeroed.
template <int MAXDEG, bool WORLD, bool DEPTH, bool SPLAT = false>
__device__ __forceinline__ void project_bwd(
    const float* __restrict__ mean, const float* __restrict__ q, const float* __restrict__ log_scale,
    const float* __restrict__ opacity, const float* __restrict__ color, const float* __restrict__ cam_P,
    const float* __restrict__ cam_K, i64 n, int sh_degree, int n_basis, const int* __restrict__ row_of,
    const float* __restrict__ g_vinv, const float* __restrict__ g_alpha, const float* __restrict__ g_ld,
    const float* __restrict__ g_depth, float* __restrict__ grad_mean, float* __restrict__ grad_q, float* __restrict__ grad_log_scale,
    float* __restrict__ grad_opacity, float* __restrict__ grad_color, float cov_eps = 1e-6f, bool clamp_colour = false,
    const float* __restrict__ g_mean_xy = nullptr, bool antialias = false) {
  // parameter rows come in and gradient rows go out through LDS as contiguous runs: straight from / to registers they are
  // 37 + 38 four-byte accesses per thread, 12-108 bytes apart (gradient rows direct: 365 us per 10^6 Gaussians; staged: 140)
  extern __shared__ float s_stage[];
  const ParamTile tile = param_tile(s_stage, n_basis);  // the gradient rows have the layout of the parameter rows: a thread's
                                                         // parameter row is replaced, in place and by that thread alone, with its
                                                         // gradient row
  const int sh_words = 3 * n_basis;
  float* lm = tile.mean + 3 * threadIdx.x;
  float* lq = tile.q + 4 * threadIdx.x;
  float* lls = tile.ls + 3 * threadIdx.x;
  float* gsh = tile.sh + sh_words * threadIdx.x;
  const Camera cam = load_camera(cam_P, cam_K);
  for (i64 base = (i64)blockIdx.x * kThreads; base < n; base += (i64)gridDim.x * kThreads) {
    load_param_tile(tile, mean, q, log_scale, color, base, (int)min((i64)kThreads, n - base), n_basis);
    __syncthreads();
    const i64 i = base + threadIdx.x;
    const i64 r = i < n ? row_of[i] : -1;
    if (r < 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) lm[k] = 0.f, lls[k] = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) lq[k] = 0.f;
      for (int k = 0; k < sh_words; ++k) gsh[k] = 0.f;
      if (i < n) grad_opacity[i] = 0.f;
    } else {
    Projected p;
    project_one(cam, tile.mean, tile.q, tile.ls, threadIdx.x, p, cov_eps);  // reads this thread's row before anything overwrites it

    // opacity = sigmoid(o)
    const float al = 1.f / (1.f + expf(-opacity[i]));
    if (!(SPLAT && antialias)) grad_opacity[i] = g_alpha[r] * al * (1.f - al);  // antialias: below, where rho is formed

    // colour: l_d[ch] = sum_k B_k(dir) sh[k][ch]
    constexpr int NB = (MAXDEG + 1) * (MAXDEG + 1);
    float dir[3];
    sh_direction<WORLD>(cam.P, p.view, dir);
    const float x = dir[0], y = dir[1], z = dir[2];
    float Bk[NB] = {kShC0, -kShC1 * y, kShC1 * z, -kShC1 * x, kShC2[0] * x * y, kShC2[1] * y * z,
                    kShC2[2] * (2.f * z * z - x * x - y * y), kShC2[3] * x * z, kShC2[4] * (x * x - y * y)};
    if (MAXDEG > 2) {
      const float xx = x * x, yy = y * y, zz = z * z;
      const float B3[7] = {kShC3[0] * y * (3.f * xx - yy), kShC3[1] * (x * y * z), kShC3[2] * y * (4.f * zz - xx - yy),
                           kShC3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy), kShC3[4] * x * (4.f * zz - xx - yy),
                           kShC3[5] * z * (xx - yy), kShC3[6] * x * (xx - 3.f * yy)};
#pragma unroll
      for (int k = 9; k < NB; ++k) Bk[k] = B3[k - 9];
    }
    const int nb = (sh_degree + 1) * (sh_degree + 1);
    bool dark[3] = {false, false, false};  // channels the forward clamped to 0
    if (SPLAT && clamp_colour) {  // the forward's own sums, bit for bit, before the coefficients are overwritten
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) dark[ch] = sh_colour<MAXDEG>(gsh, ch, sh_degree, x, y, z) < 0.f;
    }
    float gd[3] = {0.f, 0.f, 0.f};  // dL/ddir
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float g = SPLAT && dark[ch] ? 0.f : g_ld[3 * r + ch];
      // this channel's coefficients first: the gradient row goes into the very words they are read from
      float c[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) c[k] = k < nb ? gsh[3 * k + ch] : 0.f;
#pragma unroll
      for (int k = 0; k < NB; ++k)
        if (k < n_basis) gsh[3 * k + ch] = k < nb ? g * Bk[k] : 0.f;
      for (int k = NB; k < n_basis; ++k) gsh[3 * k + ch] = 0.f;
      if (sh_degree > 0) {
        gd[0] += g * (-kShC1 * c[3]);
        gd[1] += g * (-kShC1 * c[1]);
        gd[2] += g * (kShC1 * c[2]);
        if (sh_degree > 1) {
          gd[0] += g * (kShC2[0] * y * c[4] - 2.f * kShC2[2] * x * c[6] + kShC2[3] * z * c[7] + 2.f * kShC2[4] * x * c[8]);
          gd[1] += g * (kShC2[0] * x * c[4] + kShC2[1] * z * c[5] - 2.f * kShC2[2] * y * c[6] - 2.f * kShC2[4] * y * c[8]);
          gd[2] += g * (kShC2[1] * y * c[5] + 4.f * kShC2[2] * z * c[6] + kShC2[3] * x * c[7]);
        }
      }
      if (MAXDEG > 2 && sh_degree > 2) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z;
        const float* c3 = c + (MAXDEG > 2 ? 9 : 0);  // rows 9..15
        gd[0] += g * (6.f * kShC3[0] * xy * c3[0] + kShC3[1] * yz * c3[1] - 2.f * kShC3[2] * xy * c3[2] - 6.f * kShC3[3] * xz * c3[3] +
                      kShC3[4] * (4.f * zz - 3.f * xx - yy) * c3[4] + 2.f * kShC3[5] * xz * c3[5] + 3.f * kShC3[6] * (xx - yy) * c3[6]);
        gd[1] += g * (3.f * kShC3[0] * (xx - yy) * c3[0] + kShC3[1] * xz * c3[1] + kShC3[2] * (4.f * zz - xx - 3.f * yy) * c3[2] -
                      6.f * kShC3[3] * yz * c3[3] - 2.f * kShC3[4] * xy * c3[4] - 2.f * kShC3[5] * yz * c3[5] - 6.f * kShC3[6] * xy * c3[6]);
        gd[2] += g * (kShC3[1] * xy * c3[1] + 8.f * kShC3[2] * yz * c3[2] + 3.f * kShC3[3] * (2.f * zz - xx - yy) * c3[3] +
                      8.f * kShC3[4] * xz * c3[4] + kShC3[5] * (xx - yy) * c3[5]);
      }
    }
    // world frame: dir = -W^T view  ->  dL/dview = -W dL/ddir
    float gv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
      gv[k] = WORLD ? -((cam.P[4 * k] * gd[0] + cam.P[4 * k + 1] * gd[1]) + cam.P[4 * k + 2] * gd[2]) : gd[k];
    float gt[3];  // dL/dt (camera-space mean)
    {
      const float* vv = p.view;
      const float dot = gv[0] * vv[0] + gv[1] * vv[1] + gv[2] * vv[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) gt[k] = -(gv[k] - vv[k] * dot) / p.tlen;
    }

    // Sigma'^-1 = adj(A) / det  ->  dL/dA
    const float g00 = g_vinv[4 * r], g01 = g_vinv[4 * r + 1], g10 = g_vinv[4 * r + 2], g11 = g_vinv[4 * r + 3];
    const float sdot = ((g00 * p.d - g01 * p.b) - g10 * p.c) + g11 * p.a;
    const float gdet = -(sdot / p.det) / p.det;  // not sdot / det^2: a clamped covariance entry takes det past sqrt(FLT_MAX)
    const float lim = 3.4028234663852886e+38f / 1000.f;
    float D[4] = {g11 / p.det + gdet * p.d, -g01 / p.det - gdet * p.c, -g10 / p.det - gdet * p.b, g00 / p.det + gdet * p.a};
    if constexpr (SPLAT) {
      if (antialias) {  // opacity = sigmoid(o) rho;  d rho / dA = (rho / 2) (adj(A0)^T / det0 - adj(A)^T / det)
        const Compensation comp = compensation(p);  // formed here, not next to `al`: nothing of it lives through the colour chain
        const float s = 1.f / (1.f + expf(-opacity[i])), gs = g_alpha[r] * s;
        grad_opacity[i] = (g_alpha[r] * comp.rho) * (s * (1.f - s));
        const float h = 0.5f * gs, over_det = comp.rho / p.det;
        D[0] += h * (comp.d0 * comp.rho_det0 - p.d * over_det);
        D[1] += h * (p.c * over_det - p.c * comp.rho_det0);
        D[2] += h * (p.b * over_det - p.b * comp.rho_det0);
        D[3] += h * (comp.a0 * comp.rho_det0 - p.a * over_det);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (!(fabsf(p.cov[k]) <= lim)) D[k] = 0.f;  // clamped (or NaN): no gradient

    // A = J Sc J^T:  dL/dSc = J^T D J,  dL/dJ = D J Sc^T + D^T J Sc
    const float* J = p.J;
    float gSc[9], gJ[6];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        gSc[3 * a + b] = (J[a] * D[0] + J[3 + a] * D[2]) * J[b] + (J[a] * D[1] + J[3 + a] * D[3]) * J[3 + b];
    {
      float JS[6], JSt[6];  // J Sc and J Sc^T
#pragma unroll
      for (int r2 = 0; r2 < 2; ++r2)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          JS[3 * r2 + c] = J[3 * r2] * p.Sc[c] + J[3 * r2 + 1] * p.Sc[3 + c] + J[3 * r2 + 2] * p.Sc[6 + c];
          JSt[3 * r2 + c] = J[3 * r2] * p.Sc[3 * c] + J[3 * r2 + 1] * p.Sc[3 * c + 1] + J[3 * r2 + 2] * p.Sc[3 * c + 2];
        }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        gJ[c] = (D[0] * JSt[c] + D[1] * JSt[3 + c]) + (D[0] * JS[c] + D[2] * JS[3 + c]);
        gJ[3 + c] = (D[2] * JSt[c] + D[3] * JSt[3 + c]) + (D[1] * JS[c] + D[3] * JS[3 + c]);
      }
    }
    // J(t): only entries (0,0), (0,2), (1,1), (1,2) depend on t
    {
      const float fx = cam.K[0], fy = cam.K[4];
      const float zc = fmaxf(p.t[2], 1e-2f), iz2 = 1.f / (zc * zc), iz3 = iz2 / zc;
      gt[0] += gJ[2] * (-fx * iz2);
      gt[1] += gJ[5] * (-fy * iz2);
      if (p.t[2] > 1e-2f)
        gt[2] += gJ[0] * (-fx * iz2) + gJ[2] * (2.f * fx * p.t[0] * iz3) + gJ[4] * (-fy * iz2) + gJ[5] * (2.f * fy * p.t[1] * iz3);
    }
    if (SPLAT ? g_depth != nullptr : DEPTH) gt[2] += g_depth[r];  // the depth the blend weighted is t[2]
    if (SPLAT && g_mean_xy != nullptr) {
      const float ilim = 2147483647.f / 1000.f;
      const float gx = fabsf(p.px) <= ilim ? g_mean_xy[2 * r] : 0.f, gy = fabsf(p.py) <= ilim ? g_mean_xy[2 * r + 1] : 0.f;
      const float* K = cam.K;
      float ph[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) ph[j] = (p.t[0] * K[3 * j] + p.t[1] * K[3 * j + 1]) + p.t[2] * K[3 * j + 2];
      const float pz = fmaxf(ph[2], 1e-2f);
      const float d0 = gx / pz, d1 = gy / pz;
      const float d2 = ph[2] > 1e-2f ? -(gx * ph[0] + gy * ph[1]) / (pz * pz) : 0.f;
      // ph = K t  ->  dL/dt += K^T dL/dph
#pragma unroll
      for (int k = 0; k < 3; ++k) gt[k] += (K[k] * d0 + K[3 + k] * d1) + K[6 + k] * d2;
    }
    // t = W m + t0  ->  dL/dm = W^T dL/dt
#pragma unroll
    for (int k = 0; k < 3; ++k) lm[k] = (cam.P[k] * gt[0] + cam.P[4 + k] * gt[1]) + cam.P[8 + k] * gt[2];

    // Sc = W S W^T  ->  E = dL/dS = W^T gSc W
    float E[9];
    {
      float T[9];  // W^T gSc
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) T[3 * a + b] = cam.P[a] * gSc[b] + cam.P[4 + a] * gSc[3 + b] + cam.P[8 + a] * gSc[6 + b];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) E[3 * a + b] = T[3 * a] * cam.P[b] + T[3 * a + 1] * cam.P[4 + b] + T[3 * a + 2] * cam.P[8 + b];
    }
    // S = R diag(s^2) R^T:  dL/dR = (E + E^T) R diag(s^2),  dL/d(log s_k) = 2 s_k^2 (R^T E R)_kk
    const float* R = p.R;
    float gR[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float er = (E[3 * a] + E[a]) * R[k] + (E[3 * a + 1] + E[3 + a]) * R[3 + k] + (E[3 * a + 2] + E[6 + a]) * R[6 + k];
        gR[3 * a + k] = er * (p.s[k] * p.s[k]);
      }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float acc = 0.f;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) acc += R[3 * a + k] * E[3 * a + b] * R[3 * b + k];
      lls[k] = 2.f * (p.s[k] * p.s[k]) * acc;
    }
    // R(qn), qn = q / |q|
    {
      const float qx = p.qn[0], qy = p.qn[1], qz = p.qn[2], qw = p.qn[3];
      float g[4];
      g[0] = 2.f * (qy * gR[1] + qz * gR[2] + qy * gR[3] - 2.f * qx * gR[4] - qw * gR[5] + qz * gR[6] + qw * gR[7] - 2.f * qx * gR[8]);
      g[1] = 2.f * (-2.f * qy * gR[0] + qx * gR[1] + qw * gR[2] + qx * gR[3] + qz * gR[5] - qw * gR[6] + qz * gR[7] - 2.f * qy * gR[8]);
      g[2] = 2.f * (-2.f * qz * gR[0] - qw * gR[1] + qx * gR[2] + qw * gR[3] - 2.f * qz * gR[4] + qy * gR[5] + qx * gR[6] + qy * gR[7]);
      g[3] = 2.f * (-qz * gR[1] + qy * gR[2] + qz * gR[3] - qx * gR[5] - qy * gR[6] + qx * gR[7]);
      const float dot = g[0] * qx + g[1] * qy + g[2] * qz + g[3] * qw;
      const bool clamped = !(p.qlen > 1e-8f);
#pragma unroll
      for (int k = 0; k < 4; ++k) lq[k] = clamped ? g[k] / p.qlen : (g[k] - p.qn[k] * dot) / p.qlen;
    }
    }  // kept Gaussian
    __syncthreads();
    const int cnt = (int)min((i64)kThreads, n - base);
    for (int j = threadIdx.x; j < 3 * cnt; j += kThreads) grad_mean[3 * base + j] = tile.mean[j], grad_log_scale[3 * base + j] = tile.ls[j];
    for (int j = threadIdx.x; j < 4 * cnt; j += kThreads) grad_q[4 * base + j] = tile.q[j];
    float* out_sh = grad_color + base * sh_words;
    for (int j = threadIdx.x; j < sh_words * cnt; j += kThreads) out_sh[j] = tile.sh[j];
    __syncthreads();
  }
}

// host side, shared by the entry points of both files
inline int grid_for(i64 n) { return (int)((n + kThreads - 1) / kThreads < 65536 ? (n + kThreads - 1) / kThreads : 65536); }

inline bool sh_arguments_valid(int32_t sh_degree, int32_t n_basis, int32_t sh_frame) {
  return sh_degree >= 0 && sh_degree <= 3 && n_basis >= (sh_degree + 1) * (sh_degree + 1) && (sh_frame == 0 || sh_frame == 1);
}

// LDS of one block of the forward and backward kernels: the ParamTile.  0: more than the 64 KiB a block can have (n_basis > 18).
inline size_t stage_bytes(int32_t n_basis) {
  const size_t bytes = (size_t)kThreads * (10 + 3 * (size_t)n_basis) * sizeof(float);
  return bytes <= 64 * 1024 ? bytes : 0;
}

// What a forward or backward entry point checks before any HIP call, in the order the results depend on: the scalars
// (`scalars_ok`: those of the entry point's own), nothing to do, the arrays it cannot do without (the seven parameter
// arrays and `outputs`), the LDS.  kLaunch: go on; anything else is the entry point's return value.
constexpr int kLaunch = -1;
inline int check_projection_call(bool scalars_ok, const float* const (&params)[7], int64_t n_gauss, int32_t sh_degree, int32_t n_basis,
                                 int32_t sh_frame, std::initializer_list<const void*> outputs) {
  if (!scalars_ok || n_gauss < 0 || !sh_arguments_valid(sh_degree, n_basis, sh_frame)) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0) return GCP_OK;
  for (const float* p : params)
    if (!p) return GCP_ERR_INVALID_ARGUMENT;
  for (const void* p : outputs)
    if (!p) return GCP_ERR_INVALID_ARGUMENT;
  return stage_bytes(n_basis) ? kLaunch : GCP_ERR_INVALID_ARGUMENT;
}

// The instantiation of a call: degree <= 2 or degree 3, SH basis on camera-frame or world-space directions.
template <typename Kernel>
inline Kernel pick_kernel(int32_t sh_degree, int32_t sh_frame, Kernel deg2_camera, Kernel deg2_world, Kernel deg3_camera, Kernel deg3_world) {
  const bool world = sh_frame == 1;
  return sh_degree > 2 ? (world ? deg3_world : deg3_camera) : (world ? deg2_world : deg2_camera);
}

}  // namespace
