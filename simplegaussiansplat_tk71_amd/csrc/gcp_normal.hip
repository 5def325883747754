// gcp_normal.hip — what 2DGS's normal-consistency regulariser needs besides the blend.
//
// 1. Per-Gaussian normals (k_normals_fwd / k_normals_bwd): the shortest axis of every list entry's Gaussian, rotated into the
//    camera and turned towards it.  One thread per list entry, 256 threads, no grid cap (m <= INT32_MAX entries are at most
//    2^23 blocks); no atomics: `index` has no repeats, so every row of g_q has at most one writer, and the rows absent from
//    the list are cleared by a memset node in front of the kernel.  A thread's arithmetic does not depend on its position:
//    the same bits whatever the launch shape.  Nothing is read back to the host.
//
// 2. Depth -> normal -> loss (k_nc_fwd / k_nc_bwd), the stencil of 2DGS's depth_to_normal fused with the loss
//        e(p) = 1 - a(p) N(p) . n~(p)   where p and its four neighbours are inside the frame and valid, 1 elsewhere,
//        n~ = c / |c|,  c = (pt(x, y+1) - pt(x, y-1)) x (pt(x+1, y) - pt(x-1, y)),  pt = z r,  z = D / A,
//        r = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1),  valid = A >= alpha_min and D > 0.
//    As PyTorch ops that is ~30 element-wise kernels plus slicing over the B x H x W maps.  Here: one kernel per direction.
//    A 256-thread block owns a 32 x 16 pixel tile of one image (the tiling of gcp_loss.hip) and stages z = D / A of the tile
//    plus its halo in LDS, -1 standing for "not valid or outside the frame" (a valid z is > 0); rows are padded to an odd
//    number of words, so the 32 lanes of a row read 32 different banks.
//      forward : 1-pixel halo; two pixels per thread; the block's sum of e, one float per block, no atomics — the caller adds
//                the block sums in float64 in a fixed order.  Reads 8 B (D, A) + 12 B (N) per pixel.
//      backward: a gather.  2-pixel halo; the block first forms, for the 34 x 18 stencil centres around its tile, the
//                gradients of the stencil's two edge vectors u = pt_down - pt_up and v = pt_right - pt_left (six floats per
//                centre, in LDS; zero where the centre is not defined) and writes g_N = -s a n~ for the centres inside the
//                tile; then every tile pixel q adds what the four centres whose stencil contains it hand to pt(q), in a fixed
//                order (up, down, left, right), and takes it through z = D / A.  A 13-pixel footprint, every n~ recomputed,
//                nothing saved by the forward.  Reads 20 B and writes 20 B per pixel.
//    The factor a(p) = A(p) in e is a constant (2DGS's alpha.detach()): g_A has the terms through z only.  The upstream
//    scalar s is read from device memory.  An image's numbers depend on that image's maps and K alone.
//    |c| > 0 wherever the stencil is defined (c . r < 0, header), so the normalisation has no epsilon; depths so large that
//    |c|^2 leaves float32 (z^2 / (fx fy) ~ 1e19) are not guarded.
#include <math.h>

#include "gcp_device.hpp"
#include "grouped_cumprod_hip.h"

namespace {

using gcp::i64;

constexpr int kThreads = 256;

// ---- 1. per-Gaussian normals ------------------------------------------------------------------------------------------------

// Column k of R(q^) for the unit quaternion (x, y, z, w): qvec_to_rotmat_batch, the products of gcp_project.hpp.
__device__ __forceinline__ void rotation_column(int k, float x, float y, float z, float w, float n[3]) {
  if (k == 0) n[0] = 1 - 2 * (y * y + z * z), n[1] = 2 * (x * y + w * z), n[2] = 2 * (x * z - w * y);
  else if (k == 1) n[0] = 2 * (x * y - w * z), n[1] = 1 - 2 * (x * x + z * z), n[2] = 2 * (y * z + w * x);
  else n[0] = 2 * (x * z + w * y), n[1] = 2 * (y * z - w * x), n[2] = 1 - 2 * (x * x + y * y);
}

// aux byte: bits 0-1 the axis k, bit 2 set when the camera-space column was negated.
__global__ __launch_bounds__(kThreads) void k_normals_fwd(const float* __restrict__ q, const float* __restrict__ log_scale,
                                                          const float* __restrict__ mean, const float* __restrict__ P,
                                                          const i64* __restrict__ index, i64 N, i64 m, float* __restrict__ normal,
                                                          unsigned char* __restrict__ aux) {
  const i64 j = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (j >= m) return;
  const i64 i = index[j];
  if (i < 0 || i >= N) {  // not a row: nothing is read through it
    normal[3 * j] = normal[3 * j + 1] = normal[3 * j + 2] = 0.0f;
    aux[j] = 0;
    return;
  }
  const float qx = q[4 * i], qy = q[4 * i + 1], qz = q[4 * i + 2], qw = q[4 * i + 3];
  const float len = fmaxf(sqrtf(((qx * qx + qy * qy) + qz * qz) + qw * qw), 1e-8f);
  const float x = qx / len, y = qy / len, z = qz / len, w = qw / len;
  const float s0 = log_scale[3 * i], s1 = log_scale[3 * i + 1], s2 = log_scale[3 * i + 2];
  int k = 0;
  float best = s0;
  if (s1 < best) k = 1, best = s1;
  if (s2 < best) k = 2;
  float nw[3], nc[3], tc[3];
  rotation_column(k, x, y, z, w, nw);
  const float mx = mean[3 * i], my = mean[3 * i + 1], mz = mean[3 * i + 2];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    nc[r] = (P[4 * r] * nw[0] + P[4 * r + 1] * nw[1]) + P[4 * r + 2] * nw[2];
    tc[r] = ((P[4 * r] * mx + P[4 * r + 1] * my) + P[4 * r + 2] * mz) + P[4 * r + 3];
  }
  const float d = (nc[0] * tc[0] + nc[1] * tc[1]) + nc[2] * tc[2];
  const bool flip = !(d <= 0.0f);
  normal[3 * j] = flip ? -nc[0] : nc[0];
  normal[3 * j + 1] = flip ? -nc[1] : nc[1];
  normal[3 * j + 2] = flip ? -nc[2] : nc[2];
  aux[j] = (unsigned char)(k | (flip ? 4 : 0));
}

// g_nw = +-P[:, :3]^T g_n; the column's gradient w.r.t. the unit quaternion; then through q^ = q / max(|q|, 1e-8) as the
// projection's backward takes it: (g - q^ (g . q^)) / |q|, or g / 1e-8 where the length is clamped.
__global__ __launch_bounds__(kThreads) void k_normals_bwd(const float* __restrict__ q, const float* __restrict__ P,
                                                          const i64* __restrict__ index, const unsigned char* __restrict__ aux,
                                                          const float* __restrict__ g_normal, i64 N, i64 m, float* __restrict__ g_q) {
  const i64 j = (i64)blockIdx.x * kThreads + threadIdx.x;
  if (j >= m) return;
  const i64 i = index[j];
  if (i < 0 || i >= N) return;
  const int k = aux[j] & 3;
  const float sign = (aux[j] & 4) ? -1.0f : 1.0f;
  const float g0 = sign * g_normal[3 * j], g1 = sign * g_normal[3 * j + 1], g2 = sign * g_normal[3 * j + 2];
  const float a = (P[0] * g0 + P[4] * g1) + P[8] * g2;
  const float b = (P[1] * g0 + P[5] * g1) + P[9] * g2;
  const float c = (P[2] * g0 + P[6] * g1) + P[10] * g2;
  const float qx = q[4 * i], qy = q[4 * i + 1], qz = q[4 * i + 2], qw = q[4 * i + 3];
  const float len = fmaxf(sqrtf(((qx * qx + qy * qy) + qz * qz) + qw * qw), 1e-8f);
  const float x = qx / len, y = qy / len, z = qz / len, w = qw / len;
  float g[4];
  if (k == 0) {
    g[0] = 2.f * (b * y + c * z), g[1] = 2.f * ((b * x - c * w) - 2.f * a * y), g[2] = 2.f * ((b * w + c * x) - 2.f * a * z), g[3] = 2.f * (b * z - c * y);
  } else if (k == 1) {
    g[0] = 2.f * ((a * y + c * w) - 2.f * b * x), g[1] = 2.f * (a * x + c * z), g[2] = 2.f * ((c * y - a * w) - 2.f * b * z), g[3] = 2.f * (c * x - a * z);
  } else {
    g[0] = 2.f * ((a * z - b * w) - 2.f * c * x), g[1] = 2.f * ((a * w + b * z) - 2.f * c * y), g[2] = 2.f * (a * x + b * y), g[3] = 2.f * (a * y - b * x);
  }
  const float dot = ((g[0] * x + g[1] * y) + g[2] * z) + g[3] * w;
  const bool clamped = !(len > 1e-8f);
  const float qn[4] = {x, y, z, w};
#pragma unroll
  for (int t = 0; t < 4; ++t) g_q[4 * i + t] = clamped ? g[t] / len : (g[t] - qn[t] * dot) / len;
}

// ---- 2. depth -> normal -> consistency loss ---------------------------------------------------------------------------------

constexpr int kTW = 32, kTH = 16;  // the tile of gcp_loss.hip: a wave's 64 lanes are two full rows, 128 B each

struct Intrinsics {
  float fx, fy, cx, cy;
};

__device__ __forceinline__ Intrinsics intrinsics(const float* __restrict__ K, int image) {
  const float* k = K + 9 * (i64)image;  // wave-uniform: scalar loads
  return Intrinsics{k[0], k[4], k[2], k[5]};
}

__device__ __forceinline__ float ray_x(const Intrinsics& in, int x) { return (((float)x + 0.5f) - in.cx) / in.fx; }
__device__ __forceinline__ float ray_y(const Intrinsics& in, int y) { return (((float)y + 0.5f) - in.cy) / in.fy; }

// z = D / A of the tile at (x0, y0) and HALO pixels around it -> s_z, rows of kTW + 2 HALO + 1 words; -1 where the pixel is
// outside the frame or not valid.
template <int HALO>
__device__ __forceinline__ void stage_z(const float* __restrict__ D, const float* __restrict__ A, i64 base, int height, int width, int x0,
                                        int y0, float alpha_min, float* __restrict__ s_z) {
  constexpr int kHW = kTW + 2 * HALO, kHH = kTH + 2 * HALO;
  for (int i = threadIdx.x; i < kHH * kHW; i += kThreads) {
    const int r = i / kHW, c = i % kHW;
    const int y = y0 + r - HALO, x = x0 + c - HALO;
    float z = -1.0f;
    if (y >= 0 && y < height && x >= 0 && x < width) {
      const i64 o = base + (i64)y * width + x;
      const float d = D[o], a = A[o];
      if (a >= alpha_min && d > 0.0f) z = d / a;
    }
    s_z[r * (kHW + 1) + c] = z;
  }
}

// The stencil at a centre whose four neighbours are valid: u = pt_down - pt_up, v = pt_right - pt_left, c = u x v, n = c / |c|.
struct Stencil {
  float u[3], v[3], n[3], len;
};

__device__ __forceinline__ Stencil stencil(const Intrinsics& in, int x, int y, float zl, float zr, float zu, float zd) {
  Stencil s;
  const float rx = ray_x(in, x), ry = ray_y(in, y);
  const float rxl = ray_x(in, x - 1), rxr = ray_x(in, x + 1), ryu = ray_y(in, y - 1), ryd = ray_y(in, y + 1);
  s.u[0] = zd * rx - zu * rx, s.u[1] = zd * ryd - zu * ryu, s.u[2] = zd - zu;
  s.v[0] = zr * rxr - zl * rxl, s.v[1] = zr * ry - zl * ry, s.v[2] = zr - zl;
  const float c0 = s.u[1] * s.v[2] - s.u[2] * s.v[1];
  const float c1 = s.u[2] * s.v[0] - s.u[0] * s.v[2];
  const float c2 = s.u[0] * s.v[1] - s.u[1] * s.v[0];
  s.len = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
  s.n[0] = c0 / s.len, s.n[1] = c1 / s.len, s.n[2] = c2 / s.len;
  return s;
}

__device__ __forceinline__ float block_sum(float v, float* s_red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__global__ __launch_bounds__(kThreads) void k_nc_fwd(const float* __restrict__ D, const float* __restrict__ A, const float* __restrict__ Nm,
                                                     const float* __restrict__ K, int height, int width, int tiles_x, int tiles_y,
                                                     float alpha_min, float* __restrict__ e_map, float* __restrict__ dn_map,
                                                     float* __restrict__ partial) {
  constexpr int kS = kTW + 2 + 1;
  __shared__ float s_z[(kTH + 2) * kS];
  __shared__ float s_red[4];
  const int tile = blockIdx.x % (tiles_x * tiles_y), image = blockIdx.x / (tiles_x * tiles_y);
  const int x0 = (tile % tiles_x) * kTW, y0 = (tile / tiles_x) * kTH;
  const i64 plane = (i64)height * width, base = (i64)image * plane;
  const Intrinsics in = intrinsics(K, image);
  stage_z<1>(D, A, base, height, width, x0, y0, alpha_min, s_z);
  __syncthreads();
  float sum = 0.f;
  const int c = threadIdx.x % kTW;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int r = threadIdx.x / kTW + half * (kTH / 2);
    const int x = x0 + c, y = y0 + r;
    if (x < width && y < height) {
      const float zc = s_z[(r + 1) * kS + c + 1], zl = s_z[(r + 1) * kS + c], zr = s_z[(r + 1) * kS + c + 2];
      const float zu = s_z[r * kS + c + 1], zd = s_z[(r + 2) * kS + c + 1];
      const i64 o = base + (i64)y * width + x, o3 = 3 * base + (i64)y * width + x;
      float e = 1.0f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
      if (zc >= 0.f && zl >= 0.f && zr >= 0.f && zu >= 0.f && zd >= 0.f) {
        const Stencil s = stencil(in, x, y, zl, zr, zu, zd);
        n0 = s.n[0], n1 = s.n[1], n2 = s.n[2];
        const float dot = (Nm[o3] * n0 + Nm[o3 + plane] * n1) + Nm[o3 + 2 * plane] * n2;
        e = 1.0f - A[o] * dot;
      }
      sum += e;
      if (e_map) e_map[o] = e;
      if (dn_map) dn_map[o3] = n0, dn_map[o3 + plane] = n1, dn_map[o3 + 2 * plane] = n2;
    }
  }
  const float total = block_sum(sum, s_red);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void k_nc_bwd(const float* __restrict__ D, const float* __restrict__ A, const float* __restrict__ Nm,
                                                     const float* __restrict__ K, int height, int width, int tiles_x, int tiles_y,
                                                     float alpha_min, const float* __restrict__ scale, float* __restrict__ g_D,
                                                     float* __restrict__ g_A, float* __restrict__ g_N) {
  constexpr int kS = kTW + 4 + 1;             // staged z: 20 rows of 36 + 1 words
  constexpr int kCW = kTW + 2, kCH = kTH + 2;  // stencil centres: the tile and one pixel around it
  constexpr int kG = kCW + 1;
  __shared__ float s_z[(kTH + 4) * kS];
  __shared__ float s_g[6][kCH * kG];  // g_u (3 words), g_v (3 words) per centre
  const int tile = blockIdx.x % (tiles_x * tiles_y), image = blockIdx.x / (tiles_x * tiles_y);
  const int x0 = (tile % tiles_x) * kTW, y0 = (tile / tiles_x) * kTH;
  const i64 plane = (i64)height * width, base = (i64)image * plane;
  const Intrinsics in = intrinsics(K, image);
  stage_z<2>(D, A, base, height, width, x0, y0, alpha_min, s_z);
  __syncthreads();
  const float s = scale[0];
  for (int i = threadIdx.x; i < kCH * kCW; i += kThreads) {
    const int r = i / kCW, c = i % kCW;  // the centre (x0 + c - 1, y0 + r - 1): staged at row r + 1, column c + 1
    const int x = x0 + c - 1, y = y0 + r - 1;
    const float zc = s_z[(r + 1) * kS + c + 1], zl = s_z[(r + 1) * kS + c], zr = s_z[(r + 1) * kS + c + 2];
    const float zu = s_z[r * kS + c + 1], zd = s_z[(r + 2) * kS + c + 1];
    float gu[3] = {0.f, 0.f, 0.f}, gv[3] = {0.f, 0.f, 0.f}, gn[3] = {0.f, 0.f, 0.f};
    if (zc >= 0.f && zl >= 0.f && zr >= 0.f && zu >= 0.f && zd >= 0.f) {  // defined: the centre is inside the frame
      const Stencil st = stencil(in, x, y, zl, zr, zu, zd);
      const i64 o = base + (i64)y * width + x, o3 = 3 * base + (i64)y * width + x;
      const float sa = -(s * A[o]);  // dL/d(N . n~)
      const float h0 = sa * Nm[o3], h1 = sa * Nm[o3 + plane], h2 = sa * Nm[o3 + 2 * plane];  // dL/dn~
      const float hn = (h0 * st.n[0] + h1 * st.n[1]) + h2 * st.n[2];
      const float gc0 = (h0 - st.n[0] * hn) / st.len, gc1 = (h1 - st.n[1] * hn) / st.len, gc2 = (h2 - st.n[2] * hn) / st.len;  // dL/dc
      gu[0] = st.v[1] * gc2 - st.v[2] * gc1, gu[1] = st.v[2] * gc0 - st.v[0] * gc2, gu[2] = st.v[0] * gc1 - st.v[1] * gc0;  // v x g_c
      gv[0] = gc1 * st.u[2] - gc2 * st.u[1], gv[1] = gc2 * st.u[0] - gc0 * st.u[2], gv[2] = gc0 * st.u[1] - gc1 * st.u[0];  // g_c x u
      gn[0] = sa * st.n[0], gn[1] = sa * st.n[1], gn[2] = sa * st.n[2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) s_g[k][r * kG + c] = gu[k], s_g[3 + k][r * kG + c] = gv[k];
    if (r >= 1 && r <= kTH && c >= 1 && c <= kTW && x < width && y < height) {  // a pixel of the tile: its g_N, once
      const i64 o3 = 3 * base + (i64)y * width + x;
      g_N[o3] = gn[0], g_N[o3 + plane] = gn[1], g_N[o3 + 2 * plane] = gn[2];
    }
  }
  __syncthreads();
  const int c = threadIdx.x % kTW;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int r = threadIdx.x / kTW + half * (kTH / 2);
    const int x = x0 + c, y = y0 + r;
    if (x < width && y < height) {
      const i64 o = base + (i64)y * width + x;
      float gd = 0.f, ga = 0.f;
      if (s_z[(r + 2) * kS + c + 2] >= 0.f) {
        const float rx = ray_x(in, x), ry = ray_y(in, y);
        // the pixel is centre (r + 1, c + 1) of s_g; it is the DOWN neighbour of the centre above it (+g_u), the UP neighbour
        // of the one below (-g_u), the RIGHT neighbour of the one to its left (+g_v), the LEFT neighbour of the one to its right
        const int up = r * kG + c + 1, down = (r + 2) * kG + c + 1, left = (r + 1) * kG + c, right = (r + 1) * kG + c + 2;
        const float t_up = (s_g[0][up] * rx + s_g[1][up] * ry) + s_g[2][up];
        const float t_down = (s_g[0][down] * rx + s_g[1][down] * ry) + s_g[2][down];
        const float t_left = (s_g[3][left] * rx + s_g[4][left] * ry) + s_g[5][left];
        const float t_right = (s_g[3][right] * rx + s_g[4][right] * ry) + s_g[5][right];
        const float gz = (t_up - t_down) + (t_left - t_right);
        const float a = A[o], d = D[o];
        gd = gz / a;
        ga = -(gz * (d / a)) / a;
      }
      g_D[o] = gd;
      g_A[o] = ga;
    }
  }
}

inline bool frame_ok(int64_t images, int32_t height, int32_t width) {
  return images >= 0 && height >= 1 && width >= 1 && (int64_t)height * width <= INT32_MAX;
}

}  // namespace

extern "C" {

int gcp_normals_forward(const float* variance_q, const float* variance_scale, const float* mean, const float* P, const int64_t* index,
                        int64_t n_gauss, int64_t n_list, float* normal, uint8_t* aux, void* stream) {
  if (n_gauss < 0 || n_gauss > INT32_MAX || n_list < 0 || n_list > INT32_MAX) return GCP_ERR_INVALID_ARGUMENT;
  if (n_list == 0) return GCP_OK;
  if (!variance_q || !variance_scale || !mean || !P || !index || !normal || !aux) return GCP_ERR_INVALID_ARGUMENT;
  const unsigned blocks = (unsigned)((n_list + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(k_normals_fwd, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, variance_q, variance_scale, mean, P,
                     (const i64*)index, (i64)n_gauss, (i64)n_list, normal, aux);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int gcp_normals_backward(const float* variance_q, const float* P, const int64_t* index, const uint8_t* aux, const float* g_normal,
                         int64_t n_gauss, int64_t n_list, float* g_q, void* stream) {
  if (n_gauss < 0 || n_gauss > INT32_MAX || n_list < 0 || n_list > INT32_MAX) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0) return GCP_OK;
  if (!g_q) return GCP_ERR_INVALID_ARGUMENT;
  GCP_HIP(hipMemsetAsync(g_q, 0, (size_t)n_gauss * 4 * sizeof(float), (hipStream_t)stream));  // the rows absent from the list
  if (n_list == 0) return GCP_OK;
  if (!variance_q || !P || !index || !aux || !g_normal) return GCP_ERR_INVALID_ARGUMENT;
  const unsigned blocks = (unsigned)((n_list + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(k_normals_bwd, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, variance_q, P, (const i64*)index, aux, g_normal,
                     (i64)n_gauss, (i64)n_list, g_q);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int64_t gcp_normal_consistency_blocks(int64_t images, int32_t height, int32_t width) {
  if (!frame_ok(images, height, width)) return 0;
  return images * (int64_t)((width + kTW - 1) / kTW) * (int64_t)((height + kTH - 1) / kTH);
}

int gcp_normal_consistency_forward(const float* depth, const float* alpha, const float* normal, const float* K, int64_t images,
                                   int32_t height, int32_t width, float alpha_min, float* e_map, float* depth_normal, float* partial,
                                   void* stream) {
  if (!frame_ok(images, height, width) || !(alpha_min > 0.0f)) return GCP_ERR_INVALID_ARGUMENT;
  if (images == 0) return GCP_OK;
  const int64_t blocks = gcp_normal_consistency_blocks(images, height, width);
  if (blocks > 0x7fffffff || !depth || !alpha || !normal || !K || !partial) return GCP_ERR_INVALID_ARGUMENT;
  const int tx = (width + kTW - 1) / kTW, ty = (height + kTH - 1) / kTH;
  hipLaunchKernelGGL(k_nc_fwd, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, depth, alpha, normal, K, (int)height,
                     (int)width, tx, ty, alpha_min, e_map, depth_normal, partial);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int gcp_normal_consistency_backward(const float* depth, const float* alpha, const float* normal, const float* K, int64_t images,
                                    int32_t height, int32_t width, float alpha_min, const float* scale, float* g_depth, float* g_alpha,
                                    float* g_normal, void* stream) {
  if (!frame_ok(images, height, width) || !(alpha_min > 0.0f)) return GCP_ERR_INVALID_ARGUMENT;
  if (images == 0) return GCP_OK;
  const int64_t blocks = gcp_normal_consistency_blocks(images, height, width);
  if (blocks > 0x7fffffff || !depth || !alpha || !normal || !K || !scale || !g_depth || !g_alpha || !g_normal) return GCP_ERR_INVALID_ARGUMENT;
  const int tx = (width + kTW - 1) / kTW, ty = (height + kTH - 1) / kTH;
  hipLaunchKernelGGL(k_nc_bwd, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, depth, alpha, normal, K, (int)height,
                     (int)width, tx, ty, alpha_min, scale, g_depth, g_alpha, g_normal);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

}  // extern "C"
