// gcp_undistort.hip — resample photographs taken through a distorting lens into ideal pinhole cameras, once, before training:
// what `colmap image_undistorter` does on the host, here in one launch for a whole batch of images with a lens each.
//
// One thread per OUTPUT pixel.  It takes the pixel's centre (i + 0.5, j + 0.5), normalises it with the output intrinsics,
// applies the lens's distortion, maps the result to the source with the source intrinsics, clamps it to the pixel centres of
// the source's border (the edge is replicated), reads the four bilinear taps of each channel and writes the three values to
// their float32 planes.
//
// Shape: a block is 64 x 4 pixels, x fastest, so every wave writes one run of 64 consecutive floats to each plane and reads
// its taps from a few neighbouring source rows.  blockIdx.z is the image; a launch has at most 65535 of them in that
// dimension, and a block walks on by gridDim.z until the batch is done, so the batch has no bound of its own.  The image's
// lens record is addressed by the block alone: it is the same in every lane and is read with scalar loads, and the branch on
// the lens's kind is a scalar branch.  The u8 entry point reads the (H, W, 3) bytes a JPEG decodes to and fuses the permute,
// the conversion and the division by 255: 3 B read (plus what the gathered taps share) and 12 B written per pixel.
// No texture objects, no atomics, no LDS; a pixel's arithmetic depends on its own coordinates and its image's record only,
// so the results are the same bits whatever the batch or its order.  atanf, sqrtf and the divisions are the precise ones.
#include <math.h>

#include "gcp_device.hpp"
#include "grouped_cumprod_hip.h"

namespace {

using gcp::i64;

constexpr int kTileX = 64, kTileY = 4;  // pixels per block: 256 threads, one wave per row of the tile
constexpr i64 kMaxGridY = 65535, kMaxGridZ = 65535;

struct Lens {
  float fx, fy, cx, cy;      // source
  float ofx, ofy, ocx, ocy;  // output
  float k[6], p[2];
  float kind;
};
static_assert(sizeof(Lens) <= GCP_LENS_WORDS * sizeof(float), "the record of the header holds the fields read here");

// Normalised ideal (x, y) -> normalised distorted, the formulas of the header, every sum left to right.
__device__ __forceinline__ void distort(const Lens& L, float x, float y, float& xd, float& yd) {
  const float r2 = x * x + y * y;
  if (L.kind == (float)GCP_LENS_POLYNOMIAL) {
    const float num = 1.0f + r2 * (L.k[0] + r2 * (L.k[1] + r2 * L.k[2]));
    const float den = 1.0f + r2 * (L.k[3] + r2 * (L.k[4] + r2 * L.k[5]));
    const float radial = num / den;
    const float xy2 = 2.0f * x * y;
    xd = x * radial + L.p[0] * xy2 + L.p[1] * (r2 + 2.0f * x * x);
    yd = y * radial + L.p[1] * xy2 + L.p[0] * (r2 + 2.0f * y * y);
  } else if (L.kind == (float)GCP_LENS_FISHEYE) {
    const float r = sqrtf(r2);
    const float theta = atanf(r), t2 = theta * theta;
    const float theta_d = theta * (1.0f + t2 * (L.k[0] + t2 * (L.k[1] + t2 * (L.k[2] + t2 * L.k[3]))));
    const float scale = r > 0.0f ? theta_d / r : 1.0f;
    xd = x * scale;
    yd = y * scale;
  } else {
    xd = x;
    yd = y;
  }
}

struct SourceU8 {  // (n, H, W, 3) bytes
  const uint8_t* base;
  __device__ __forceinline__ float at(i64 image, int c, int y, int x, int H, int W) const {
    return (float)base[(image * H * W + (i64)y * W + x) * 3 + c];
  }
  static __device__ __forceinline__ float finish(float v) { return v / 255.0f; }
};

struct SourceF32 {  // (n, 3, H, W) floats
  const float* base;
  __device__ __forceinline__ float at(i64 image, int c, int y, int x, int H, int W) const {
    return base[(image * 3 + c) * H * W + (i64)y * W + x];
  }
  static __device__ __forceinline__ float finish(float v) { return v; }
};

template <typename Source>
__global__ __launch_bounds__(kTileX* kTileY) void k_undistort(Source src, const float* __restrict__ lenses, i64 images, int H, int W,
                                                              float* __restrict__ dst) {
  const int i = blockIdx.x * kTileX + threadIdx.x, j = blockIdx.y * kTileY + threadIdx.y;
  if (i >= W || j >= H) return;
  const i64 plane = (i64)H * W;
  for (i64 image = blockIdx.z; image < images; image += gridDim.z) {
    const Lens& L = *(const Lens*)(lenses + image * GCP_LENS_WORDS);
    const float x = ((float)i + 0.5f - L.ocx) / L.ofx, y = ((float)j + 0.5f - L.ocy) / L.ofy;
    float xd, yd;
    distort(L, x, y, xd, yd);
    // fmaxf / fminf return the other operand for a NaN: whatever the record holds, the taps stay inside the source
    const float u = fminf(fmaxf(L.fx * xd + L.cx, 0.5f), (float)W - 0.5f) - 0.5f;
    const float v = fminf(fmaxf(L.fy * yd + L.cy, 0.5f), (float)H - 0.5f) - 0.5f;
    const int x0 = min(max((int)u, 0), W - 1), y0 = min(max((int)v, 0), H - 1);  // u, v >= 0: truncation is the floor
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float wx = u - (float)x0, wy = v - (float)y0;
    float* out = dst + image * 3 * plane + (i64)j * W + i;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = src.at(image, c, y0, x0, H, W), b = src.at(image, c, y0, x1, H, W);
      const float d = src.at(image, c, y1, x0, H, W), e = src.at(image, c, y1, x1, H, W);
      const float top = a + wx * (b - a), bottom = d + wx * (e - d);
      out[c * plane] = Source::finish(top + wy * (bottom - top));
    }
  }
}

// What both entry points refuse, before any HIP call.  A plane is indexed with 32-bit ints, the rows of the image are the
// grid's y dimension, and the byte offset of the last output word must fit 63 bits.
int refuse(const void* src, const float* lenses, int64_t images, int32_t height, int32_t width, const float* dst) {
  if (images < 0 || height < 1 || width < 1) return GCP_ERR_INVALID_ARGUMENT;
  const i64 plane = (i64)height * width;
  if (plane > INT32_MAX || (height + kTileY - 1) / kTileY > kMaxGridY) return GCP_ERR_INVALID_ARGUMENT;
  if (images > INT64_MAX / (12 * plane)) return GCP_ERR_INVALID_ARGUMENT;
  if (images > 0 && (!src || !lenses || !dst)) return GCP_ERR_INVALID_ARGUMENT;
  return GCP_OK;
}

template <typename Source>
int launch(Source src, const float* lenses, int64_t images, int32_t height, int32_t width, float* dst, void* stream) {
  const dim3 grid((unsigned)((width + kTileX - 1) / kTileX), (unsigned)((height + kTileY - 1) / kTileY),
                  (unsigned)(images < kMaxGridZ ? images : kMaxGridZ));
  hipLaunchKernelGGL(k_undistort<Source>, grid, dim3(kTileX, kTileY), 0, (hipStream_t)stream, src, lenses, (i64)images, (int)height, (int)width, dst);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

}  // namespace

extern "C" int gcp_undistort_u8(const uint8_t* src, const float* lenses, int64_t images, int32_t height, int32_t width, float* dst, void* stream) {
  if (const int status = refuse(src, lenses, images, height, width, dst)) return status;
  if (images == 0) return GCP_OK;
  return launch(SourceU8{src}, lenses, images, height, width, dst, stream);
}

extern "C" int gcp_undistort_f32(const float* src, const float* lenses, int64_t images, int32_t height, int32_t width, float* dst, void* stream) {
  if (const int status = refuse(src, lenses, images, height, width, dst)) return status;
  if (images == 0) return GCP_OK;
  return launch(SourceF32{src}, lenses, images, height, width, dst, stream);
}
