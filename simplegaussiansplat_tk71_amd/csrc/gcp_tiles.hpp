// gcp_tiles.hpp — what the tile stages share: gcp_bin.hip (binning), gcp_blend.hip (fused
// blend), gcp_sort.hip (M-sized sort), gcp_walk.hip (tile-list walk, pair lists), gcp_compact.hip (compaction).
//
// What the reference does around its scan (reference: gs_model.py:598-663, :666-692, :786-820):
// expand every Gaussian's box into M splat-pixel pairs, compute the Gaussian kernel per pair,
// radix-sort the M pixel keys, scan, un-sort (second radix sort), compact, blend, scatter-add
// into the image with atomics — ~20 passes over M-length arrays — and the same again (recomputed)
// in backward, plus a pair->Gaussian scatter_reduce.
//
// MI355X-first restatement, same results, no M-length array at all: bin the Gaussians into 16x16-pixel tiles (f2,
// gcp_bin.hip) and let one block per tile walk its depth-ordered list (f1, gcp_blend.hip; gcp_walk.hip).
//
// Reference semantics kept: integer inclusive boxes (uitility.py:336-366), depth order = input
// order, pair dropped when its INCLUSIVE product is exactly 0 (gs_model.py:560,:575-578),
// image layout (H+1, W+1, 3) (gs_model.py:505), single chunk.
#pragma once
#include "gcp_device.hpp"
#include "grouped_cumprod_hip.h"

namespace gcp {

constexpr int kTileLog2 = 4;
constexpr int kTile = 1 << kTileLog2;  // tile edge in pixels; 256 pixels = one block, 4 rows per wave
constexpr int kStage = 256;         // list entries staged per LDS round (forward)
constexpr int kSortChunk = 4096;    // keys per radix-sort block
constexpr int kDropTileLog2 = 12;   // the walk counts the zeros it writes per 2^12 consecutive pairs = one compaction tile
constexpr int kCompactTile = 1 << kDropTileLog2;

struct TileGrid { int tx, ty; };
inline TileGrid tile_grid(int W, int H) { return {(W + 1 + kTile - 1) / kTile, (H + 1 + kTile - 1) / kTile}; }

struct Box { int x0, y0, x1, y1; };
__device__ __forceinline__ bool load_box(const int* start, const int* end, i64 g, int W, int H, Box& b) {
  b.x0 = max(start[2 * g], 0);
  b.y0 = max(start[2 * g + 1], 0);
  b.x1 = min(end[2 * g], W);
  b.y1 = min(end[2 * g + 1], H);
  return b.x1 >= b.x0 && b.y1 >= b.y0;
}

// Chunk (4096 keys) of this block.  Blocks are dealt round-robin over the 8 XCDs; with the remap XCD x takes the x-th
// CONTIGUOUS eighth of the chunks, so the blocks that run on one XCD at the same time hold neighbouring chunks: their
// runs inside every digit bucket are adjacent in the destination, and the partial cache lines at the run ends merge in
// that XCD's L2 instead of being written back half-filled from two.  -1: no such chunk (the grid is rounded up to 8).
__device__ __forceinline__ i64 sort_chunk(i64 b, i64 nblk, int xcd_remap) {
  if (!xcd_remap) return b < nblk ? b : -1;
  const i64 per = (nblk + 7) >> 3;
  const i64 c = (b & 7) * per + (b >> 3);
  return ((b >> 3) < per && c < nblk) ? c : -1;
}
inline unsigned sort_grid(i64 nblk, int xcd_remap) { return (unsigned)(xcd_remap ? ((nblk + 7) >> 3) * 8 : nblk); }

// the set bits of a wave-uniform 64-bit word, lowest first, on the scalar unit
__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
  return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
         (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}

// Exclusive prefix sum of int32 (out has n+1 entries, out[n] = total); ws needs gcp_scan_i32_workspace_bytes(n).
// Defined in gcp_bin.hip.
int launch_excl_scan(const int* in, int* out, i64 n, int* ws, hipStream_t stream);

}  // namespace gcp

// The kernels that walk a tile's list take this by value.  It stays local to each translation unit, like the kernels
// themselves: their symbol names spell their parameter types, and profiles and tests are read by those names.
namespace {

struct BlendArgs {
  const int* start;      // [N,2] x,y inclusive
  const int* end;        // [N,2]
  const float* mean;     // [N,2] x,y
  const float* vinv;     // [N,2,2]
  const float* opacity;  // [N]
  const float* l_d;      // [N,3]
  const int* tile_start; // [n_tiles+1]
  const unsigned* tile_list;  // [K] gaussian id, depth order inside each tile
  int W, H, tiles_x;
};

inline int make_args(BlendArgs& a, const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy,
                     const float* vinv, const float* opacity, const float* l_d, int32_t width, int32_t height,
                     const int32_t* tile_start, const int32_t* tile_list) {
  if (width < 0 || height < 0 || !tile_start) return GCP_ERR_INVALID_ARGUMENT;
  a.start = start_xy; a.end = end_xy; a.mean = mean_xy; a.vinv = vinv; a.opacity = opacity; a.l_d = l_d;
  a.tile_start = tile_start; a.tile_list = (const unsigned*)tile_list;
  a.W = width; a.H = height; a.tiles_x = gcp::tile_grid(width, height).tx;
  return GCP_OK;
}

}  // namespace
