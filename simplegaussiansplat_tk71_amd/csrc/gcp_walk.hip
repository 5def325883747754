// gcp_walk.hip — what walks the tile lists pair by pair: the per-pixel CSR export, the tile-list walk of rows a5 / a6, and
// the Gaussian-major pair lists (rect expansion, box sizes).
//
//   The per-pixel CSR (pixel offsets, pair->Gaussian, pair->rect index) that the scan API
//   consumes is exported by the same traversal (k_pixel_count / k_pixel_fill): bit-exact with
//   torch.sort(stable=True) of the reference's pixel keys (gs_model.py:546-547).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "gcp_tiles.hpp"

namespace {
using namespace gcp;

// ------------------------------------------------------------------------------------------
// per-pixel CSR export (what torch.sort(stable) + unique give the reference, gs_model.py:546-548)
// ------------------------------------------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(256) void k_pixel_lists(const BlendArgs a, int* __restrict__ pixel_count,
                                                     const int* __restrict__ pixel_off,
                                                     const int* __restrict__ box_off, int* __restrict__ pair_gauss,
                                                     int* __restrict__ pair_index, int* __restrict__ pair_key) {
  __shared__ int4 s_box[kStage];
  __shared__ int s_g[kStage];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int tile = blockIdx.x;
  const int px = (tile % a.tiles_x) * kTile + (lane & 15);
  const int py = (tile / a.tiles_x) * kTile + w * 4 + (lane >> 4);
  const bool in_img = px <= a.W && py <= a.H;
  const int first = a.tile_start[tile], last = a.tile_start[tile + 1];
  int n = 0;
  i64 o = 0;
  if (FILL && in_img) o = pixel_off[(i64)py * (a.W + 1) + px];
  for (int base = first; base < last; base += kStage) {
    const int cnt = min(kStage, last - base);
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += 256) {
      const i64 g = a.tile_list[base + j];
      Box b;
      load_box(a.start, a.end, g, a.W, a.H, b);
      s_box[j] = make_int4(b.x0, b.y0, b.x1, b.y1);
      s_g[j] = (int)g;
    }
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      const int4 bx = s_box[k];
      const bool in = (px >= bx.x) & (px <= bx.z) & (py >= bx.y) & (py <= bx.w);
      if (in) {
        if (FILL) {
          const int g = s_g[k];
          pair_gauss[o + n] = g;
          // position of this pixel in the Gaussian-major rect list (uitility.py:336-366):
          // row-major inside the box, boxes concatenated in depth order
          pair_index[o + n] = box_off[g] + (py - bx.y) * (bx.z - bx.x + 1) + (px - bx.x);
          if (pair_key) pair_key[o + n] = py * 10000 + px;  // the reference's pixel key (gs_model.py:538-541)
        }
        ++n;
      }
    }
  }
  if (!FILL && in_img) pixel_count[(i64)py * (a.W + 1) + px] = n;
}

// ------------------------------------------------------------------------------------------
// Rows a5 / a6 for a caller that still holds the BOXES its rect list was expanded from (gs_model.py:601 `_create_rects`
// feeds :607): the sort -> gather -> scan -> un-sort of _create_alpha_brend (gs_model.py:546-555) collapses into one walk
// of the depth-ordered tile lists.  One block per 16x16 tile, one pixel per lane; every lane walks the tile's list and,
// for the entries whose box holds its pixel, reads the pair's value at its Gaussian-major position
//   box_off[g] + (py - y0) * width_g + (px - x0)            (uitility.py:336-366)
// folds it into its running product / sum and writes the INCLUSIVE value back to the same position — exactly
// `output[torch.argsort(index)]` of gs_model.py:555, with every pixel scanned strictly front to back (the CPU path's own
// association; MODE 2: back to front = grad_cumsum's flipped scan, gs_model.py:716-722).  No M-sized sort, no M-sized
// index array: 8 B per pair.  Lanes of one pixel row read and write consecutive addresses (64 B per box row and tile).
// ------------------------------------------------------------------------------------------
constexpr int kWalkStage = 64;  // list entries staged per round: one hit word per wave
constexpr int kWalkBatch = 8;   // listed entries whose loads are in flight together

// A batch: kWalkBatch listed entries of one wave's hit word.  The staged records are read together and the values
// loaded together (walk_load); walk_fold then multiplies / adds them in list order and stores the running values.
// Straight-line code — no branch around a load: a lane outside the box, or a slot past the last hit (record -1: no bits
// set), reads pair 0 and discards it.  gfx950 counts loads and stores in ONE in-order counter, and behind a conditional
// load the compiler can only wait for "everything": every store of a batch then waited for the store before it.
// WIDE = false: pair positions are 32-bit byte offsets from the (wave-uniform) array bases — no 64-bit address
// arithmetic per pair.
struct WalkBatch {
  bool in[kWalkBatch];
  unsigned off[kWalkBatch];
  float v[kWalkBatch];
};
template <int MODE, bool WIDE>
__device__ __forceinline__ void walk_load(WalkBatch& b, unsigned long long& hits, const int4* __restrict__ ent,
                                          unsigned lane_bits, int ly, int lxo, const float* __restrict__ x) {
  int k[kWalkBatch];
#pragma unroll
  for (int u = 0; u < kWalkBatch; ++u) {  // scalar: the next set bit, -1 when none is left
    if (MODE == 2) {
      k[u] = hits ? 63 - __builtin_clzll(hits) : -1;
      hits &= ~(1ull << (k[u] & 63));
    } else {
      k[u] = hits ? __builtin_ctzll(hits) : -1;
      hits &= hits - 1ull;
    }
  }
  int4 e[kWalkBatch];
#pragma unroll
  for (int u = 0; u < kWalkBatch; ++u) e[u] = ent[k[u]];
#pragma unroll
  for (int u = 0; u < kWalkBatch; ++u) {
    asm volatile("" :: "v"(e[u].x), "v"(e[u].y));  // the whole record is read ahead of the membership test
    b.in[u] = ((unsigned)e[u].z & lane_bits) == lane_bits;
    const unsigned o = (unsigned)e[u].x + (unsigned)lxo + __umul24((unsigned)ly, (unsigned)e[u].y);
    b.off[u] = b.in[u] ? o : 0u;
    b.v[u] = WIDE ? x[b.off[u]] : *(const float*)((const char*)x + b.off[u]);
  }
}
// COUNT: how many of the values just written are exactly 0 — what the `!= 0` compaction that follows drops
// (gs_model.py:560) — per kCompactTile consecutive pairs.  One integer add per wave, list entry and tile that has any
// (none at all in a scene without opaque or underflowing layers): the sums do not depend on the order.
template <bool WIDE>
__device__ __forceinline__ void walk_count_dropped(bool drop, unsigned off, int* __restrict__ dropped) {
  unsigned long long dm = __ballot(drop);
  if (!dm) return;
  const unsigned blk = off >> (WIDE ? kDropTileLog2 : kDropTileLog2 + 2);
  const int lane = (int)(threadIdx.x & 63);
  while (dm) {
    const int leader = __builtin_ctzll(dm);
    const unsigned b = (unsigned)__builtin_amdgcn_readlane((int)blk, leader);
    const unsigned long long same = __ballot(drop && blk == b);
    if (lane == leader) atomicAdd(dropped + b, __builtin_popcountll(same));
    dm &= ~same;
  }
}
// OUT: what a pair receives.  kWalkInclusive: its inclusive value (gs_model.py:555); kWalkCount: the same, and the zeros
// written are counted per 4096 pairs; kWalkFinal: the FINAL value of _create_alpha_brend — inclusive / self (cumprod,
// gs_model.py:562) or inclusive - self (cumsum, :564): the pair's own value is in a register anyway, and it is the same
// fp32 division / subtraction the compaction pass would do on the stored inclusive value, so the bits are the same — while
// the `!= 0` test of :560 is taken on the inclusive value here: a pair whose inclusive value is exactly 0 clears its byte of
// `keep` (pre-set to 1 by the launcher) and is counted.  A scene that drops nothing is finished after this kernel.
constexpr int kWalkInclusive = 0, kWalkCount = 1, kWalkFinal = 2;
template <int MODE, bool WIDE, int OUT>
__device__ __forceinline__ void walk_fold(const WalkBatch& b, float* __restrict__ out, float& acc, int* __restrict__ dropped,
                                          unsigned char* __restrict__ keep) {
#pragma unroll
  for (int u = 0; u < kWalkBatch; ++u) {
    bool drop = false;
    if (b.in[u]) {
      acc = (MODE == 0) ? acc * b.v[u] : acc + b.v[u];
      drop = acc == 0.0f;  // NaN is kept, as `!= 0` keeps it
      const float res = (OUT != kWalkFinal) ? acc : (MODE == 0 ? acc / b.v[u] : acc - b.v[u]);
      if (WIDE) out[b.off[u]] = res;
      else *(float*)((char*)out + b.off[u]) = res;
    }
    if (OUT != kWalkInclusive) {
      if (OUT == kWalkFinal && __ballot(drop) != 0ull) {  // wave-uniform: no store instruction at all where nothing drops
        if (drop) keep[WIDE ? b.off[u] : (b.off[u] >> 2)] = 0;
      }
      walk_count_dropped<WIDE>(drop, b.off[u], dropped);
    }
  }
}

// Which tile a block of the walk takes.  Blocks are dealt round-robin over the 8 XCDs (block b runs on XCD b % 8), and tiles
// that share cache lines should share an L2 (see the kernel).  xcd_remap 1: XCD x takes the x-th contiguous eighth of the
// tiles — a band of tile rows.  xcd_remap >= 2: STRIPES of 2^(xcd_remap - 2) tile rows dealt round-robin to the XCDs, so that
// every XCD holds stripes from all over the image: a scene whose Gaussians crowd one region (bands: the XCDs of that region
// do most of the work while the others idle) is spread evenly, and all but the lines that straddle a stripe edge still
// share an L2.  0: tile = block.
__device__ __forceinline__ int walk_tile(unsigned b, int n_tiles, int tiles_x, int xcd_remap) {
  if (xcd_remap < 2) return (int)sort_chunk(b, n_tiles, xcd_remap);
  const int sh = xcd_remap - 2;                  // log2 of the tile rows per stripe
  const int x = (int)(b & 7u), j = (int)(b >> 3);  // XCD, and the block's number on it
  const int per_stripe = tiles_x << sh;
  const int stripe = (j / per_stripe) * 8 + x, within = j % per_stripe;
  const int tile = stripe * per_stripe + within;
  return tile < n_tiles ? tile : -1;
}
inline unsigned walk_grid(int n_tiles, int tiles_x, int xcd_remap) {
  if (xcd_remap < 2) return sort_grid(n_tiles, xcd_remap);
  const int per_stripe = tiles_x << (xcd_remap - 2);
  const int stripes = (n_tiles + per_stripe - 1) / per_stripe;
  return (unsigned)(((stripes + 7) / 8) * 8 * per_stripe);
}

// A wave all of whose 64 pixels have reached a product of exactly 0 (cumprod: it stays 0 — behind an opaque pair, or where the
// product has underflowed, hundreds of layers deep) has nothing left to compute: every further pair of its strip is dropped
// whatever its value.  The rest of the tile's list then costs it one byte per pair — the pair's `keep` byte is cleared and the
// drop counted — instead of a 4-byte load, a multiplication and a 4-byte store (whose result nobody reads: the compaction
// that follows moves kept values only).  Scenes that crowd one region drop a large share of their pairs this way.
template <bool WIDE>
__device__ __forceinline__ void walk_dead(unsigned long long hits, const int4* __restrict__ ent, unsigned lane_bits, int ly, int lxo,
                                          int* __restrict__ dropped, unsigned char* __restrict__ keep) {
  while (hits) {
    const int k = __builtin_ctzll(hits);
    hits &= hits - 1ull;
    const int4 e = ent[k];
    const bool in = ((unsigned)e.z & lane_bits) == lane_bits;
    const unsigned o = (unsigned)e.x + (unsigned)lxo + __umul24((unsigned)ly, (unsigned)e.y);
    if (in) keep[WIDE ? o : (o >> 2)] = 0;
    walk_count_dropped<WIDE>(in, in ? o : 0u, dropped);
  }
}

template <int MODE, bool WIDE, int OUT>  // MODE 0 cumprod, 1 cumsum, 2 reverse cumsum; WIDE: more than 2^30 pairs
// (pinned to eight waves per SIMD the byte-offset form fits 63 VGPRs without a spill — and runs no faster: 0.62 ms either way)
__global__ __launch_bounds__(256) void k_pairs_scan_boxes(const BlendArgs a, const int* __restrict__ box_off,
                                                          const float* __restrict__ x, float* __restrict__ out,
                                                          int* __restrict__ dropped, unsigned char* __restrict__ keep,
                                                          int n_tiles, int xcd_remap) {
  // a staged entry: x = position of the tile's first pixel in the entry's box run (box_off + (tile_y0 - y0) * width +
  // (tile_x0 - x0), may lie before the run), y = box width — both in bytes unless WIDE —, z = the box as bits over the
  // tile's columns (0-15) and rows (16-31).  A lane's pair is x + row * y + column, and it is in the box when both of
  // its bits are set: membership is one AND and one compare.
  __shared__ int4 s_ent_[kWalkStage + 1];
  __shared__ unsigned long long s_hits[4];
  int4* const s_ent = s_ent_ + 1;  // record -1: no bits set, what a batch reads for the slots past its last hit
  if (threadIdx.x == 0) s_ent[-1] = make_int4(0, 0, 0, 0);
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // A box is one contiguous run of the pair arrays (row-major, uitility.py:336-366) but lies across up to 2 x 2 tiles: with
  // blocks dealt round-robin over the XCDs its pieces would be written from different L2s and reach memory as partial
  // lines (measured: 2.6x the algorithmic bytes).  An XCD therefore takes whole tile ROWS (walk_tile): the two pieces of a
  // box row, which share cache lines, always meet in one L2; only the line a box's rows 15 | 16 of a tile-row pair straddle
  // is written from two.
  const int tile = walk_tile(blockIdx.x, n_tiles, a.tiles_x, xcd_remap);
  if (tile < 0) return;
  const int tile_x0 = (tile % a.tiles_x) * kTile, tile_y0 = (tile / a.tiles_x) * kTile;
  constexpr int kUnit = WIDE ? 1 : 4;
  // the lane's pixel in the tile: column lane & 15 (lxo: in pair units), row ly — 4 pixel rows per wave
  const int lxo = (lane & 15) * kUnit, ly = w * 4 + (lane >> 4);
  const unsigned lane_bits = (1u << (lane & 15)) | (1u << (16 + ly));
  const int first = a.tile_start[tile], last = a.tile_start[tile + 1];
  const int nrounds = (last - first + kWalkStage - 1) / kWalkStage;
  float acc = (MODE == 0) ? 1.0f : 0.0f;
  for (int q0 = 0; q0 < nrounds; ++q0) {
    const int q = (MODE == 2) ? (nrounds - 1 - q0) : q0;
    const int base = first + q * kWalkStage;
    const int cnt = min(kWalkStage, last - base);
    __syncthreads();
    if (w == 0) {  // wave 0 stages the round (a fifth wave staging one round ahead of the walkers: measured 6 % slower)
      unsigned rm = 0u;
      if (lane < cnt) {
        const i64 g = a.tile_list[base + lane];
        Box b;
        load_box(a.start, a.end, g, a.W, a.H, b);
        const int wd = b.x1 - b.x0 + 1;
        const int c0 = max(b.x0 - tile_x0, 0), c1 = min(b.x1 - tile_x0, kTile - 1);
        const int r0 = max(b.y0 - tile_y0, 0), r1 = min(b.y1 - tile_y0, kTile - 1);
        const unsigned long long cm = (c1 >= c0) ? ((2ull << c1) - (1ull << c0)) : 0ull;
        rm = (r1 >= r0 && cm) ? ((2u << r1) - (1u << r0)) : 0u;
        // modulo 2^32: every pair of the list lies below 2^32 bytes (2^31 pairs when WIDE), whatever the tile's corner does
        const unsigned p0 = (unsigned)box_off[g] + (unsigned)(tile_y0 - b.y0) * (unsigned)wd + (unsigned)(tile_x0 - b.x0);
        s_ent[lane] = make_int4((int)(p0 * (unsigned)kUnit), wd * kUnit, (int)((unsigned)cm | (rm << 16)), 0);
      }
#pragma unroll
      for (int w2 = 0; w2 < 4; ++w2) {  // wave w2 walks pixel rows 4 w2 .. 4 w2 + 3
        const unsigned long long touched = __ballot(((rm >> (4 * w2)) & 0xfu) != 0u);
        if (lane == 0) s_hits[w2] = touched;
      }
    }
    __syncthreads();
    unsigned long long hits = uniform64(s_hits[w]);
    if (MODE == 0 && OUT == kWalkFinal && hits && __ballot(acc != 0.0f) == 0ull) {  // wave-uniform, decided once per round
      walk_dead<WIDE>(hits, s_ent, lane_bits, ly, lxo, dropped, keep);
      continue;
    }
    // two batches in flight: the loads of the next one are issued before the stores of the one in hand, so that waiting
    // for loaded values (in-order counter) never waits for the stores just issued
    if (hits) {
      WalkBatch A, B;
      walk_load<MODE, WIDE>(A, hits, s_ent, lane_bits, ly, lxo, x);
      for (;;) {
        if (!hits) { walk_fold<MODE, WIDE, OUT>(A, out, acc, dropped, keep); break; }
        walk_load<MODE, WIDE>(B, hits, s_ent, lane_bits, ly, lxo, x);
        walk_fold<MODE, WIDE, OUT>(A, out, acc, dropped, keep);
        if (!hits) { walk_fold<MODE, WIDE, OUT>(B, out, acc, dropped, keep); break; }
        walk_load<MODE, WIDE>(A, hits, s_ent, lane_bits, ly, lxo, x);
        walk_fold<MODE, WIDE, OUT>(B, out, acc, dropped, keep);
      }
    }
  }
}

// Gaussian-major rect list (reference: Utilities.make_rect_points_parallel, uitility.py:336-366, called by
// _create_rects, gs_model.py:480-482): pair i of Gaussian g is pixel (x0 + i % w, y0 + i / w) of its box.
// Parallel over the BOXES, not over the pairs: a block takes kExpandBoxes consecutive Gaussians, each wave writes one box
// at a time — its lanes over consecutive pairs, 512 contiguous bytes per store instruction — and a box of more than
// kExpandBig pairs is written by the whole block.  Nothing is searched (one thread per pair had to find its Gaussian by a
// 20-step bisection of dependent loads in the box offsets: 2.2 ms for 1.65e8 pairs, 0.6 TB/s of stores), and the box's
// width is wave-uniform: i / w is one multiplication by its reciprocal and one correction step (exact: i < 2^24).
constexpr int kExpandBoxes = 64;
constexpr int kExpandBig = 8192;

template <bool BIG>
__device__ __forceinline__ void expand_box(const int* __restrict__ start, const int* __restrict__ end, const int* __restrict__ box_off, i64 g,
                                           i64 m, int W, int H, int t, int step, int2* __restrict__ rects, int* __restrict__ pair_gauss) {
  Box b;
  if (!load_box(start, end, g, W, H, b)) return;
  const int bw = b.x1 - b.x0 + 1;
  i64 size = (i64)bw * (b.y1 - b.y0 + 1);
  if ((size > kExpandBig) != BIG) return;
  const i64 off = box_off[g];
  if (off < 0 || off > m) return;  // (offsets that do not belong to these boxes: nothing is written outside the list)
  size = min(size, m - off);
  if (size < (1 << 24)) {
    const float rw = 1.0f / (float)bw;
    for (int l = t; l < (int)size; l += step) {
      int q = (int)((float)l * rw), r = l - q * bw;
      if (r < 0) { --q; r += bw; }
      else if (r >= bw) { ++q; r -= bw; }
      rects[off + l] = make_int2(b.x0 + r, b.y0 + q);
      if (pair_gauss) pair_gauss[off + l] = (int)g;
    }
  } else {
    for (i64 l = t; l < size; l += step) {
      const i64 q = l / bw;
      rects[off + l] = make_int2(b.x0 + (int)(l - q * bw), b.y0 + (int)q);
      if (pair_gauss) pair_gauss[off + l] = (int)g;
    }
  }
}

__global__ __launch_bounds__(256) void k_expand_rects(const int* __restrict__ start, const int* __restrict__ end, const int* __restrict__ box_off,
                                                      i64 n_gauss, i64 m, int W, int H, int2* __restrict__ rects /*[m]*/,
                                                      int* __restrict__ pair_gauss /*[m] or null*/) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const i64 b0 = (i64)blockIdx.x * kExpandBoxes, b1 = min(n_gauss, b0 + kExpandBoxes);
  for (i64 g = b0 + w; g < b1; g += 4) expand_box<false>(start, end, box_off, g, m, W, H, lane, 64, rects, pair_gauss);
  for (i64 g = b0; g < b1; ++g) expand_box<true>(start, end, box_off, g, m, W, H, (int)threadIdx.x, 256, rects, pair_gauss);
}

__global__ void k_box_sizes(const int* start, const int* end, i64 n, int W, int H, int* size) {
  const i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  Box b;
  size[g] = load_box(start, end, g, W, H, b) ? (b.x1 - b.x0 + 1) * (b.y1 - b.y0 + 1) : 0;
}

}  // namespace

extern "C" {

int gcp_pixel_lists_count(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width,
                          int32_t height, const int32_t* tile_start, const int32_t* tile_list,
                          int32_t* pixel_count, int32_t* box_size, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BlendArgs a;
  const int st = make_args(a, start_xy, end_xy, nullptr, nullptr, nullptr, nullptr, width, height, tile_start, tile_list);
  if (st != GCP_OK || !pixel_count || !box_size || n_gauss < 0) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss > 0 && (!start_xy || !end_xy)) return GCP_ERR_INVALID_ARGUMENT;
  const TileGrid tg = tile_grid(width, height);
  hipLaunchKernelGGL((k_pixel_lists<false>), dim3((unsigned)(tg.tx * tg.ty)), dim3(256), 0, stream, a, pixel_count,
                     (const int*)nullptr, (const int*)nullptr, (int*)nullptr, (int*)nullptr, (int*)nullptr);
  GCP_HIP(hipGetLastError());
  return gcp_box_sizes(start_xy, end_xy, n_gauss, width, height, box_size, stream_);
}

// what the walk's FINAL and counting forms start from: every pair kept until the walk finds its inclusive value 0, no zero
// counted yet (either array may be absent)
static int walk_fills(uint8_t* keep, int32_t* dropped_per_tile, int64_t n_pairs, hipStream_t stream) {
  if (keep) GCP_HIP(hipMemsetAsync(keep, 1, (size_t)n_pairs, stream));
  if (dropped_per_tile)
    GCP_HIP(hipMemsetAsync(dropped_per_tile, 0, (size_t)((n_pairs + kCompactTile - 1) / kCompactTile) * sizeof(int), stream));
  return GCP_OK;
}

// keep != NULL: the FINAL form (values + keep mask + zero counts); else the inclusive form, counting when `dropped_per_tile`
static int walk_impl(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width, int32_t height,
                     const int32_t* tile_start, const int32_t* tile_list, const int32_t* box_off, const float* x, float* out,
                     int64_t n_pairs, int32_t mode, int32_t* dropped_per_tile, uint8_t* keep, void* stream_, bool prepared = false) {
  hipStream_t stream = (hipStream_t)stream_;
  BlendArgs a;
  const int st = make_args(a, start_xy, end_xy, nullptr, nullptr, nullptr, nullptr, width, height, tile_start, tile_list);
  if (st != GCP_OK || n_gauss < 0 || mode < 0 || mode > 2 || n_pairs < 0 || n_pairs > 0x7fffffffLL) return GCP_ERR_INVALID_ARGUMENT;
  if (keep && !dropped_per_tile && n_pairs > 0) return GCP_ERR_INVALID_ARGUMENT;
  if (n_pairs == 0) return GCP_OK;
  if (!prepared) {
    const int fs = walk_fills(keep, dropped_per_tile, n_pairs, stream);
    if (fs != GCP_OK) return fs;
  }
  if (n_gauss == 0) return GCP_OK;
  if (!start_xy || !end_xy || !tile_list || !box_off || !x || !out || x == out) return GCP_ERR_INVALID_ARGUMENT;
  const TileGrid tg = tile_grid(width, height);
  // stripes of one tile row dealt round-robin to the XCDs (walk_tile): as fast as contiguous bands on a scene that fills the
  // image evenly (0.65 against 0.64 ms at cfg3), and 18 % / 43 % faster where the Gaussians crowd the middle (sigma = extent / 4,
  // / 8: the bands of the crowded region worked while the others idled) — profiles/r04_walk_experiments.md
  constexpr int xcd_remap = 2;
  // pair positions as 32-bit byte offsets while the list is no longer than 2^30 pairs (GCP_WALK_WIDE=1 forces the other form)
  const char* fw = getenv("GCP_WALK_WIDE");  // read per call: the tests switch it inside one process
  const bool wide = (fw && *fw && atoi(fw) != 0) || n_pairs > (1LL << 30);
  // a pair's position is formed with ONE 24-bit multiply (row in the tile) x (box width, in bytes unless WIDE): a box can be
  // as wide as the image, so the image has to fit — 2^22 columns in the byte-offset form, 2^24 in the element form
  if ((int64_t)width + 1 >= (wide ? (1LL << 24) : (1LL << 22))) return GCP_ERR_INVALID_ARGUMENT;
  const int out_mode = keep ? kWalkFinal : (dropped_per_tile ? kWalkCount : kWalkInclusive);
  const int n_tiles = tg.tx * tg.ty;
  const dim3 grid(walk_grid(n_tiles, tg.tx, xcd_remap)), block(256);
#define GCP_WALK(M, W_, O_) \
  hipLaunchKernelGGL((k_pairs_scan_boxes<M, W_, O_>), grid, block, 0, stream, a, box_off, x, out, dropped_per_tile, keep, n_tiles, xcd_remap)
#define GCP_WALK_OUT(M, W_)                                  \
  do {                                                       \
    if (out_mode == kWalkFinal) GCP_WALK(M, W_, kWalkFinal); \
    else if (out_mode == kWalkCount) GCP_WALK(M, W_, kWalkCount); \
    else GCP_WALK(M, W_, kWalkInclusive);                    \
  } while (0)
#define GCP_WALK_MODE(M) do { if (wide) GCP_WALK_OUT(M, true); else GCP_WALK_OUT(M, false); } while (0)
  if (mode == 0) GCP_WALK_MODE(0);
  else if (mode == 1) GCP_WALK_MODE(1);
  else GCP_WALK_MODE(2);
#undef GCP_WALK_MODE
#undef GCP_WALK_OUT
#undef GCP_WALK
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int gcp_pairs_scan_boxes(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width, int32_t height,
                         const int32_t* tile_start, const int32_t* tile_list, const int32_t* box_off, const float* x,
                         float* inclusive, int64_t n_pairs, int32_t mode, int32_t* dropped_per_tile, void* stream) {
  if (n_gauss == 0) return (n_gauss < 0 || n_pairs < 0 || mode < 0 || mode > 2 || width < 0 || height < 0 || !tile_start) ? GCP_ERR_INVALID_ARGUMENT : GCP_OK;
  return walk_impl(start_xy, end_xy, n_gauss, width, height, tile_start, tile_list, box_off, x, inclusive, n_pairs, mode,
                   dropped_per_tile, nullptr, stream);
}

int gcp_pairs_finish_prepare(uint8_t* keep, int32_t* dropped_per_tile, int64_t n_pairs, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_pairs < 0 || n_pairs > 0x7fffffffLL) return GCP_ERR_INVALID_ARGUMENT;
  if (n_pairs == 0) return GCP_OK;
  if (!keep || !dropped_per_tile) return GCP_ERR_INVALID_ARGUMENT;
  return walk_fills(keep, dropped_per_tile, n_pairs, stream);
}

int gcp_pairs_finish_boxes(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width, int32_t height,
                           const int32_t* tile_start, const int32_t* tile_list, const int32_t* box_off, const float* x,
                           float* values, uint8_t* keep, int64_t n_pairs, int32_t mode, int32_t* dropped_per_tile, int32_t prepared,
                           void* stream) {
  if (n_pairs > 0 && (!keep || !dropped_per_tile)) return GCP_ERR_INVALID_ARGUMENT;
  return walk_impl(start_xy, end_xy, n_gauss, width, height, tile_start, tile_list, box_off, x, values, n_pairs, mode,
                   dropped_per_tile, keep, stream, prepared != 0);
}

int gcp_box_sizes(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width, int32_t height,
                  int32_t* box_size, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_gauss < 0 || width < 0 || height < 0) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0) return GCP_OK;
  if (!start_xy || !end_xy || !box_size) return GCP_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_box_sizes, dim3((unsigned)((n_gauss + 255) / 256)), dim3(256), 0, stream, start_xy, end_xy,
                     (i64)n_gauss, width, height, box_size);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int gcp_expand_rects(const int32_t* start_xy, const int32_t* end_xy, const int32_t* box_off, int64_t n_gauss,
                     int64_t n_pairs, int32_t width, int32_t height, int32_t* rects_xy, int32_t* pair_gauss,
                     void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_gauss < 0 || n_pairs < 0 || width < 0 || height < 0) return GCP_ERR_INVALID_ARGUMENT;
  if (n_pairs == 0) return GCP_OK;
  if (!start_xy || !end_xy || !box_off || !rects_xy || n_gauss == 0) return GCP_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_expand_rects, dim3((unsigned)((n_gauss + kExpandBoxes - 1) / kExpandBoxes)), dim3(256), 0, stream, start_xy, end_xy,
                     box_off, (i64)n_gauss, (i64)n_pairs, width, height, (int2*)rects_xy, pair_gauss);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int gcp_pixel_lists_fill(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width,
                         int32_t height, const int32_t* tile_start, const int32_t* tile_list,
                         const int32_t* pixel_off, const int32_t* box_off, int32_t* pair_gauss,
                         int32_t* pair_index, int32_t* pair_key, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  BlendArgs a;
  const int st = make_args(a, start_xy, end_xy, nullptr, nullptr, nullptr, nullptr, width, height, tile_start, tile_list);
  if (st != GCP_OK || n_gauss < 0) return GCP_ERR_INVALID_ARGUMENT;
  if (n_gauss == 0) return GCP_OK;
  if (!start_xy || !end_xy || !pixel_off || !box_off || !pair_gauss || !pair_index) return GCP_ERR_INVALID_ARGUMENT;
  const TileGrid tg = tile_grid(width, height);
  hipLaunchKernelGGL((k_pixel_lists<true>), dim3((unsigned)(tg.tx * tg.ty)), dim3(256), 0, stream, a, (int*)nullptr,
                     pixel_off, box_off, pair_gauss, pair_index, pair_key);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

}  // extern "C"
