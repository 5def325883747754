// gcp_bin.hip — tile binning and the int32 prefix sum every tile stage uses.
//
//   f2  Bin Gaussians (given in depth order) into 16x16-pixel tiles: count tiles per box, prefix
//       sum, emit (tile, gaussian) entries Gaussian-major, STABLE LSD radix sort on the tile id
//       (8-bit digits; ranks from wave ballots, waves ordered by an LDS prefix => deterministic), so every
//       tile's list is in depth order.  K entries (~3 per Gaussian) instead of M pairs (~166).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gcp_tiles.hpp"

namespace {
using namespace gcp;

constexpr int kScanChunk = 2048;    // ints per prefix-sum block

// ------------------------------------------------------------------------------------------
// Exclusive prefix sum of int32 (out has n+1 entries, out[n] = total).  Two small launches.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int block_excl_scan_256(int v, int* s_w, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int inc = wave_incl_scan_i(v);
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  int woff = 0, tot = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { const int t = s_w[j]; if (j < w) woff += t; tot += t; }
  total = tot;
  __syncthreads();
  return woff + inc - v;
}

__global__ __launch_bounds__(256) void k_scan_reduce(const int* in, int* bsum, i64 n) {
  __shared__ int s_w[4];
  const i64 base = (i64)blockIdx.x * kScanChunk + (i64)threadIdx.x * 8;
  int s = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) if (base + k < n) s += in[base + k];
  int total;
  block_excl_scan_256(s, s_w, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// second (last) launch: every block first reduces the block sums in front of it (<= a few thousand ints,
// L2-resident) to get its own offset — cheaper than a third launch for the block-sum scan
__global__ __launch_bounds__(256) void k_scan_apply(const int* in, const int* bsum, int* out, i64 n, i64 nb) {
  __shared__ int s_w[4];
  int part = 0;
  for (i64 j = threadIdx.x; j < (i64)blockIdx.x; j += 256) part += bsum[j];
  int boff;
  block_excl_scan_256(part, s_w, boff);  // boff = sum of all parts = offset of this block
  const i64 base = (i64)blockIdx.x * kScanChunk + (i64)threadIdx.x * 8;
  int v[8];
  int s = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) { v[k] = (base + k < n) ? in[base + k] : 0; s += v[k]; }
  int total;
  int ex = block_excl_scan_256(s, s_w, total) + boff;
#pragma unroll
  for (int k = 0; k < 8; ++k) { if (base + k < n) out[base + k] = ex; ex += v[k]; }
  if ((i64)blockIdx.x == nb - 1 && threadIdx.x == 0) out[n] = boff + total;
}

}  // namespace

// host: ws needs ceil(n/2048) ints
int gcp::launch_excl_scan(const int* in, int* out, i64 n, int* ws, hipStream_t stream) {
  if (n <= 0) {
    GCP_HIP(hipMemsetAsync(out, 0, sizeof(int), stream));
    return GCP_OK;
  }
  const i64 nb = (n + kScanChunk - 1) / kScanChunk;
  hipLaunchKernelGGL(k_scan_reduce, dim3((unsigned)nb), dim3(256), 0, stream, in, ws, n);
  hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(256), 0, stream, in, (const int*)ws, out, n, nb);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

namespace {

// ------------------------------------------------------------------------------------------
// f2: tile binning
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tile_count(const int* start, const int* end, i64 n, int W, int H, int* cnt,
                                                     unsigned long long* total64) {
  __shared__ unsigned long long s_total;
  if (threadIdx.x == 0) s_total = 0;
  __syncthreads();
  // grid-stride: few blocks, so the 64-bit total (which lets the host refuse a K that does not fit the int32
  // prefix sums) costs a few hundred atomics, not one per 256 Gaussians
  unsigned long long wide = 0;
  for (i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x; g < n; g += (i64)gridDim.x * blockDim.x) {
    Box b;
    int c = 0;
    if (load_box(start, end, g, W, H, b))
      c = ((b.x1 >> kTileLog2) - (b.x0 >> kTileLog2) + 1) * ((b.y1 >> kTileLog2) - (b.y0 >> kTileLog2) + 1);
    cnt[g] = c;
    wide += (unsigned long long)c;
  }
  if (wide) atomicAdd(&s_total, wide);  // integer adds: order-independent, deterministic
  __syncthreads();
  if (threadIdx.x == 0 && s_total) atomicAdd(total64, s_total);
}

// `capacity` / `info` (capture-safe binning, gcp_bin_tiles): a Gaussian whose entries do not fit below `capacity` is
// left out together with everything behind it; info[0] = entries actually listed, info[1] = 1 if anything was left out.
// A box over many tiles (a background splat: 8 100 of them at 1080p) is emitted by its whole wave, lane l taking entries l,
// l + 64, ... — one thread writing them all kept the launch waiting (0.16 -> 0.49 ms for twenty such boxes).
constexpr int kEmitWide = 128;
__global__ __launch_bounds__(256) void k_tile_emit(const int* start, const int* end, i64 n, int W, int H, int tiles_x,
                                                   const int* off, unsigned* key, unsigned* val, i64 capacity, int* info,
                                                   const unsigned long long* total64) {
  const i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool live = g < n;
  if (info) {
    if (*total64 > 0x7fffffffull) {  // the int32 prefix sums have wrapped: nothing can be listed
      if (g == 0) { info[0] = 0; info[1] = 1; }
      return;
    }
    if (live) {
      const i64 lo = off[g], hi = off[g + 1];
      if (g == 0 && (i64)off[n] <= capacity) { info[0] = off[n]; info[1] = 0; }
      if (lo <= capacity && hi > capacity) { info[0] = (int)lo; info[1] = 1; }  // the one Gaussian that straddles the bound
      if (hi > capacity) live = false;
    }
  }
  Box b = {0, 0, -1, -1};
  if (live) live = load_box(start, end, g, W, H, b);
  const int tx0 = b.x0 >> kTileLog2, ty0 = b.y0 >> kTileLog2;
  const int ntx = live ? (b.x1 >> kTileLog2) - tx0 + 1 : 0, nty = live ? (b.y1 >> kTileLog2) - ty0 + 1 : 0;
  const int e0 = live ? off[g] : 0;
  const bool wide = ntx * nty >= kEmitWide;
  if (live && !wide) {
    int e = e0;
    for (int ty = ty0; ty < ty0 + nty; ++ty)
      for (int tx = tx0; tx < tx0 + ntx; ++tx) {
        key[e] = (unsigned)(ty * tiles_x + tx);
        val[e] = (unsigned)g;
        ++e;
      }
  }
  for (unsigned long long todo = __ballot(wide); todo; todo &= todo - 1ull) {  // wave-uniform: one wide box at a time
    const int owner = __builtin_ctzll(todo);
    const int wtx0 = __builtin_amdgcn_readlane(tx0, owner), wty0 = __builtin_amdgcn_readlane(ty0, owner);
    const int wntx = __builtin_amdgcn_readlane(ntx, owner), wcount = wntx * __builtin_amdgcn_readlane(nty, owner);
    const int we0 = __builtin_amdgcn_readlane(e0, owner);
    const unsigned wg = (unsigned)(g - lane + owner);
    for (int i = lane; i < wcount; i += 64) {
      const int ty = i / wntx, tx = i - ty * wntx;
      key[we0 + i] = (unsigned)((wty0 + ty) * tiles_x + wtx0 + tx);
      val[we0 + i] = wg;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Stable LSD radix sort of (key, payload) pairs, 8-bit digits — used for the (tile, Gaussian) entries of the
// binning (M-sized pixel-key arrays have a sort of their own, gcp_sort.hip).  Per pass: per-block digit histogram laid out [digit][block], ONE
// linear exclusive scan of it (= first output slot of every (digit, block)), then a stable scatter of 4096-key
// blocks.  Inside a block wave w owns keys [1024w, 1024w+1024): (A) every wave counts its digits, (B) a prefix
// over digits and waves gives every (wave, digit) its first slot, (C) each wave ranks its keys 64 at a time in
// order — peers with the same digit from 8 ballots, rank = earlier lanes among the peers — and parks them in
// LDS in digit order, (D) the block copies LDS out, so every digit run is one coalesced global write.
// Deterministic: no atomic ever decides a slot.
// ------------------------------------------------------------------------------------------
// n_dev (optional): the number of keys lives on the device (capture-safe binning); n is then only the bound the grid was
// sized for, and blocks past the real count contribute empty histograms / copy nothing
__global__ __launch_bounds__(256) void k_sort_hist(const unsigned* key, i64 n, int shift, int* hist, int nblk, const int* n_dev,
                                                   int xcd_remap) {
  __shared__ int h[256];
  const i64 chunk = sort_chunk(blockIdx.x, nblk, xcd_remap);
  if (chunk < 0) return;
  if (n_dev) n = min(n, (i64)*n_dev);
  h[threadIdx.x] = 0;
  __syncthreads();
  const i64 base = chunk * kSortChunk;
#pragma unroll 4
  for (int i = threadIdx.x; i < kSortChunk; i += 256)
    if (base + i < n) atomicAdd(&h[(key[base + i] >> shift) & 255u], 1);
  __syncthreads();
  hist[(i64)threadIdx.x * nblk + chunk] = h[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_sort_scatter(const unsigned* key, const unsigned* val, unsigned* key_out,
                                                       unsigned* val_out, i64 n, int shift, const int* hist_excl,
                                                       int nblk, const int* n_dev, int xcd_remap) {
  const i64 chunk = sort_chunk(blockIdx.x, nblk, xcd_remap);
  if (chunk < 0) return;
  if (n_dev) n = min(n, (i64)*n_dev);
  __shared__ unsigned s_key[kSortChunk];
  __shared__ unsigned s_val[kSortChunk];
  __shared__ int off[4][256];   // (A) per-wave digit counts -> (B) first LDS slot of (wave, digit)
  __shared__ int gdelta[256];   // global slot = LDS slot + gdelta[digit]
  __shared__ int s_w[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int d = lane; d < 256; d += 64) off[w][d] = 0;
  __syncthreads();
  const i64 bbase = chunk * kSortChunk;
  const i64 wbase = bbase + (i64)w * (kSortChunk / 4);
  constexpr int kSteps = kSortChunk / 4 / 64;  // 16
  unsigned k[kSteps], v[kSteps];
#pragma unroll
  for (int st = 0; st < kSteps; ++st) {  // (A)
    const i64 i = wbase + st * 64 + lane;
    const bool valid = i < n;
    k[st] = valid ? key[i] : 0u;
    v[st] = valid ? val[i] : 0u;
    if (valid) atomicAdd(&off[w][(k[st] >> shift) & 255u], 1);  // counts only: order-independent
  }
  __syncthreads();
  {  // (B) thread d: digit total -> block-wide exclusive prefix over digits -> per-wave LDS bases
    const int c0 = off[0][tid], c1 = off[1][tid], c2 = off[2][tid], c3 = off[3][tid];
    int total;
    const int lstart = block_excl_scan_256(c0 + c1 + c2 + c3, s_w, total);
    off[0][tid] = lstart;
    off[1][tid] = lstart + c0;
    off[2][tid] = lstart + c0 + c1;
    off[3][tid] = lstart + c0 + c1 + c2;
    gdelta[tid] = hist_excl[(i64)tid * nblk + chunk] - lstart;
  }
  __syncthreads();
#pragma unroll
  for (int st = 0; st < kSteps; ++st) {  // (C) stable ranks, staged into LDS in digit order
    const i64 i = wbase + st * 64 + lane;
    const bool valid = i < n;
    const unsigned d = (k[st] >> shift) & 255u;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const int rank = __builtin_popcountll(peers & ((1ull << lane) - 1ull));
    const int pos = off[w][d];
    if (valid && rank == 0) off[w][d] = pos + __builtin_popcountll(peers);
    if (valid) {
      s_key[pos + rank] = k[st];
      s_val[pos + rank] = v[st];
    }
  }
  __syncthreads();
  const int nvalid = (int)((n - bbase < kSortChunk) ? (n - bbase) : kSortChunk);
  for (int i = tid; i < nvalid; i += 256) {  // (D) coalesced copy-out: consecutive lanes, consecutive slots
    const unsigned kk = s_key[i];
    const i64 g = (i64)i + gdelta[(kk >> shift) & 255u];
    key_out[g] = kk;
    val_out[g] = s_val[i];
  }
}

// tile_start[t] = first sorted entry whose tile id is >= t, for t in [0, n_tiles]
__global__ void k_tile_bounds(const unsigned* key, i64 K, int n_tiles, int* tile_start, const int* n_dev) {
  if (n_dev) K = min(K, (i64)*n_dev);
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > K) return;
  const int prev = (i == 0) ? -1 : (int)key[i - 1];
  const int cur = (i == K) ? n_tiles : (int)key[i];
  for (int t = prev + 1; t <= cur; ++t) tile_start[t] = (int)i;
}

}  // namespace

extern "C" {

int gcp_tile_grid(int32_t width, int32_t height, int32_t* tiles_x, int32_t* tiles_y) {
  if (width < 0 || height < 0 || !tiles_x || !tiles_y) return GCP_ERR_INVALID_ARGUMENT;
  const TileGrid t = tile_grid(width, height);
  *tiles_x = t.tx;
  *tiles_y = t.ty;
  return GCP_OK;
}

size_t gcp_scan_i32_workspace_bytes(int64_t n) {
  return align256((size_t)((n + kScanChunk - 1) / kScanChunk + 1) * sizeof(int));
}

int gcp_exclusive_scan_i32(const int32_t* in, int32_t* out, int64_t n, void* ws, size_t ws_bytes, void* stream) {
  if (n < 0 || !out || (n > 0 && (!in || !ws))) return GCP_ERR_INVALID_ARGUMENT;
  if (n > 0 && ws_bytes < gcp_scan_i32_workspace_bytes(n)) return GCP_ERR_WORKSPACE;
  return launch_excl_scan(in, out, n, (int*)ws, (hipStream_t)stream);
}

// The count pass: every Gaussian's tile count, their exclusive prefix sum in tile_off and their 64-bit total in *total64.
// The counts and the prefix sum's own workspace lie behind the first 256 bytes of ws.
static int count_tiles(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width, int32_t height,
                       int32_t* tile_off, unsigned long long* total64, void* ws, hipStream_t stream) {
  char* p = (char*)ws + 256;
  int* cnt = carve<int>(p, (size_t)n_gauss);
  int* sws = (int*)p;
  GCP_HIP(hipMemsetAsync(total64, 0, sizeof(unsigned long long), stream));
  const i64 count_blocks = (n_gauss + 255) / 256 < 512 ? (n_gauss + 255) / 256 : 512;
  hipLaunchKernelGGL(k_tile_count, dim3((unsigned)count_blocks), dim3(256), 0, stream, start_xy, end_xy,
                     (i64)n_gauss, width, height, cnt, total64);
  GCP_HIP(hipGetLastError());
  return launch_excl_scan(cnt, tile_off, n_gauss, sws, stream);
}

int gcp_bin_tiles_count(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width,
                        int32_t height, int32_t* tile_off, int64_t* n_tile_pairs_host, void* ws,
                        size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_gauss < 0 || width < 0 || height < 0 || !tile_off || !n_tile_pairs_host) return GCP_ERR_INVALID_ARGUMENT;
  *n_tile_pairs_host = 0;
  if (n_gauss == 0) {
    GCP_HIP(hipMemsetAsync(tile_off, 0, sizeof(int), stream));
    return GCP_OK;
  }
  if (!start_xy || !end_xy || !ws) return GCP_ERR_INVALID_ARGUMENT;
  const size_t need = 256 + align256((size_t)n_gauss * sizeof(int)) + gcp_scan_i32_workspace_bytes(n_gauss);
  if (ws_bytes < need) return GCP_ERR_WORKSPACE;
  unsigned long long* total64 = (unsigned long long*)ws;
  const int st = count_tiles(start_xy, end_xy, n_gauss, width, height, tile_off, total64, ws, stream);
  if (st != GCP_OK) return st;
  unsigned long long total = 0;
  GCP_HIP(hipMemcpyAsync(&total, total64, sizeof(total), hipMemcpyDeviceToHost, stream));
  GCP_HIP(hipStreamSynchronize(stream));
  if (total > 0x7fffffffull) return GCP_ERR_INVALID_ARGUMENT;  // (tile, Gaussian) entries are indexed with int32
  *n_tile_pairs_host = (int64_t)total;
  return GCP_OK;
}

size_t gcp_bin_workspace_bytes(int64_t n_gauss, int64_t n_tile_pairs) {
  const int64_t k = n_tile_pairs > 0 ? n_tile_pairs : 1;
  const int64_t nblk = (k + kSortChunk - 1) / kSortChunk;
  size_t b = 0;
  b += 3 * align256((size_t)k * sizeof(unsigned));                 // key A, key B, val B
  b += 2 * align256((size_t)(256 * nblk + 1) * sizeof(int));       // hist, hist_excl
  b += gcp_scan_i32_workspace_bytes(256 * nblk);
  const size_t count_need = 256 + align256((size_t)(n_gauss > 0 ? n_gauss : 1) * sizeof(int)) +
                            gcp_scan_i32_workspace_bytes(n_gauss > 0 ? n_gauss : 1);
  return (b > count_need ? b : count_need) + 512;  // + room for gcp_bin_tiles' 64-bit total behind everything else
}

// emit + stable sort by tile + tile bounds; `info` non-null = capture-safe mode (K is the capacity, the real count is info[0])
static int bin_fill(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width, int32_t height,
                    const int32_t* tile_off, int64_t K, int32_t* tile_start, int32_t* tile_list, int* info,
                    const unsigned long long* total64, void* ws, hipStream_t stream) {
  const TileGrid tg = tile_grid(width, height);
  const int n_tiles = tg.tx * tg.ty;
  const i64 nblk = (K + kSortChunk - 1) / kSortChunk;
  char* p = (char*)ws;
  unsigned* keyA = carve<unsigned>(p, (size_t)K);
  unsigned* keyB = carve<unsigned>(p, (size_t)K);
  unsigned* valB = carve<unsigned>(p, (size_t)K);
  int* hist = carve<int>(p, (size_t)(256 * nblk + 1));
  int* hist_ex = carve<int>(p, (size_t)(256 * nblk + 1));
  int* sws = (int*)p;
  unsigned* valA = (unsigned*)tile_list;  // the caller's output buffer doubles as one value buffer
  const int* n_dev = info;                // info[0] = entries listed

  hipLaunchKernelGGL(k_tile_emit, dim3((unsigned)((n_gauss + 255) / 256)), dim3(256), 0, stream, start_xy, end_xy,
                     (i64)n_gauss, width, height, tg.tx, tile_off, keyA, valA, (i64)K, info, total64);
  GCP_HIP(hipGetLastError());
  int bits = 1;
  while ((1 << bits) < n_tiles) ++bits;
  int passes = (bits + 7) / 8;
  if (passes & 1) ++passes;  // even number of passes: the result lands back in (keyA, valA = tile_list)
  unsigned *ks = keyA, *vs = valA, *kd = keyB, *vd = valB;
  for (int pass = 0; pass < passes; ++pass) {
    const int shift = 8 * pass;
    hipLaunchKernelGGL(k_sort_hist, dim3((unsigned)nblk), dim3(256), 0, stream, (const unsigned*)ks, K, shift, hist, (int)nblk, n_dev, 0);
    GCP_HIP(hipGetLastError());
    const int st = launch_excl_scan(hist, hist_ex, 256 * nblk, sws, stream);
    if (st != GCP_OK) return st;
    hipLaunchKernelGGL(k_sort_scatter, dim3((unsigned)nblk), dim3(256), 0, stream, (const unsigned*)ks,
                       (const unsigned*)vs, kd, vd, K, shift, (const int*)hist_ex, (int)nblk, n_dev, 0);
    GCP_HIP(hipGetLastError());
    unsigned* t;
    t = ks; ks = kd; kd = t;
    t = vs; vs = vd; vd = t;
  }
  hipLaunchKernelGGL(k_tile_bounds, dim3((unsigned)((K + 1 + 255) / 256)), dim3(256), 0, stream, ks, K, n_tiles,
                     tile_start, n_dev);
  GCP_HIP(hipGetLastError());
  return GCP_OK;
}

int gcp_bin_tiles_fill(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width,
                       int32_t height, const int32_t* tile_off, int64_t n_tile_pairs, int32_t* tile_start,
                       int32_t* tile_list, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_gauss < 0 || n_tile_pairs < 0 || width < 0 || height < 0 || !tile_start) return GCP_ERR_INVALID_ARGUMENT;
  const TileGrid tg = tile_grid(width, height);
  const int n_tiles = tg.tx * tg.ty;
  const i64 K = n_tile_pairs;
  if (K == 0) {
    GCP_HIP(hipMemsetAsync(tile_start, 0, (size_t)(n_tiles + 1) * sizeof(int), stream));
    return GCP_OK;
  }
  if (!start_xy || !end_xy || !tile_off || !tile_list || !ws) return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < gcp_bin_workspace_bytes(n_gauss, K)) return GCP_ERR_WORKSPACE;
  return bin_fill(start_xy, end_xy, n_gauss, width, height, tile_off, K, tile_start, tile_list, nullptr, nullptr, ws, stream);
}

int gcp_bin_tiles(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width, int32_t height,
                  int64_t capacity, int32_t* tile_off, int32_t* tile_start, int32_t* tile_list, int32_t* info, void* ws,
                  size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_gauss < 0 || width < 0 || height < 0 || capacity < 1 || capacity > 0x7fffffffLL || !tile_off || !tile_start || !tile_list ||
      !info || !ws)
    return GCP_ERR_INVALID_ARGUMENT;
  const TileGrid tg = tile_grid(width, height);
  const int n_tiles = tg.tx * tg.ty;
  if (n_gauss == 0) {
    GCP_HIP(hipMemsetAsync(tile_off, 0, sizeof(int), stream));
    GCP_HIP(hipMemsetAsync(tile_start, 0, (size_t)(n_tiles + 1) * sizeof(int), stream));
    GCP_HIP(hipMemsetAsync(info, 0, 2 * sizeof(int), stream));
    return GCP_OK;
  }
  if (!start_xy || !end_xy) return GCP_ERR_INVALID_ARGUMENT;
  if (ws_bytes < gcp_bin_workspace_bytes(n_gauss, capacity)) return GCP_ERR_WORKSPACE;
  // count + prefix sum (as gcp_bin_tiles_count, without handing the total to the host); the 64-bit total sits in the
  // last 256 bytes of the workspace, which the sort buffers never reach (gcp_bin_workspace_bytes adds them)
  unsigned long long* total64 = (unsigned long long*)((char*)ws + ((ws_bytes - 256) & ~(size_t)255));
  const int st = count_tiles(start_xy, end_xy, n_gauss, width, height, tile_off, total64, ws, stream);
  if (st != GCP_OK) return st;
  // (a total beyond int32 wraps tile_off negative, which the emit kernel reads as "does not fit": flagged as overflow)
  return bin_fill(start_xy, end_xy, n_gauss, width, height, tile_off, capacity, tile_start, tile_list, info, total64, ws, stream);
}

}  // extern "C"
