// gcp_blend_shared.hpp — the one copy of what the kernels that walk a tile's list share: gcp_blend.hip (fused blend, forward
// and backward), gcp_absgrad.hip (absolute screen-space gradient) and gcp_contrib.hip (per-Gaussian contribution).
//
//   staging      a chunk of a tile list into LDS: the record (composed, so a kernel pays LDS only for what it reads) and
//                stage_entries.  All four tile kernels use it.
//   walk         the BACK-TO-FRONT walk of the blend backward as a skeleton: walk_pixel sets a lane's pixel up, walk_back runs
//                the chunks and forms T_k, tg, c_k, d = c_k - R_k and the R recurrence for every entry; what is done with them
//                (the backward's transposed row reduction of seven or eight values, the absgrad's two row sums), the zeros of a
//                dead chunk and the fold of a chunk's rows are the caller's.  The absgrad is DEFINED on the backward's pair set
//                and T_k: both are this code.  The forward walks (blend_fwd_tile, k_contrib_tile) are written for other
//                trade-offs and stay in their files.
//   slots        the Gaussian-major slot of a (tile, Gaussian) entry, and the per-Gaussian reduction over a Gaussian's slots
//                with the accumulator as a parameter.
// gcp_distort.hip (depth distortion) runs on all three: its record carries z instead of the colour, and its c_k comes from a
// hook of walk_back that compiles out of the other kernels.
// Everything is in an anonymous namespace, per translation unit, as BlendArgs in gcp_tiles.hpp: the kernels' symbol names spell
// their parameter types, and profiles and tests are read by those names.
#pragma once
#include <type_traits>

#include "gcp_tiles.hpp"

namespace {
using namespace gcp;

constexpr int kStageBwd = 32;       // entries per chunk of the back-to-front walk (its LDS also holds per-pixel-row partial sums)
constexpr int kCkpt = kStageBwd;    // the forward saves every pixel's transmittance every kCkpt list entries
static_assert(kStage % kCkpt == 0 && 64 % kCkpt == 0 && kCkpt <= 32, "checkpoints fall on hit-word boundaries");
static_assert(kStageBwd <= 32, "one 32-bit word of hits per wave");
constexpr int kReduceWide = 128;    // tile slots from which a Gaussian is summed by its wave (reduce_slots)

// sum over each 16-lane DPP row (= one pixel row of the tile); valid in lanes 15, 31, 47, 63
__device__ __forceinline__ float row_sum16(float v) {
  v += dpp_f<0x111, 0xf>(0.0f, v);
  v += dpp_f<0x112, 0xf>(0.0f, v);
  v += dpp_f<0x114, 0xf>(0.0f, v);
  v += dpp_f<0x118, 0xf>(0.0f, v);
  return v;
}

// The depth / alpha / background variant of the blend (gcp_blend_forward_depth / gcp_blend_backward_depth /
// gcp_blend_absgrad_depth).  Per pixel, with w_k = T_k o_k g_k as for the colour and T_N the transmittance behind the list:
//   depth = sum_k w_k z_k (not divided by alpha),   alpha = 1 - T_N,   image += T_N bg.
// In the backward the background and the alpha map are one more, fully absorbing layer behind the list: the recursion
// starts at R_N = dL/dI . bg - dL/dA (0 where T_N == 0: an exact zero, or an underflow whose true derivative is
// negligible) and c_k gains dL/dD z_k.
struct DepthArgs {
  const float* z;           // [N] camera-space depth of every Gaussian
  const float* bg;          // float[3] background colour, or nullptr (black)
  float* depth;             // forward: [(H+1)(W+1)] expected depth
  float* alpha;             // forward: [(H+1)(W+1)] 1 - T_N
  const float* grad_depth;  // backward: dL/d(depth map), or nullptr (zero)
  const float* grad_alpha;  // backward: dL/d(alpha map), or nullptr (zero)
  float* tile_bg;           // blend backward: [n_tiles][3] per-tile sums of dL/dI T_N, or nullptr (no background gradient)
};

// ---- staging ----------------------------------------------------------------------------------------------------------------

// What every tile kernel stages per list entry; the records below add what only some of them read.
template <int STAGE>
struct Staged {
  static constexpr bool kHasCol = false, kHasRaw = false, kHasZ = false;
  int4 box[STAGE];     // x0, y0, x1-x0, y1-y0 (clamped to the image)
  float4 geo[STAGE];   // mx, my, opacity, box mask as bits (0-15: tile columns inside the box, 16-31: tile rows)
  float4 vin[STAGE];   // Λ' = -0.5*log2(e) * Λ, Λ = [[a,b],[c,d]]: a b c d (forward walks) or a, b + c, d, - (back-to-front walk)
  // hits[w][c]: bit j set = staged entry 64*c + j reaches into the four pixel rows of wave w.  A wave walks the set
  // bits of its own words (scalar s_ff1 / s_andn2) and never sees the entries that miss it.
  unsigned long long hits[4][(STAGE + 63) / 64];
};
template <int STAGE>
struct StagedCol : Staged<STAGE> {  // + colour: the blend and the absgrad
  static constexpr bool kHasCol = true;
  float4 col[STAGE];   // l0 l1 l2, z (depth variants; 0 otherwise)
};
template <int STAGE>
struct StagedColRaw : StagedCol<STAGE> {  // + Λ itself: the absgrad
  static constexpr bool kHasRaw = true;
  float4 raw[STAGE];   // A B C D
};

template <int STAGE>
struct StagedZ : Staged<STAGE> {  // + the depth alone: the distortion
  static constexpr bool kHasZ = true;
  float z[STAGE];
};

template <bool QUAD3, bool DEPTH, class S>
__device__ __forceinline__ void stage_entries(const BlendArgs& a, S& s, int first, int cnt, int tile_x0, int tile_y0,
                                              const float* z = nullptr) {
  for (int j = threadIdx.x; j < cnt; j += blockDim.x) {
    const i64 g = a.tile_list[first + j];
    Box b;
    load_box(a.start, a.end, g, a.W, a.H, b);
    s.box[j] = make_int4(b.x0, b.y0, b.x1 - b.x0, b.y1 - b.y0);
    // the box as two 16-bit masks over the tile's columns and rows: membership of a pixel is ONE and + ONE compare
    // against the lane's own two bits
    const int c0 = max(b.x0 - tile_x0, 0), c1 = min(b.x1 - tile_x0, kTile - 1);
    const int r0 = max(b.y0 - tile_y0, 0), r1 = min(b.y1 - tile_y0, kTile - 1);
    const unsigned cm = (c1 >= c0) ? ((2u << c1) - (1u << c0)) : 0u;
    const unsigned rm = (r1 >= r0) ? ((2u << r1) - (1u << r0)) : 0u;
#pragma unroll
    for (int w2 = 0; w2 < 4; ++w2) {  // entries j of one 64-lane staging wave form one word per target wave
      const unsigned long long touched = __ballot(((rm >> (4 * w2)) & 0xfu) != 0u);
      if ((threadIdx.x & 63) == 0) s.hits[w2][j >> 6] = touched;
    }
    s.geo[j] = make_float4(a.mean[2 * g], a.mean[2 * g + 1], a.opacity[g], __uint_as_float(cm | (rm << 16)));
    // Λ pre-scaled by -0.5*log2(e): g = exp(-0.5 d Λ d^T) becomes ONE v_exp_f32 of d Λ' d^T.  The extra rounding of
    // Λ' moves g by < 1e-7 absolute (relative 6e-8*|log2 g|, and g decays as fast as that factor grows).
    constexpr float kS = -0.5f * 1.44269504088896341f;
    const float A = a.vinv[4 * g], B = a.vinv[4 * g + 1], C = a.vinv[4 * g + 2], D = a.vinv[4 * g + 3];
    // QUAD3 (back-to-front walk): a, b + c, d — the quadratic form in five VALU instead of six; the forward walks keep a, b, c, d
    // and the association of the reference's two matmuls: their per-entry chain is latency-bound and the shorter form is 6 %
    // slower there
    s.vin[j] = QUAD3 ? make_float4(kS * A, kS * B + kS * C, kS * D, 0.0f) : make_float4(kS * A, kS * B, kS * C, kS * D);
    if constexpr (S::kHasRaw) s.raw[j] = make_float4(A, B, C, D);
    if constexpr (S::kHasCol) s.col[j] = make_float4(a.l_d[3 * g], a.l_d[3 * g + 1], a.l_d[3 * g + 2], DEPTH ? z[g] : 0.0f);
    if constexpr (S::kHasZ) s.z[j] = z[g];
  }
}

// ---- Gaussian-major slots ---------------------------------------------------------------------------------------------------

// The slot of list entry `entry` (Gaussian g in tile (ttx, tty)): g's slots start at tile_off[g] and run over the tiles of its
// box, row by row.  bx is the entry's staged box.
__device__ __forceinline__ i64 entry_slot(const BlendArgs& a, const int* __restrict__ tile_off, int entry, const int4& bx, int ttx,
                                          int tty) {
  const i64 g = a.tile_list[entry];
  const int ntx = ((bx.x + bx.z) >> 4) - (bx.x >> 4) + 1;
  return (i64)tile_off[g] + (i64)(tty - (bx.y >> 4)) * ntx + (ttx - (bx.x >> 4));
}

// Per Gaussian (one thread each, g = its index): its tile slots folded in order into an accumulator.  Acc starts as the empty
// fold and has add(slot, e) — take slot e in — and wave_all() — fold the 64 lanes' accumulators in a fixed butterfly, every lane
// ending with the same result.  Only slots a tile kernel wrote are read: a Gaussian's entries [tile_off[g], tile_off[g+1]) count
// iff they lie inside what the binning LISTED (tile_start[n_tiles] entries: everything with exact binning; with a capture-safe
// capacity the Gaussians that fit; nothing at all when the int32 prefix sums wrapped at > 2^31 entries — the offsets behind the
// wrap are negative or decreasing, and even the ones before it point at slots nobody wrote).  The empty fold otherwise.
// A Gaussian whose box covers many tiles (a background splat over the whole frame: 8 100 slots of 9 values) is not left to one
// thread — 73 000 dependent loads, 1.1 ms for twenty of them while the rest of the launch takes 0.04 — but folded by its whole
// wave: lane l takes slots e0 + l, e0 + l + 64, ... in order, and the 64 partial results meet in the butterfly.  Which
// Gaussians go that way depends on their slot count alone, so the result is the same from run to run.
// Every thread of the wave must call this (also g >= n).
template <class Acc, class Slot>
__device__ __forceinline__ Acc reduce_slots(const Slot* __restrict__ slot, const int* __restrict__ tile_off,
                                            const int* __restrict__ tile_start, int n_tiles, i64 g, i64 n, i64 capacity) {
  const int lane = threadIdx.x & 63;
  Acc r;
  const i64 listed = min((i64)tile_start[n_tiles], capacity);
  i64 e0 = 0, e1 = 0;
  if (g < n) {
    e0 = tile_off[g];
    e1 = tile_off[g + 1];
    if (e0 < 0 || e1 < e0 || e1 > listed) e1 = e0 < 0 ? 0 : e0;
    if (e0 < 0) e0 = 0;
  }
  const bool wide = e1 - e0 >= kReduceWide;
  if (!wide) {
    for (i64 e = e0; e < e1; ++e) r.add(slot, e);
  }
  for (unsigned long long todo = __ballot(wide); todo; todo &= todo - 1ull) {  // wave-uniform: one wide Gaussian at a time
    const int owner = __builtin_ctzll(todo);
    const i64 f0 = (i64)__builtin_amdgcn_readlane((int)e0, owner), f1 = (i64)__builtin_amdgcn_readlane((int)e1, owner);  // (entries < 2^31)
    Acc p;
    for (i64 e = f0 + lane; e < f1; e += 64) p.add(slot, e);
    p.wave_all();
    if (lane == owner) r = p;
  }
  return r;
}

// NV sums per slot of NV floats
template <int NV>
struct SlotSums {
  float v[NV];
  __device__ __forceinline__ SlotSums() {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = 0.0f;
  }
  __device__ __forceinline__ void add(const float* __restrict__ slot, i64 e) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] += slot[e * NV + i];
  }
  __device__ __forceinline__ void wave_all() {
#pragma unroll
    for (int i = 0; i < NV; ++i)
      for (int o = 32; o > 0; o >>= 1) v[i] += __shfl_xor(v[i], o);
  }
};

// ---- transmittance checkpoints ----------------------------------------------------------------------------------------------

// Slot q of tile t holds every pixel's transmittance in front of list entry first + q kCkpt, for q = 0 .. ceil(n / kCkpt)
// — the last one is the transmittance behind the whole list — 256 floats each (one per pixel of the tile, thread order).
// Tile t's slots start at first / kCkpt + 2 t: consecutive tiles never overlap
// (floor(first/c) + ceil(n/c) + 1 <= floor((first+n)/c) + 2), so K / kCkpt + 2 n_tiles + 2 slots hold them all without a
// separate prefix sum.
__device__ __forceinline__ i64 ckpt_slot0(int first, int tile) { return (i64)(first / kCkpt) + 2 * (i64)tile; }

// ---- the back-to-front walk -------------------------------------------------------------------------------------------------
//
// Per pixel, with k running over the list entries whose box holds the pixel, T_k the exclusive transmittance,
// a_k = o_k g_k, c_k = (dL/dI . l_k) (+ dL/dD z_k), p_k = T_k a_k l_k (gs_model.py:500):
//   S_k = sum_{j>k} (dL/dI . p_j)                    exclusive suffix sum, gs_model.py:716-722
//   S_k / (1 - a_k) = T_k R_k,   R_{k-1} = a_k c_k + (1 - a_k) R_k = R_k + a_k (c_k - R_k),   R_last = 0
//   dL/do_k    = T_k g_k (c_k - R_k)                 gs_model.py:733-740   (= gp/o - (g/anti) S)
//   "common"_k = T_k a_k (c_k - R_k)                 gs_model.py:747-748, :757-758   (= gp - (a/anti) S)
//   dL/dl_k    = dL/dI T_k a_k                       (true gradient; the reference's is channel-collapsed, Q2)
// The list is walked back to front, one staged chunk of kStageBwd entries at a time, in ONE pass: the transmittance in
// front of an entry comes from the one behind it, T_k = T_{k+1} / (1 - a_k) (v_rcp_f32, 1 ulp), restarted at every chunk
// from the checkpoint the forward kernel saved for the chunk's END — so the quotients never chain further than one chunk
// (<= 32 roundings, ~2e-6 relative) and nothing is subtracted or accumulated in T.  A quotient cannot undo an
// underflow: a chunk in which some pixel's transmittance falls below FLT_MIN (at most one chunk per pixel) is handled by
// its wave with T_k recomputed front to back from the chunk's START checkpoint for every entry instead (exact; the product
// up to an entry's group of eight is formed once per group: ~160 entry evaluations per chunk, two more registers).
// g_k = 0 where the pixel is outside the box or the pair was dropped (gs_model.py:560) — such an entry then contributes
// exactly nothing.  Every gradient term is T_k times a convex combination of the c_j: its round-off is relative to the
// layer's own transmittance at any depth.

// T behind staged entry j for this lane's pixel, given T in front of it: T * (1 - o_j g_j) inside the entry's box, T outside
template <class S>
__device__ __forceinline__ float slow_factor(const S& s, int j, float fx, float fy, unsigned lane_bits, float T) {
  const float4 gj = s.geo[j];
  const float4 vj = s.vin[j];
  const float dxj = fx - gj.x, dyj = fy - gj.y;
  const float g_j = __builtin_amdgcn_exp2f(dxj * (vj.x * dxj + vj.y * dyj) + (vj.z * dyj) * dyj);
  return ((__float_as_uint(gj.w) & lane_bits) == lane_bits) ? T * (1.0f - gj.z * g_j) : T;
}

// One lane's pixel of a 256-thread block on tile blockIdx.x, one pixel per lane, four pixel rows per wave
struct WalkPixel {
  int lane, w;              // lane of the wave; wave id in an SGPR: the row tests are scalar
  int tile, ttx, tty, px, py;
  float fx, fy;
  unsigned lane_bits;       // the pixel's column bit and row bit, against geo.w
  int first, last, nchunks; // the tile's list [first, last) and its chunks of kStageBwd
  const float* ck;          // this thread's word of the tile's first checkpoint slot
  float g0, g1, g2, gz;     // dL/dI and dL/dD (depth variant) of the pixel; 0 outside the frame
  float T_N;                // depth variant: the transmittance behind the whole list
  float R;                  // R behind the list: 0, or the absorbing layer's (DepthArgs)
};

// IMAGE false: no dL/dI is read (g0 = g1 = g2 = 0; grad_image may be null) — the distortion's walk
template <bool DEPTH, bool IMAGE = true>
__device__ __forceinline__ WalkPixel walk_pixel(const BlendArgs& a, const float* __restrict__ t_ckpt,
                                                const float* __restrict__ grad_image, const DepthArgs& da) {
#pragma clang fp contract(fast)  // as in walk_back
  WalkPixel p;
  p.lane = threadIdx.x & 63;
  p.w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  p.tile = blockIdx.x;
  p.ttx = p.tile % a.tiles_x; p.tty = p.tile / a.tiles_x;
  p.px = p.ttx * kTile + (p.lane & 15);
  p.py = p.tty * kTile + p.w * 4 + (p.lane >> 4);
  p.fx = (float)p.px; p.fy = (float)p.py;
  p.first = a.tile_start[p.tile];
  p.last = a.tile_start[p.tile + 1];
  p.g0 = p.g1 = p.g2 = 0.0f;
  if (IMAGE && p.px <= a.W && p.py <= a.H) {
    const i64 o = ((i64)p.py * (a.W + 1) + p.px) * 3;
    p.g0 = grad_image[o]; p.g1 = grad_image[o + 1]; p.g2 = grad_image[o + 2];
  }
  p.lane_bits = (1u << (p.lane & 15)) | (1u << (16 + p.w * 4 + (p.lane >> 4)));
  p.ck = t_ckpt + ckpt_slot0(p.first, p.tile) * 256 + threadIdx.x;
  p.nchunks = (p.last - p.first + kStageBwd - 1) / kStageBwd;
  p.R = 0.0f;  // the suffix behind the end of the list is empty
  p.gz = 0.0f;
  p.T_N = 0.0f;
  if (DEPTH) {
    p.T_N = p.ck[(i64)p.nchunks * 256];
    float ga = 0.0f;
    if (p.px <= a.W && p.py <= a.H) {
      const i64 o = (i64)p.py * (a.W + 1) + p.px;
      if (da.grad_depth) p.gz = da.grad_depth[o];
      if (da.grad_alpha) ga = da.grad_alpha[o];
    }
    const float cb = da.bg ? p.g0 * da.bg[0] + p.g1 * da.bg[1] + p.g2 * da.bg[2] : 0.0f;
    p.R = (p.T_N != 0.0f) ? cb - ga : 0.0f;  // the absorbing layer behind the list (DepthArgs)
  }
  return p;
}

// The walk itself.  `s` is the caller's staging record in LDS (with colour).  Per entry that reaches the wave, deepest first:
//   body(k, opacity, dx, dy, tg, d)   staged entry k; tg = T_k g_k (0 outside the box and for a dropped pair), d = c_k - R_k
// per chunk that every pixel of the wave enters behind an exact zero, instead:
//   zero(hits)                        hand the fold zeros for the wave's entries (the set bits)
// and per chunk, after a barrier, one thread per entry:
//   fold(j, entry)                    staged entry j = list entry `entry`, into its Gaussian-major slot (entry_slot)
// `hook` replaces c_k = dL/dI . l_k (+ dL/dD z_k) where the caller's c_k is not a fixed per-entry number but depends on the lane's
// own state: with Hook::kOn the record needs no colour, and per entry, before the body,
//   c_k = hook.c(s, k, w_k)           w_k = T_k o_k g_k (0 outside the box and for a dropped pair)
// The default compiles out.
struct NoHook {
  static constexpr bool kOn = false;
};
template <bool DEPTH, class S, class Body, class Zero, class Fold, class Hook = NoHook>
__device__ __forceinline__ void walk_back(const BlendArgs& a, const DepthArgs& da, S& s, const WalkPixel& p, Body body, Zero zero, Fold fold,
                                          Hook&& hook = Hook{}) {
  // The blend kernels are VALU-issue bound: let a*b+c contract into v_fma_f32 here (the library is otherwise built
  // with -ffp-contract=off).  One rounding instead of two per contraction; results stay within the 1e-5 bar.
#pragma clang fp contract(fast)
  const float fx = p.fx, fy = p.fy;
  const unsigned lane_bits = p.lane_bits;
  const float g0 = p.g0, g1 = p.g1, g2 = p.g2, gz = p.gz;
  float R = p.R;  // R_k of the deepest entry handled so far
  for (int q = p.nchunks - 1; q >= 0; --q) {
    const int base = p.first + q * kStageBwd;
    const int cnt = __builtin_amdgcn_readfirstlane(min(kStageBwd, p.last - base));  // scalar loop bound
    // transmittance behind this chunk (the next chunk's start, or the end of the list) and in front of it; issued ahead
    // of the staging: their latency hides behind the barrier
    const float T_end = p.ck[(i64)(q + 1) * 256];
    const float T_start = (q > 0) ? p.ck[(i64)q * 256] : 1.0f;
    __syncthreads();
    stage_entries<true, DEPTH>(a, s, base, cnt, p.ttx * kTile, p.tty * kTile, da.z);
    __syncthreads();
    // only the entries whose rows reach this wave, deepest first (the fold skips this wave's rows for the others,
    // so nothing needs zeroing)
    const unsigned hits = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)s.hits[p.w][0]);
    // wave-uniform: some pixel of the strip underflows inside this chunk — quotients cannot be trusted for it
    const bool slow = __ballot(T_end < 1.17549435e-38f && T_start != 0.0f) != 0ull;
    float Tn = T_end;  // transmittance behind the entry in hand
    float T_group = T_start;
    int slow_group = -1;
    auto walk_chunk = [&](auto slow_tag) {
      constexpr bool kSlow = decltype(slow_tag)::value;
      unsigned h = hits;
      while (h) {
        const int k = 31 - __builtin_clz(h);
        h &= ~(1u << k);
        // straight-line for all 64 lanes; lanes outside the box / dropped pairs are zeroed with selects
        const float4 ge = s.geo[k];
        const float4 vi = s.vin[k];
        float4 co;
        if constexpr (!std::decay_t<Hook>::kOn) co = s.col[k];
        const bool in = (__float_as_uint(ge.w) & lane_bits) == lane_bits;
        const float dx = fx - ge.x, dy = fy - ge.y;
        // (d Λ) d^T (gs_model.py:495) as a dx^2 + (b + c) dx dy + d dy^2
        const float gv = __builtin_amdgcn_exp2f(dx * (vi.x * dx + vi.y * dy) + (vi.z * dy) * dy);
        const float og = ge.z * gv;
        const float anti = 1.0f - og;                       // gs_model.py:535
        float Tk, incl;
        if (!kSlow) {
          incl = Tn;                                          // what the forward pass left behind this pair
          Tk = (Tn == 0.0f) ? 0.0f : Tn * __builtin_amdgcn_rcpf(anti);
        } else {
          // T_k front to back from the chunk's start checkpoint: the same products in the same order for every entry, but not
          // from scratch for each — the product up to the entry's group of eight slots is formed once per group (the walk
          // visits the groups back to front: 0 + 8 + 16 + 24 slots) and only the group's own earlier slots per entry
          // (<= 7): about 160 entry evaluations per chunk instead of 496.  A scene whose pixels underflow at different
          // depths takes this branch in many chunks of a wave (blend backward 0.81 -> 2.0 ms with the Gaussians crowding the
          // image centre, before this).
          const unsigned below_group = (1u << (k & ~7)) - 1u;
          if ((k & ~7) != slow_group) {  // wave-uniform
            slow_group = k & ~7;
            T_group = T_start;
            for (unsigned hh = hits & below_group; hh; hh &= hh - 1) T_group = slow_factor(s, __builtin_ctz(hh), fx, fy, lane_bits, T_group);
          }
          Tk = T_group;
          for (unsigned hh = hits & ((1u << k) - 1u) & ~below_group; hh; hh &= hh - 1) Tk = slow_factor(s, __builtin_ctz(hh), fx, fy, lane_bits, Tk);
          incl = Tk * anti;
        }
        const bool keep = in & (incl != 0.0f);                // dropped when the inclusive product is exactly 0 (gs_model.py:560)
        Tn = in ? Tk : Tn;
        const float tg = keep ? Tk * gv : 0.0f;
        float c;
        if constexpr (std::decay_t<Hook>::kOn) {
          c = hook.c(s, k, tg * ge.z);
        } else {
          c = g0 * co.x + g1 * co.y + g2 * co.z;              // dL/dI . l
          if (DEPTH) c += gz * co.w;                            // + dL/dD z
        }
        const float d = c - R;
        body(k, ge.z, dx, dy, tg, d);
        R = keep ? R + og * d : R;                              // R_{k-1} = R_k + a_k (c_k - R_k)
      }
    };
    // two copies of the loop, chosen per chunk: the common one carries nothing of the other's (with one loop and the test inside,
    // the common path ran 2-6 % slower after the slow one grew its per-group product)
    if (__ballot(T_start != 0.0f) == 0ull) {
      // every pixel of the strip enters the chunk behind an exact zero: T_k = 0 throughout, every term is 0 and R does not
      // move — the wave hands the fold its zeros and goes on (a scene that crowds one region has half its pairs there)
      zero(hits);
    } else if (slow) {
      walk_chunk(std::true_type{});
    } else {
      walk_chunk(std::false_type{});
    }
    __syncthreads();
    // one thread per entry: the caller adds the entry's pixel rows in fixed order and writes the entry's slot
    for (int j = threadIdx.x; j < cnt; j += 256) fold(j, base + j);
  }
}

}  // namespace
