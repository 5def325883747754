/*
 * grouped_cumprod_hip.h — C ABI of libgrouped_cumprod_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the per-pixel alpha-compositing scan of
 * TaiseiNiman/SimpleGaussianSplat_tk71.  Every entry point below replaces one
 * function the reference registers in its pybind11 module `grouped_cumprod`
 * (reference: cuda_kernel/cuda_kernel.cpp:5-22).  Plain pointers and sizes only:
 * no torch types, no C++ types.  All pointers are DEVICE pointers on the
 * current HIP device; `stream` is a hipStream_t passed as void* (NULL = the
 * legacy default stream, which is what the reference launches on,
 * cuda_kernel/grouped_cumprod_backward.cu:56).
 *
 * Conventions shared by all entry points
 *   - arrays are 1-D, contiguous, fp32 values / int32 keys (reference contract:
 *     data_ptr<float>() / data_ptr<int>(), grouped_cumprod_forward.cu:8-10);
 *   - a "group" (one pixel's depth-sorted splat list) is a maximal run of equal
 *     ADJACENT keys — keys need not be globally sorted
 *     (thrust::equal_to<int>, grouped_cumprod_forward.cu:21);
 *   - outputs are caller-allocated and overwritten; nothing is retained by the
 *     library.  The forward scans (gcp_cumprod_forward, gcp_cumsum_forward,
 *     gcp_cumsum_reverse) may run EXACTLY in place, y == x, as the reference's
 *     thrust::inclusive_scan_by_key may (grouped_cumprod_forward.cu:17-23): the
 *     library then takes every carry from its tile descriptors instead of
 *     re-reading the neighbouring tile's inputs (0.5 instead of 0.7 of the HBM
 *     roof).  Any other overlap of an output with an input of the same call —
 *     shifted views, the backward, the carry and indexed forms — returns
 *     GCP_ERR_INVALID_ARGUMENT (blocks re-read raw inputs of the neighbouring
 *     tile while that tile's block is already storing).
 *   - launches are asynchronous on `stream`; no host synchronisation, no
 *     allocation when a workspace is supplied (graph-capturable);
 *   - every function returns GCP_OK (0) or a GCP_ERR_* code; n == 0 is a no-op;
 *   - results are deterministic run to run, bit for bit, whatever the timing: no value-carrying atomic, and a tile
 *     that is finished by the follow-up launch (below) gets the bits it would have got inside the main launch.
 *
 * Workspace: the scans are single-pass.  A group longer than one tile's raw look-back window (4096 elements)
 * continues on per-tile descriptors inside the same launch; a tile that would have to wait too long for another
 * tile's descriptor is finished by a small follow-up launch (a no-op otherwise), which completes the descriptor
 * tree in the main launch's fixed association and re-runs the tile with the carry taken from it.  Both need
 * gcp_workspace_bytes(n) bytes of scratch (0.4 % of one array).  Pass ws == NULL to let the library use an internal
 * per-device scratch buffer (grown with hipMalloc on demand — not graph-capturable, and not safe for concurrent
 * launches on two streams).  A caller-provided workspace must be zeroed ONCE before its first use
 * (gcp_workspace_init, or any memset of the whole buffer): it carries a launch counter and two descriptor sets used
 * alternately, each launch clearing the set the next one will publish into.  After that it may be reused by any
 * number of calls of any size that fits, as long as they are ORDERED on one stream (or otherwise never overlap).
 */
#ifndef GROUPED_CUMPROD_HIP_H
#define GROUPED_CUMPROD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCP_OK 0
#define GCP_ERR_INVALID_ARGUMENT 1 /* NULL pointer with n > 0, negative n, n too large, output overlapping an input */
#define GCP_ERR_WORKSPACE 2        /* workspace too small / misaligned */
#define GCP_ERR_HIP 3              /* a HIP call failed: see gcp_last_hip_error() */

#define GCP_ABI_VERSION 4

/* ABI version of the loaded library (== GCP_ABI_VERSION it was built with). */
int gcp_abi_version(void);

/* Hash of the kernel sources + headers + compile flags this binary was built from (the build recipe passes it as
 * -DGCP_SOURCE_HASH); the Python binding refuses a library whose hash differs from the checkout's. */
const char* gcp_source_hash(void);

/* hipError_t (as int) of the most recent failing HIP call on this host thread, 0 if none. */
int gcp_last_hip_error(void);

/* Static string for a GCP_* return code. */
const char* gcp_status_string(int status);

/* Bytes of scratch needed for arrays of n elements (multiple of 256). */
size_t gcp_workspace_bytes(int64_t n);

/* Zero a caller-provided workspace (async on `stream`); required once before its first use. */
int gcp_workspace_init(void* ws, size_t ws_bytes, void* stream);

/*
 * y[i] = prod of x[k] over k <= i in the same key-run as i   (inclusive).
 * Replaces grouped_cumprod_forward(x, key, y)
 *   reference: cuda_kernel/cuda_kernel.cpp:5,18;
 *              cuda_kernel/grouped_cumprod_forward.cu:6-24
 *              (thrust::inclusive_scan_by_key, equal_to<int>, multiplies<float>).
 * Traffic: 12 B / element (x, key in; y out).
 */
int gcp_cumprod_forward(const float* x, const int32_t* key, float* y, int64_t n,
                        void* ws, size_t ws_bytes, void* stream);

/*
 * y[i] = sum of x[k] over k <= i in the same key-run as i   (inclusive).
 * Replaces grouped_cumsum_forward(x, key, y)
 *   reference: cuda_kernel/cuda_kernel.cpp:14,21;
 *              cuda_kernel/grouped_cumsum_forward.cu:6-24 (thrust::plus<float>).
 * Traffic: 12 B / element.
 */
int gcp_cumsum_forward(const float* x, const int32_t* key, float* y, int64_t n,
                       void* ws, size_t ws_bytes, void* stream);

/*
 * VJP of gcp_cumprod_forward:
 *   grad_in[j] = sum_{i=j}^{end(j)-1} grad_out[i] * param_cumprod[i] / p'_j,
 *   p'_j = param[j] != 0 ? param[j] : 1e-8f,   end(j) = inv_len[inv[j]].
 * Replaces grouped_cumprod_backward(param, param_cumprod, grad_out, inv,
 *                                   grad_in, inv_len)
 *   reference: cuda_kernel/cuda_kernel.cpp:6-13,19-20;
 *              cuda_kernel/grouped_cumprod_backward.cu:9-41 (kernel), :43-65.
 * `inv` is the dense group id 0..G-1 of every element (non-decreasing runs),
 * `inv_len[g]` the exclusive end offset of group g (cuda_test.py:27).  The two
 * must describe the same partition (what gs_model.py / cuda_test.py pass;
 * gcp_check_groups() verifies it).  The group ends are taken from `inv_len`:
 * for every 1024-element range the kernel reads `inv` at the two ends only and
 * the entries of `inv_len` between them.  A range where those do not describe
 * the range exactly (ids outside [0, n_groups), ends out of order or not
 * bracketing the range, more than 255 groups) takes its ends from the runs of
 * `inv` instead; `inv_len` is never read outside [0, n_groups).  So a call with
 * `inv` = any key with the right runs and a one-entry dummy `inv_len` is still
 * served, at the old cost.  The reference's O(sum L^2) per-element loop is
 * replaced by one O(n) reverse segmented scan.
 * `param_cumprod` must be the inclusive grouped product of `param` over the
 * same groups, that is gcp_cumprod_forward's output for (`param`, `inv`): what
 * the reference's callers pass.  The kernel does not stream it: every
 * 1024-element range rebuilds its part from `param` (a differently associated
 * fp32 product, so grad_in agrees with gcp_cumprod_backward_given to rounding,
 * not bit for bit) and reads the given array only for one anchor element below
 * the range and for the look-back behind a 4096-element tile.  Which elements
 * are read depends on positions and data alone: results are deterministic.
 * Traffic: 12 B / element (param, grad_out in; grad_in out) plus anchors and
 * look-back (~0.3 B / element) and ~4 B per group (16 B / element on ranges
 * that fall back to `inv`).
 */
int gcp_cumprod_backward(const float* param, const float* param_cumprod,
                         const float* grad_out, const int32_t* inv, float* grad_in,
                         const int32_t* inv_len, int64_t n, int64_t n_groups,
                         void* ws, size_t ws_bytes, void* stream);

/*
 * The same sum with every factor taken from the GIVEN `param_cumprod`, which
 * may then be any array: the sum is linear in it, so the plain product times
 * a per-group factor (what gcp_cumprod_forward_carry produces) gives that
 * factor times the plain result.  Same operands and rules as
 * gcp_cumprod_backward.  Traffic: 16 B / element plus ~4 B per group (20 B /
 * element on ranges that fall back to `inv`).
 */
int gcp_cumprod_backward_given(const float* param, const float* param_cumprod,
                               const float* grad_out, const int32_t* inv, float* grad_in,
                               const int32_t* inv_len, int64_t n, int64_t n_groups,
                               void* ws, size_t ws_bytes, void* stream);

/*
 * Suffix form of gcp_cumsum_forward: y[i] = sum of x[k] over k >= i in the same
 * key-run.  The reference obtains this by flipping its arrays around
 * grouped_cumsum_forward (gs_model.py:716-722); this entry point does the same
 * scan in place without the two flips.  Traffic: 12 B / element.
 */
int gcp_cumsum_reverse(const float* x, const int32_t* key, float* y, int64_t n,
                       void* ws, size_t ws_bytes, void* stream);

/*
 * INDEXED forms: the sort -> scan -> un-sort sandwich of _create_alpha_brend (reference: gs_model.py:548
 * `anti_opacity[index]`, :551/:553 the scan, :555 `output[torch.argsort(index)]`) in ONE pass.  `x` and `y` are in the
 * caller's ORIGINAL pair order, `sorted_key` / `index` are what gcp_sort_pairs_u32 / gcp_sort_rects returned
 * (sorted_key[i] = key of original element index[i]; `index` a permutation of 0..n-1):
 *   y[index[i]] = scan over i, inside runs of equal adjacent sorted_key, of x[index[i]].
 * Neither the sorted copy of the values nor the sorted result is materialised.  Same association, determinism and
 * workspace rules as the plain scans.  Traffic: 16 B / element (key 4, index 4, gathered value 4, scattered result 4).
 */
int gcp_cumprod_forward_indexed(const float* x, const int32_t* sorted_key, const int32_t* index, float* y, int64_t n,
                                void* ws, size_t ws_bytes, void* stream);
int gcp_cumsum_forward_indexed(const float* x, const int32_t* sorted_key, const int32_t* index, float* y, int64_t n,
                               void* ws, size_t ws_bytes, void* stream);
int gcp_cumsum_reverse_indexed(const float* x, const int32_t* sorted_key, const int32_t* index, float* y, int64_t n,
                               void* ws, size_t ws_bytes, void* stream);

/*
 * Exact chunk carry.  Same scans, but group g starts from carry[g]
 * instead of the identity: y[i] = carry[inv[i]] (*|+) scan.  `inv` must be the DENSE group id
 * (it indexes `carry`, f32[n_groups]).  A caller that splits every pixel's depth-sorted list
 * into memory chunks (reference: gs_model.py:428, :675-686 forward, :634-643 backward) passes
 * the previous chunk's last inclusive value per pixel and gets the single-chunk result
 * exactly; the reference's own carry drops one factor per chunk boundary (its `amin` of the
 * EXCLUSIVE transmittance, gs_model.py:582-586).  For the reverse form the carry
 * is the suffix sum entering from the deeper chunk.  Traffic: 12 B / element + 4 B / group.
 */
int gcp_cumprod_forward_carry(const float* x, const int32_t* inv, const float* carry, float* y,
                              int64_t n, int64_t n_groups, void* ws, size_t ws_bytes, void* stream);
int gcp_cumsum_forward_carry(const float* x, const int32_t* inv, const float* carry, float* y,
                             int64_t n, int64_t n_groups, void* ws, size_t ws_bytes, void* stream);
int gcp_cumsum_reverse_carry(const float* x, const int32_t* inv, const float* carry, float* y,
                             int64_t n, int64_t n_groups, void* ws, size_t ws_bytes, void* stream);

/*
 * Debug aid (synchronises `stream`): checks that `inv` is a dense
 * non-decreasing group id starting at 0 and that inv_len[g] is the exclusive
 * end offset of run g.  *n_bad receives the number of violations found.
 */
int gcp_check_groups(const int32_t* inv, const int32_t* inv_len, int64_t n,
                     int64_t n_groups, int64_t* n_bad, void* stream);

/*
 * Operand checks for the two forms that index memory through an operand (debug aids like gcp_check_groups: they
 * allocate a scratch buffer and synchronise `stream`).  The scans themselves trust these operands — an `index` entry
 * outside [0, n) or an `inv` entry outside [0, n_groups) is an out-of-bounds device access.
 *   gcp_check_permutation: GCP_OK if index[0..n) is a permutation of 0..n-1 (what the indexed scans need: they read
 *     x[index[i]] and write y[index[i]]), GCP_ERR_INVALID_ARGUMENT otherwise; *n_bad (may be NULL) receives the
 *     number of entries that are out of range or repeat an earlier value.
 *   gcp_check_group_ids: GCP_OK if every inv[i] lies in [0, n_groups) (what the carry forms index `carry` with),
 *     GCP_ERR_INVALID_ARGUMENT otherwise; *n_bad (may be NULL) = entries out of range.
 *   gcp_set_validate_operands(1) (or environment GCP_VALIDATE_OPERANDS=1), process-wide, default off: every
 *     gcp_cum*_indexed call first runs gcp_check_permutation on its `index`, every gcp_cum*_carry call
 *     gcp_check_group_ids on its `inv`, and returns GCP_ERR_INVALID_ARGUMENT WITHOUT launching the scan when the
 *     operand is bad — at the price of one extra pass and a host synchronisation per call (not graph-capturable).
 */
int gcp_check_permutation(const int32_t* index, int64_t n, int64_t* n_bad, void* stream);
int gcp_check_group_ids(const int32_t* inv, int64_t n, int64_t n_groups, int64_t* n_bad, void* stream);
int gcp_set_validate_operands(int on);

/* Tuning / introspection (used by bench.py and the tests). */
/* Elements per scan tile of the loaded build. */
int gcp_tile_elems(void);
/* Number of tiles the most recent scan on workspace `ws` could not resolve inside the main launch (their wait for
 * another tile's descriptor ran out) and that the follow-up launch fixed up
 * (synchronises `stream`; ws == NULL selects the internal workspace). */
int gcp_last_fallback_tiles(void* ws, void* stream, int64_t* n_tiles);
/* Longest time (microseconds) a tile waits for another tile's descriptor before it leaves its carry to the
 * follow-up launch; default 200 (environment GCP_DESC_WAIT_US).  0 = look once, never wait; negative = skip the
 * descriptor walk altogether (every group that starts more than one tile back goes to the follow-up launch — the
 * two-pass behaviour, kept for tests and A/B timing).  Process-wide; results are bit-identical for every setting
 * (tests/test_scan_gpu.py::test_results_do_not_depend_on_the_descriptor_wait). */
int gcp_set_lookback_wait_us(int64_t us);
/* Number of tiles of that scan whose group started more than one tile back and that resolved their carry through
 * the descriptor look-back inside the main launch. */
int gcp_last_lookback_tiles(void* ws, void* stream, int64_t* n_tiles);


/* ------------------------------------------------------------------------------------------
 * Rows f1 / f2 of SURVEY.md §8: everything the reference's autograd Function does AROUND its
 * scan (reference: gs_model.py:598-663 _forward_batch/_backward_batch, :666-692 forward,
 * :786-820 backward), restated tile-based so that no splat-pixel pair array is ever
 * materialised.  Gaussians are given in depth order (front to back = array order) with integer
 * INCLUSIVE pixel boxes start_xy/end_xy int32[N,2] (x,y) (uitility.py:336-366), float means
 * [N,2], precision matrices vinv f32[N,2,2], opacity f32[N], colour l_d f32[N,3].  Images are
 * f32[(H+1),(W+1),3] (gs_model.py:505).  Tiles are 16x16 pixels.
 * ------------------------------------------------------------------------------------------ */

/* Tile grid of a (height+1) x (width+1) image. */
int gcp_tile_grid(int32_t width, int32_t height, int32_t* tiles_x, int32_t* tiles_y);

/* Exclusive prefix sum of int32; out has n+1 entries (out[n] = total). */
size_t gcp_scan_i32_workspace_bytes(int64_t n);
int gcp_exclusive_scan_i32(const int32_t* in, int32_t* out, int64_t n, void* ws, size_t ws_bytes,
                           void* stream);

/* f2, step 1: tile_off[g] = exclusive prefix of the number of tiles box g touches
 * (tile_off has n_gauss+1 entries).  Synchronises `stream` once to return the total K on the
 * host (the reference synchronises likewise: uitility.py:348 `.item()`).
 * ws: gcp_bin_workspace_bytes(n_gauss, 0) bytes. */
int gcp_bin_tiles_count(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss,
                        int32_t width, int32_t height, int32_t* tile_off,
                        int64_t* n_tile_pairs_host, void* ws, size_t ws_bytes, void* stream);
size_t gcp_bin_workspace_bytes(int64_t n_gauss, int64_t n_tile_pairs);
/* f2, step 2: tile_list[K] = Gaussian ids grouped by tile, depth order inside each tile (stable
 * radix sort of the Gaussian-major (tile, gaussian) entries); tile_start[n_tiles+1] = first entry
 * of every tile.  Replaces torch.sort / argsort / unique over M pixel keys
 * (gs_model.py:546-555, :582-586). */
int gcp_bin_tiles_fill(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss,
                       int32_t width, int32_t height, const int32_t* tile_off,
                       int64_t n_tile_pairs, int32_t* tile_start, int32_t* tile_list, void* ws,
                       size_t ws_bytes, void* stream);

/* The same binning in ONE call without a host read-back (graph-capturable): the caller bounds the entry count by
 * `capacity` (tile_list has `capacity` slots, ws = gcp_bin_workspace_bytes(n_gauss, capacity)); the real count stays on
 * the device.  info[0] = entries listed, info[1] = 1 if the capacity was too small — Gaussians whose entries did not
 * fit are then left out (front-most first kept) and get zero gradients; the caller reads info once per step, after the
 * fact, instead of synchronising inside the Function (the reference synchronises on `.item()` calls per chunk,
 * gs_model.py:677,793,801-802).  Buffers derived from the bins (checkpoints, backward workspace) are sized by
 * `capacity`, and `capacity` is what gcp_blend_backward takes as n_tile_pairs. */
int gcp_bin_tiles(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width,
                  int32_t height, int64_t capacity, int32_t* tile_off, int32_t* tile_start,
                  int32_t* tile_list, int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* f1 forward: image = sum over pairs of T * l * o * g with T the exclusive grouped cumprod of
 * (1 - o g) per pixel in depth order; pairs whose inclusive product is exactly 0 are dropped.
 * Replaces _forward_batch + index_put_(accumulate=True) (gs_model.py:598-624, :510-514).
 * t_ckpt: NULL (inference), or gcp_blend_checkpoint_floats(K, width, height) floats that receive every pixel's
 * transmittance at every GCP-internal checkpoint interval of its tile's list — what gcp_blend_backward restarts
 * its per-chunk front-to-back pass from (the reference keeps the whole M-length T array for that, gs_model.py:691). */
size_t gcp_blend_checkpoint_floats(int64_t n_tile_pairs, int32_t width, int32_t height);
int gcp_blend_forward(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy,
                      const float* vinv, const float* opacity, const float* l_d, int64_t n_gauss,
                      int32_t width, int32_t height, const int32_t* tile_start,
                      const int32_t* tile_list, float* image, float* t_ckpt, void* stream);

/* f1 backward: gradients of <image, grad_image> w.r.t. mean [N,2], vinv [N,2,2], opacity [N],
 * l_d [N,3].  `t_ckpt` is what gcp_blend_forward wrote for the same inputs and bins.  Replaces _backward_batch +
 * grad_list_to_gause (gs_model.py:627-663, :733-783).  Every tile list is walked BACK TO FRONT: the per-pixel
 * suffix sums the reference takes from a flipped grouped cumsum (gs_model.py:716-722) are carried as
 * S_k / (1 - o_k g_k) = T_k R_k with R_{k-1} = R_k + o_k g_k (dL/dI . l_k - R_k) (no cancellation, no division), so
 * a gradient's round-off is relative to the transmittance of its own layer at any depth.  grad_l is the TRUE
 * gradient (the reference's is channel-collapsed, gs_model.py:710-712,:763-766), and dL/dopacity is the true one
 * also at opacity == 0 (the reference drops the direct term there, gs_model.py:737-738).
 * ws: gcp_blend_backward_workspace_bytes(K). */
size_t gcp_blend_backward_workspace_bytes(int64_t n_tile_pairs);
int gcp_blend_backward(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy,
                       const float* vinv, const float* opacity, const float* l_d, int64_t n_gauss,
                       int32_t width, int32_t height, const int32_t* tile_off,
                       int64_t n_tile_pairs, const int32_t* tile_start, const int32_t* tile_list,
                       const float* t_ckpt, const float* grad_image, float* grad_mean,
                       float* grad_vinv, float* grad_opacity, float* grad_l, void* ws,
                       size_t ws_bytes, void* stream);

/* f1 with depth, alpha and a background colour: the same blend, the same bins and checkpoints, and per pixel p of the
 * (H+1) x (W+1) frame, with w_k = T_k o_k g_k the colour weights (pairs whose inclusive product is exactly 0 have
 * w_k = 0) and T_N the transmittance behind the pixel's whole list:
 *   depth_map(p) = sum_k w_k z_k       (z = depth [N], e.g. the camera-space depth; NOT divided by alpha)
 *   alpha_map(p) = 1 - T_N(p)
 *   image(p)     = sum_k w_k l_k + T_N(p) * background   (background: float[3] in DEVICE memory, or NULL = black, in which
 *                                                         case the image is gcp_blend_forward's bit for bit)
 * t_ckpt as for gcp_blend_forward (NULL: no backward).  The backward returns the exact derivatives of these definitions
 * for kept pairs (dropped pairs get zero) of <image, grad_image> + <depth_map, grad_depth_map> + <alpha_map,
 * grad_alpha_map>: grad_depth_map / grad_alpha_map may be NULL (zero); grad_depth [N] receives dL/dz; grad_background
 * (float[3], or NULL: not computed) sum_p grad_image(p) T_N(p), summed in a fixed order (no atomics).  With
 * n_gauss == 0 only grad_background is written.  ws: gcp_blend_backward_depth_workspace_bytes(K, width, height). */
int gcp_blend_forward_depth(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy,
                            const float* vinv, const float* opacity, const float* l_d, const float* depth,
                            const float* background, int64_t n_gauss, int32_t width, int32_t height,
                            const int32_t* tile_start, const int32_t* tile_list, float* image,
                            float* depth_map, float* alpha_map, float* t_ckpt, void* stream);
size_t gcp_blend_backward_depth_workspace_bytes(int64_t n_tile_pairs, int32_t width, int32_t height);
int gcp_blend_backward_depth(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy,
                             const float* vinv, const float* opacity, const float* l_d, const float* depth,
                             const float* background, int64_t n_gauss, int32_t width, int32_t height,
                             const int32_t* tile_off, int64_t n_tile_pairs, const int32_t* tile_start,
                             const int32_t* tile_list, const float* t_ckpt, const float* grad_image,
                             const float* grad_depth_map, const float* grad_alpha_map, float* grad_mean,
                             float* grad_vinv, float* grad_opacity, float* grad_l, float* grad_depth,
                             float* grad_background, void* ws, size_t ws_bytes, void* stream);

/* Stable sort of n uint32 keys that also returns the permutation: keys_out[i] = keys_in[index_out[i]], equal
 * keys keep their input order — what the reference asks of torch.sort for its pixel keys (gs_model.py:546-547;
 * depth order inside a pixel rides on that stability).  LSD radix sort over the low `key_bits` bits (8 per
 * pass; the keys must be < 2^key_bits), deterministic (no atomic decides a slot).  n < 2^31.
 * ws: gcp_sort_workspace_bytes(n) bytes. */
size_t gcp_sort_workspace_bytes(int64_t n);
int gcp_sort_pairs_u32(const uint32_t* keys_in, int64_t n, int32_t key_bits, uint32_t* keys_out,
                       int32_t* index_out, void* ws, size_t ws_bytes, void* stream);
/* The same sort with the reference's pixel key computed on the fly from its rect list (gs_model.py:538-541, :546:
 * key = y * 10000 + x of rects_xy[i] = (x, y)): the int32 key array of `unique()` never exists.  keys_out receives
 * the sorted keys (what `sorted_inv` is at gs_model.py:547), index_out the permutation.
 *   id_width == 0: key_bits must cover max(y) * 10000 + max(x) (24 at 1920x1080, 25 at 3840x2160);
 *   id_width  > 0: the caller knows the image: every x < id_width (= width + 1).  The passes then run on the compact
 *     ids y * id_width + x (same order, fewer bits, narrower digits: 3 x 7 bits at 1920x1080) and the last pass writes
 *     the reference's keys; key_bits must cover max(y) * id_width + max(x) and be <= 24. */
int gcp_sort_rects(const int32_t* rects_xy, int64_t n, int32_t key_bits, int32_t id_width, uint32_t* keys_out,
                   int32_t* index_out, void* ws, size_t ws_bytes, void* stream);
/* max over i of (y_i * 10000 + x_i) and min over i of min(x_i, y_i), written to out_dev[0], out_dev[1] (device int32[2]):
 * what a caller needs to choose key_bits when it does not know the image size. */
int gcp_rects_key_range(const int32_t* rects_xy, int64_t n, int32_t* out_dev, void* stream);

/* Rows a5 / a6 for callers that still hold the boxes their rect list was expanded from (gs_model.py:601 -> :607): key,
 * stable sort, gather, grouped scan and un-sort of _create_alpha_brend (gs_model.py:546-555) as ONE walk of the tile lists of
 * gcp_bin_tiles*.  x / inclusive: f32[M] in the reference's Gaussian-major rect order (uitility.py:336-366); box_off:
 * int32[n_gauss + 1] exclusive prefix sums of the clamped box sizes (gcp_box_sizes + gcp_exclusive_scan_i32).
 *   inclusive[pair] = product (mode 0) / sum (mode 1) of x over the pairs of the same pixel up to and including this one
 *   in depth order; mode 2: sum from this one to the deepest (grad_cumsum's flipped scan, gs_model.py:716-722).
 * Every pixel is scanned sequentially in depth order (the association of the CPU statement).  8 B / pair.  Feed the result
 * to gcp_compact_finish.  n_pairs = M = box_off[n_gauss], the length of x and inclusive (< 2^31; up to 2^30 the kernel
 * addresses pairs by 32-bit byte offsets).  width + 1 must stay below 2^22 (2^24 beyond 2^30 pairs): a pair's position is
 * formed with one 24-bit multiply by the box width; GCP_ERR_INVALID_ARGUMENT otherwise.  dropped_per_tile: NULL, or int32[ceil(n_pairs / 4096)] that receives, for
 * every 4096 consecutive pairs, how many inclusive values are exactly 0 (integer adds, one per wave and list entry that
 * has any: deterministic) — the per-tile counts gcp_compact_finish would otherwise read the array once more for. */
int gcp_pairs_scan_boxes(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width, int32_t height,
                         const int32_t* tile_start, const int32_t* tile_list, const int32_t* box_off, const float* x,
                         float* inclusive, int64_t n_pairs, int32_t mode, int32_t* dropped_per_tile, void* stream);

/* The walk writing the FINAL values of _create_alpha_brend (gs_model.py:557-564), so that a list that drops nothing needs no
 * compaction pass at all.  Same walk as gcp_pairs_scan_boxes, same arguments, but every pair receives
 *   keep[pair]   = (inclusive != 0)                                  (gs_model.py:560, :575-578)
 * as one byte per pair (the call sets every byte to 1 and the walk clears the bytes of the pairs it drops), and every KEPT pair
 *   values[pair] = inclusive / x[pair] (mode 0, gs_model.py:562)  or  inclusive - x[pair] (modes 1, 2, :564)
 * — the fp32 operation gcp_compact_finish would apply to the stored inclusive value: the same bits.  values[pair] of a dropped
 * pair is unspecified: in mode 0 a wave whose 64 pixels have all reached the product 0 stores nothing there (whatever the
 * buffer held stays), and gcp_compact_kept_write moves kept values only;
 * dropped_per_tile (required, int32[ceil(n_pairs / 4096)]) counts them per 4096 consecutive pairs.  prepared != 0: the
 * caller has already run gcp_pairs_finish_prepare(keep, dropped_per_tile, n_pairs, stream) on the same stream — the two
 * fills, which depend on nothing but n_pairs, can then be queued BEFORE the host waits for gcp_rects_cut's info8 and run
 * while it does.  When
 * gcp_compact_kept_count reports that everything was kept, `values` and `keep` ARE the result of _create_alpha_brend
 * (8 B per pair + the 1 B fill of the mask instead of 21); otherwise gcp_compact_kept_write moves the kept values together
 * (5 B read + 4 B written per pair). */
int gcp_pairs_finish_prepare(uint8_t* keep, int32_t* dropped_per_tile, int64_t n_pairs, void* stream);
int gcp_pairs_finish_boxes(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width, int32_t height,
                           const int32_t* tile_start, const int32_t* tile_list, const int32_t* box_off, const float* x,
                           float* values, uint8_t* keep, int64_t n_pairs, int32_t mode, int32_t* dropped_per_tile, int32_t prepared,
                           void* stream);

/* The stream compaction that remains after gcp_pairs_finish_boxes, split at the one device->host read that sizes the result
 * (the reference's `output[mask]`, gs_model.py:575-578, synchronises likewise):
 *   gcp_compact_kept_count: count_dev[0] (device int32) = number of set bytes of keep[begin, end) — the rows a
 *     `cutting_number` slice leaves (gs_model.py:557-559) — and, in ws, the kept count of every 4096-element tile of the range
 *     (ONE launch when the walk's counts serve; the prefix sums are made by gcp_compact_kept_write, only when needed).
 *     dropped_per_tile (may be NULL; what the walk counted for the WHOLE array of n_total elements) is used instead of
 *     reading the keep bytes when the range starts at a multiple of 4096 and ends at one or at n_total.
 *   gcp_compact_kept_write: values_out[k] = values_in[i] for the k-th kept i of [begin, end), in order; `ws` as the count
 *     call left it, for the same range.  Not needed when the count equals end - begin.
 * Stable, no atomics, deterministic.  ws: gcp_compact_kept_workspace_bytes(end - begin). */
size_t gcp_compact_kept_workspace_bytes(int64_t n);
int gcp_compact_kept_count(const uint8_t* keep, const int32_t* dropped_per_tile, int64_t n_total, int64_t begin, int64_t end,
                           int32_t* count_dev, void* ws, size_t ws_bytes, void* stream);
int gcp_compact_kept_write(const float* values_in, const uint8_t* keep, int64_t begin, int64_t end, float* values_out, void* ws,
                           size_t ws_bytes, void* stream);

/* The rect list of the reference cut back into rectangles (gcp_pairs.hip), so that _create_alpha_brend / grad_cumsum can
 * take the tile-walk route (gcp_pairs_scan_boxes) from nothing but `rects` — which `_create_rects` always writes as a
 * concatenation of row-major boxes (gs_model.py:480-482, uitility.py:336-366).  Valid for ANY list: a list that is not made
 * of boxes yields about as many rectangles as elements, and the caller then sorts instead.
 *   gcp_rects_rows: rows = maximal runs (x, y), (x+1, y), ...  row_start[k] = index of the k-th row's first element,
 *     row_start[rows] = n, row_xy[k] = its (x, y); both have room for row_capacity entries.  info (device int32[5]) =
 *     {rows, max x, max y, min coordinate, not_boxes}; not_boxes != 0 — bit 1: the list has more than row_capacity - 1 rows;
 *     bit 0: an x >= 10000 (the reference's key y * 10000 + x then merges different pixels, gs_model.py:538-541: only the
 *     key-based sort route reproduces its groups) or a y >= 2^17 — nothing was written, sort instead.  gcp_rects_rows_capacity(n) = n / 2 + 2
 *     is what a list of boxes is allowed; a caller whose list starts or ends with c single-pixel carry rows (the
 *     `cutting_number` rows of gs_model.py:611, :636 — lexicographically sorted unique pixels: they come out as one-pixel-wide
 *     rectangles) passes c + gcp_rects_rows_capacity(n - c).
 *   gcp_rows_rectangles: rectangles = maximal runs of rows with equal first x and length and y growing by one.
 *     rect_row[b] = first row of rectangle b (room for n_rows + 1 entries; rect_row[rectangles] = n_rows).  info (device
 *     int32[2]) = {rectangles, 0}.
 *   gcp_rectangle_boxes: start_xy / end_xy (inclusive, int32[n_rects][2]) and box_off (int32[n_rects + 1], box_off[b] =
 *     index of the rectangle's first pair, box_off[n_rects] = n): the arguments of gcp_bin_tiles* and gcp_pairs_scan_boxes.
 * Each cut is a stable stream compaction without atomics on the data path (per-tile counts, one exclusive scan, ranked
 * writes); the first reads the M-sized list once.  ws: the matching *_workspace_bytes. */
/* The three cuts AND the binning's counting pass in ONE call with nothing read back in between (gcp_rects_cut): what
 * _create_alpha_brend / grad_cumsum run by default.  Every stage takes its predecessor's count from device memory; the caller
 * reads info8 once:
 *   info8 (device int32[8]) = {rows, max x, max y, min coordinate, flags, rectangles, K, 0}
 *   flags: 0 = start_xy / end_xy / box_off (as gcp_rectangle_boxes) and tile_off (as gcp_bin_tiles_count: exclusive prefix
 *     sums of the tiles every rectangle touches, tile_off[rectangles] = K — the image being [0, max x] x [0, max y], the
 *     binning's clamp is the identity) are valid: hand them to gcp_bin_tiles_fill(…, max x, max y, tile_off, K, …).
 *     1 = a coordinate the walk cannot take (x >= 10000, y >= 2^17: see gcp_rects_rows) — sort instead;
 *     2 = more rows than there is room for (slot_rows per 4096-pair tile on average; tiles that need more draw on a shared
 *       pool of n / 32 records) — take the step-by-step cut (gcp_rects_rows: room for a row per two pairs) or sort;
 *     4 = more than rect_capacity rectangles; 8 = K does not fit int32.  A negative min coordinate: refuse the list.
 *   slot_rows: row records a tile of boxes may park (<= 4096; 512 serves boxes of 8 columns and more).  carry_front /
 *     carry_back: the list starts / ends with that many single-pixel carry rows (the `cutting_number` rows of gs_model.py:611,
 *     :636): their tiles get one slot per element.  rect_capacity: rectangles start_xy / end_xy (int32[cap][2]), box_off and
 *     tile_off (int32[cap + 1]) have room for.
 * Scratch (ws, 256-byte aligned): 8 B x slot_rows per tile for the parked records, as much again for the rows (kept
 * packed), the pool and a few words per tile: 2.3 B per pair at slot_rows = 512 (+ 28 B per rectangle of capacity in the
 * caller's arrays: 0.45 B per pair at 64 pairs per rectangle), against gcp_rects_rows' 8 B + the caller's 6 B per pair. */
size_t gcp_rects_cut_workspace_bytes(int64_t n, int64_t carry_front, int64_t carry_back, int32_t slot_rows, int64_t rect_capacity);
int gcp_rects_cut(const void* rects_xy, int32_t rects_are_int64, int64_t n, int64_t carry_front, int64_t carry_back, int32_t slot_rows,
                  int64_t rect_capacity, int32_t* start_xy, int32_t* end_xy, int32_t* box_off, int32_t* tile_off, int32_t* info8,
                  void* ws, size_t ws_bytes, void* stream);

/* ---- the per-pixel carry of the reference's chunked calls ----------------------------------
 * `_create_alpha_brend_min(rects, T)` (gs_model.py:582-586; every forward chunk, :609 / :615) =
 * torch.unique(rects, dim=0) + scatter_reduce(amin) over its inverse, and `create_grad_alphabrend_min(rects, grad)`
 * (:724-730; every backward chunk, :639 / :643) = the same with the pair's own index as the value.
 * gcp_pixels_min: for every distinct pixel of the list — in (x, y) ascending order, the row order of
 * torch.unique(dim=0) — its coordinates (out_xy, [capacity][2] of the element width of rects_xy) and the minimum of
 * `values` over its pairs (out_val; a NaN among them gives NaN, as amin does); with values = NULL, the index of its
 * FIRST pair, as the float the reference carries it in (gs_model.py:728: exact below 2^24, rounded to nearest-even
 * above).  One pass over the list (integer minima into an image-sized table: the result does not depend on the order
 * the pairs arrive in), then the table is read out; nothing M-sized is written or sorted.
 *   width, height: every coordinate must lie in [0, width] x [0, height] (the reference's (H+1) x (W+1) image,
 *   gs_model.py:505); info (device int32[4]) = {distinct pixels, 1 if a coordinate lay outside (those pairs are
 *   skipped), 0, 0}.  Rows beyond `capacity` are counted but not written ((width + 1) * (height + 1) always suffices).
 *   ws: gcp_pixels_min_workspace_bytes(width, height) (0: image too large), 256-byte aligned.
 * gcp_pixels_range: out3 (device int32[3]) = {max x, max y, min coordinate} of a list, for callers that do not hold
 * the image size. */
int gcp_pixels_range(const void* rects_xy, int32_t rects_are_int64, int64_t n, int32_t* out3, void* stream);
size_t gcp_pixels_min_workspace_bytes(int32_t width, int32_t height);
int gcp_pixels_min(const void* rects_xy, int32_t rects_are_int64, const float* values /* NULL: the pair's index */, int64_t n,
                   int32_t width, int32_t height, void* out_xy, float* out_val, int64_t capacity, int32_t* info, void* ws,
                   size_t ws_bytes, void* stream);

size_t gcp_rects_rows_workspace_bytes(int64_t n);
int64_t gcp_rects_rows_capacity(int64_t n);
int gcp_rects_rows(const int32_t* rects_xy, int64_t n, int64_t row_capacity, int32_t* row_start, int32_t* row_xy, int32_t* info,
                   void* ws, size_t ws_bytes, void* stream);
/* The same on a list of int64 coordinates — the dtype the reference's own make_rect_points_parallel returns
 * (uitility.py:336-366: `start + ix`, ix from torch.arange): read where it lies instead of being narrowed by a pass of its
 * own.  A coordinate outside [0, 2^31) is reported as a negative minimum (info[3] < 0). */
int gcp_rects_rows_i64(const int64_t* rects_xy, int64_t n, int64_t row_capacity, int32_t* row_start, int32_t* row_xy, int32_t* info,
                       void* ws, size_t ws_bytes, void* stream);
size_t gcp_rows_rectangles_workspace_bytes(int64_t n_rows);
int gcp_rows_rectangles(const int32_t* row_start, const int32_t* row_xy, int64_t n_rows, int32_t* rect_row, int32_t* info, void* ws,
                        size_t ws_bytes, void* stream);
int gcp_rectangle_boxes(const int32_t* rect_row, const int32_t* row_start, const int32_t* row_xy, int64_t n_rects, int64_t n,
                        int32_t* start_xy, int32_t* end_xy, int32_t* box_off, void* stream);

/* The tail of _create_alpha_brend (gs_model.py:557-564) on the un-sorted inclusive scan values, elements [begin, end)
 * of the original pair order (the reference's `cutting_number` slices, :557-559):
 *   keep[j]   = inclusive[begin + j] != 0                                   (:560, :575-578)
 *   values[k] = inclusive[i] / self[i] (mode 0, :562) or inclusive[i] - self[i] (mode 1, :564)
 *               for the k-th kept i, in order                               (the boolean-mask compaction)
 * count_dev[0] (device int32) receives the number of kept elements.  Stable stream compaction in two launches (per-tile
 * counts, then ranks from one exclusive scan of them): no atomics, deterministic.  values needs room for end - begin
 * floats.  ws: gcp_compact_workspace_bytes(end - begin).  Traffic: 17 B / element.
 * dropped_per_tile: NULL, or what gcp_pairs_scan_boxes counted for THIS inclusive array (int32 per 4096 elements of
 * the whole array, how many are exactly 0): the counting launch is then skipped (13 B / element); begin must be a
 * multiple of 4096. */
size_t gcp_compact_workspace_bytes(int64_t n);
int gcp_compact_finish(const float* inclusive, const float* self, int64_t begin, int64_t end, int32_t mode, float* values,
                       uint8_t* keep, int32_t* count_dev, const int32_t* dropped_per_tile, void* ws, size_t ws_bytes, void* stream);

/* The index plumbing of _create_alpha_brend around the scan, with the int32 permutation of gcp_sort_pairs_u32:
 * gcp_gather_f32: dst[i] = src[index[i]] (gs_model.py:548); gcp_unsort_finish: full[index[i]] = inclusive[i] / x_i
 * (mode 0, gs_model.py:562) or inclusive[i] - x_i (mode 1, :564) with x_i = sorted_x[i], keep[index[i]] =
 * (inclusive[i] != 0) (gs_model.py:560) — the un-sort (:555) fused with the steps that follow the compaction. */
int gcp_gather_f32(const float* src, const int32_t* index, float* dst, int64_t n, void* stream);
int gcp_unsort_finish(const float* inclusive, const float* sorted_x, const int32_t* index, float* full,
                      uint8_t* keep, int64_t n, int32_t mode, void* stream);

/* The reference's Gaussian-major rect list (Utilities.make_rect_points_parallel, uitility.py:336-366;
 * _create_rects, gs_model.py:480-482) for callers that still want it: box sizes (clamped to the image), then —
 * given their exclusive prefix sum box_off[N+1] — rects_xy int32[M,2] and optionally the owning Gaussian of
 * every pair (gause_points_inv, gs_model.py:768-773). */
int gcp_box_sizes(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width,
                  int32_t height, int32_t* box_size, void* stream);
int gcp_expand_rects(const int32_t* start_xy, const int32_t* end_xy, const int32_t* box_off,
                     int64_t n_gauss, int64_t n_pairs, int32_t width, int32_t height,
                     int32_t* rects_xy, int32_t* pair_gauss /* may be NULL */, void* stream);

/* f2, CSR export for callers of the scan API: per-pixel pair counts (row-major over the
 * (H+1)x(W+1) image = ascending pixel key y*10000+x) and box sizes; then, given their exclusive
 * prefix sums, pair_gauss[M] (Gaussian of every pair, pixel-major, depth order) and
 * pair_index[M] (the pair's position in the reference's Gaussian-major rect list) — i.e. the
 * `index` torch.sort(stable) returns at gs_model.py:547, bit for bit. */
int gcp_pixel_lists_count(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss,
                          int32_t width, int32_t height, const int32_t* tile_start,
                          const int32_t* tile_list, int32_t* pixel_count, int32_t* box_size,
                          void* stream);
int gcp_pixel_lists_fill(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss,
                         int32_t width, int32_t height, const int32_t* tile_start,
                         const int32_t* tile_list, const int32_t* pixel_off,
                         const int32_t* box_off, int32_t* pair_gauss, int32_t* pair_index,
                         int32_t* pair_key /* optional: y*10000+x of every pair, may be NULL */,
                         void* stream);

/* ---- the caller's camera projection, fused ----------------------------------------------
 * One camera of GS_model_with_param.forward up to the Function call (reference: gs_model.py:289-365, :404-425;
 * helpers uitility.py:231-287, :431-462): world->camera, pinhole projection, pixel covariance J W S W^T J^T + 1e-6 I,
 * 3-sigma box from its eigen-decomposition, its inverse, SH colour (real spherical harmonics in the usual 3DGS order and
 * sign, sh_degree 0..3, coefficients [n_basis][3] per Gaussian with n_basis >= (sh_degree + 1)^2: rows above the active
 * degree are stored, not read, and get zero gradients), sigmoid opacity, the cull test and the clamped integer box.
 *   cam_P float[12] = [R|t] row major, cam_K float[9] row major, both in device memory;
 *   mean, quat_xyzw, log_scale, opacity_logit and sh_coeff need only the 4-byte
 *   alignment of a float — views at any element offset into a larger buffer are fine; an array that happens to be 16-byte
 *   aligned is read with wider loads, with the same result bit for bit.  This holds for every gcp_project_* and gcp_splat_*
 *   entry point; the arrays that do need more (record, vinv, start_xy, end_xy, mean_xy) say so below;
 *   box_clamp = the float the 3-sigma half extents are clamped to before truncation (gs_model.py:364-365).
 * gcp_project_forward writes, in the Gaussians' own order: record float[n_gauss][16] (16-byte aligned; opaque, read
 * back by gcp_project_gather), sort_key int32 (bit pattern of the positive camera depth, 0x7fffffff for culled
 * Gaussians: a stable ascending sort of the keys IS the depth order of gs_model.py:356 with the kept ones first),
 * keep uint8 (the cull mask of gs_model.py:405-407) and row_of = -1.
 * gcp_project_gather: for the first n_kept entries of the sorted permutation `perm`, the Function's arguments in
 * depth order (boxes, pixel means, boxsize = gs_model.py:425, Sigma'^-1 [4], opacity, l_d [3], index = Gaussian id)
 * and row_of[index[r]] = r.  With `keep` (the mask gcp_project_forward wrote) and n_kept = n_gauss, the list holds ALL
 * Gaussians without the kept count ever being read back: the culled ones follow the kept ones with an empty box (binned
 * into no tile, blended nowhere, zero gradients) — the capture-safe form; keep = NULL: the first n_kept entries only.
 * gcp_project_backward: gradients of (mean, quaternion, log scale, opacity logit, SH coefficients), n_gauss rows
 * each, all rows written (zeros where row_of < 0), from those of (Sigma'^-1, opacity, l_d) in list order.
 * gcp_project_gather_depth / gcp_project_backward_depth: the same plus each Gaussian's camera-space depth z (the
 * positive depth the sort key holds; 0 for a culled entry of the capture-safe form) in list order, and its gradient
 * grad_depth [n_kept] (dz/dmean = row 2 of [R|t]).
 * gcp_project_forward_sh / gcp_project_backward_sh: the same with the direction the SH basis is evaluated on chosen by
 * sh_frame: 0 = -t/|t| in camera coordinates (what the entry points above use: the reference's call site,
 * gs_model.py:335-338), 1 = the world-space unit vector from the camera centre to the Gaussian, R^T t/|t| (R = the
 * rotation of [R|t], taken to be orthonormal) — the convention of other 3DGS renderers; the colour then does not change
 * when the camera rolls about its axis.  gcp_project_backward_sh serves both backwards: grad_depth may be NULL (no depth
 * gradient).  Every entry point returns GCP_ERR_INVALID_ARGUMENT, before any HIP call, for sh_degree outside 0..3,
 * n_basis < (sh_degree + 1)^2 or sh_frame outside {0, 1}; n_gauss == 0 is a no-op after those checks. */
int gcp_project_forward(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                        const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                        int32_t n_basis, int32_t width, int32_t height, float box_clamp, float* record, int32_t* sort_key,
                        uint8_t* keep, int32_t* row_of, void* stream);
int gcp_project_gather(const float* record, const int32_t* perm, int64_t n_kept, int32_t* start_xy, int32_t* end_xy,
                       int32_t* mean_xy, int64_t* boxsize, float* vinv, float* alpha, float* l_d, int64_t* index,
                       int32_t* row_of, const uint8_t* keep /* may be NULL */, void* stream);
int gcp_project_backward(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                         const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                         int32_t n_basis, const int32_t* row_of, const float* grad_vinv, const float* grad_alpha,
                         const float* grad_l_d, float* grad_mean, float* grad_quat, float* grad_log_scale,
                         float* grad_opacity_logit, float* grad_sh_coeff, void* stream);
int gcp_project_gather_depth(const float* record, const int32_t* perm, int64_t n_kept, int32_t* start_xy, int32_t* end_xy,
                             int32_t* mean_xy, int64_t* boxsize, float* vinv, float* alpha, float* l_d, float* depth,
                             int64_t* index, int32_t* row_of, const uint8_t* keep /* may be NULL */, void* stream);
int gcp_project_backward_depth(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                               const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                               int32_t n_basis, const int32_t* row_of, const float* grad_vinv, const float* grad_alpha,
                               const float* grad_l_d, const float* grad_depth, float* grad_mean, float* grad_quat,
                               float* grad_log_scale, float* grad_opacity_logit, float* grad_sh_coeff, void* stream);
int gcp_project_forward_sh(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                           const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                           int32_t n_basis, int32_t sh_frame, int32_t width, int32_t height, float box_clamp, float* record,
                           int32_t* sort_key, uint8_t* keep, int32_t* row_of, void* stream);
int gcp_project_backward_sh(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                            const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                            int32_t n_basis, int32_t sh_frame, const int32_t* row_of, const float* grad_vinv,
                            const float* grad_alpha, const float* grad_l_d, const float* grad_depth /* may be NULL */,
                            float* grad_mean, float* grad_quat, float* grad_log_scale, float* grad_opacity_logit,
                            float* grad_sh_coeff, void* stream);

/* ---- the projection with float centres, covariance dilation and colour clamp (gcp_splat.hip) ----------
 * The chain of gcp_project_forward_sh / gcp_project_gather[_depth] / gcp_project_backward_sh with the three conventions of
 * other 3DGS renderers, each chosen by an argument and each with its exact gradient:
 *   cov_eps (>= 0, finite): added to the diagonal of the pixel covariance in place of 1e-6 — J W S W^T J^T + cov_eps I;
 *     0.3 is the usual screen-space dilation, 1e-6 the reference's.  det = a d - b c + 1e-6 stays; the 3-sigma half extents
 *     come from the dilated covariance.
 *   mean_offset (finite): the pixel centre is kept as two FLOATS, c = clamp(p, +-(2^31 - 1) / 1000) + mean_offset, where
 *     gcp_project_forward truncates p to integers.  Half-pixel convention: the model crops [1:, 1:] of the (H+1) x (W+1)
 *     frame, so pixel i of the cropped image is frame pixel i + 1, and in the COLMAP / 3DGS convention that pixel's centre
 *     lies at i + 0.5 in the coordinates of K.  With mean_offset = 0.5 the blend evaluates dx = (i + 1) - (px + 0.5) =
 *     (i + 0.5) - px: what those renderers evaluate.  0 keeps the reference's coordinates.
 *     The box goes around the float centre: with h = min(half extent, box_clamp), columns (int)ceil(cx - h) ..
 *     (int)floor(cx + h) and rows likewise (the floats clamped to +-(2^31 - 1) / 1000 before conversion): every pixel within
 *     the clamped 3-sigma extent and no other.  A Gaussian is kept when its depth is > 0, the box is not empty (x1 >= x0,
 *     y1 >= y0) and x0 < width, x1 > 0, y0 < height, y1 > 0; the stored box is clamped to [0, width] x [0, height].
 *   clamp_colour (0 or 1): 1 = every channel of the SH colour is max(sum, 0); a channel whose sum is < 0 passes no gradient
 *     to the coefficients or the direction, a sum of exactly 0 does.
 * gcp_splat_forward writes record / sort_key / keep / row_of as gcp_project_forward_sh does (record words 4-5: the float
 * centre).  gcp_splat_gather: as gcp_project_gather, with mean_xy float[n_kept][2] (8-byte aligned, finite for every entry)
 * and `depth` optional — NULL, or float[n_kept] as gcp_project_gather_depth fills it; `keep` selects the capture-safe form
 * as there.  gcp_splat_backward: as gcp_project_backward_sh (grad_depth may be NULL) plus grad_mean_xy, NULL or
 * float[n_kept][2] in list order: dL/dc, chained through px = ph0 / pz, py = ph1 / pz, ph = K t (the full K, skew
 * included), pz = max(ph2, 1e-2) — dph0 = gx / pz, dph1 = gy / pz, dph2 = -(gx ph0 + gy ph1) / pz^2 where ph2 > 1e-2, else
 * 0 — into the camera-space gradient K^T dph that reaches `mean` through R; zero where the centre was clamped.
 * Every entry point returns GCP_ERR_INVALID_ARGUMENT, before any HIP call, for sh_degree / n_basis / sh_frame out of range
 * (as gcp_project_forward_sh), cov_eps negative or not finite, mean_offset not finite, clamp_colour outside {0, 1}, a NULL
 * array with Gaussians to process, or a misaligned record / vinv / mean_xy; n_gauss == 0 (n_kept == 0) is a no-op after
 * the checks of the scalar arguments.
 *
 * gcp_splat_forward_flags / gcp_splat_backward_flags: the same calls with `int32_t flags` where clamp_colour stands, a set
 * of GCP_SPLAT_* bits; any other bit is refused with GCP_ERR_INVALID_ARGUMENT before any HIP call.  gcp_splat_forward and
 * gcp_splat_backward are these with flags = clamp_colour (still refusing a clamp_colour outside {0, 1}).
 *   GCP_SPLAT_CLAMP_COLOUR: clamp_colour = 1.
 *   GCP_SPLAT_ANTIALIAS: opacity compensation of the dilation.  Sigma' = Sigma + cov_eps I paints sqrt(det Sigma' / det Sigma)
 *     times the energy of the Gaussian it replaces; with this bit the record's opacity word (the gather's alpha) holds
 *     sigmoid(o) rho,  rho = sqrt(max(det0, 0) / det),  det0 = a0 d0 - b c  on the clamped pixel covariance BEFORE cov_eps,
 *     det = (a0 + cov_eps)(d0 + cov_eps) - b c + 1e-6, the determinant Sigma'^-1 is formed with.  Every other word of the
 *     record, sort_key, keep and row_of are what they are without the bit.  Backward: grad_alpha is dL/d(sigmoid(o) rho);
 *     grad_opacity_logit = grad_alpha rho s (1 - s) with s = sigmoid(o), and dL/drho = grad_alpha s is added to the
 *     covariance's gradient through both determinants, (rho / 2)(adj(Sigma)^T / det0 - adj(Sigma')^T / det), under the
 *     rule of the clamped entries.  A Gaussian with det0 <= 0 (a covariance that underflowed or lost its rank to rounding)
 *     has rho = 0: its opacity is exactly 0, its logit gets 0, and nothing passes through rho.  Without a dilation
 *     (cov_eps = 1e-6) rho is 1 up to the two 1e-6: the bit is meant for cov_eps > 0 such as 0.3. */
#define GCP_SPLAT_CLAMP_COLOUR 1
#define GCP_SPLAT_ANTIALIAS 2
int gcp_splat_forward(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                      const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                      int32_t n_basis, int32_t sh_frame, int32_t width, int32_t height, float box_clamp, float cov_eps,
                      float mean_offset, int32_t clamp_colour, float* record, int32_t* sort_key, uint8_t* keep, int32_t* row_of,
                      void* stream);
int gcp_splat_gather(const float* record, const int32_t* perm, int64_t n_kept, int32_t* start_xy, int32_t* end_xy, float* mean_xy,
                     int64_t* boxsize, float* vinv, float* alpha, float* l_d, float* depth /* may be NULL */, int64_t* index,
                     int32_t* row_of, const uint8_t* keep /* may be NULL */, void* stream);
int gcp_splat_backward(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                       const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                       int32_t n_basis, int32_t sh_frame, const int32_t* row_of, const float* grad_vinv, const float* grad_alpha,
                       const float* grad_l_d, const float* grad_depth /* may be NULL */, float cov_eps, int32_t clamp_colour,
                       const float* grad_mean_xy /* may be NULL */, float* grad_mean, float* grad_quat, float* grad_log_scale,
                       float* grad_opacity_logit, float* grad_sh_coeff, void* stream);
int gcp_splat_forward_flags(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                            const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                            int32_t n_basis, int32_t sh_frame, int32_t width, int32_t height, float box_clamp, float cov_eps,
                            float mean_offset, int32_t flags, float* record, int32_t* sort_key, uint8_t* keep, int32_t* row_of,
                            void* stream);
int gcp_splat_backward_flags(const float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit,
                             const float* sh_coeff, const float* cam_P, const float* cam_K, int64_t n_gauss, int32_t sh_degree,
                             int32_t n_basis, int32_t sh_frame, const int32_t* row_of, const float* grad_vinv,
                             const float* grad_alpha, const float* grad_l_d, const float* grad_depth /* may be NULL */,
                             float cov_eps, int32_t flags, const float* grad_mean_xy /* may be NULL */, float* grad_mean,
                             float* grad_quat, float* grad_log_scale, float* grad_opacity_logit, float* grad_sh_coeff,
                             void* stream);

/* ---- the caller's training loss, fused ---------------------------------------------------
 * (1 - lambda) * mean|a - b| + lambda * (1 - mean SSIM(a, b)) of gs_control.py:180-182 (kornia.metrics.ssim with an
 * 11-tap Gaussian window and reflect padding), over `planes` = batch * channels planes of height x width floats.
 *   window11_host: the 11 normalised window weights, HOST memory (passed to the kernel by value); c1, c2 = (0.01 L)^2,
 *   (0.03 L)^2.
 * gcp_ssim_l1_forward writes partial[2 * b] = sum of the SSIM map and partial[2 * b + 1] = sum of |a - b| over block
 * b of gcp_ssim_blocks() (no atomics: the caller adds them, in any fixed order, for a reproducible loss) and, when
 * the three map pointers are non-NULL, dSSIM/dmu1, dSSIM/dE[a^2], dSSIM/dE[ab] per pixel for the backward.
 * gcp_ssim_l1_backward: grad_img1 = scales[0] * dSum(SSIM)/da + scales[1] * sign(a - b), scales in DEVICE memory
 * (so that an upstream gradient needs no host read); the adjoint of the reflect-padded blur is exact. */
int64_t gcp_ssim_blocks(int64_t planes, int32_t height, int32_t width);
int gcp_ssim_l1_forward(const float* img1, const float* img2, int64_t planes, int32_t height, int32_t width,
                        const float* window11_host, float c1, float c2, float* dm_dmu1, float* dm_de11, float* dm_de12,
                        float* partial, void* stream);
int gcp_ssim_l1_backward(const float* img1, const float* img2, const float* dm_dmu1, const float* dm_de11, const float* dm_de12,
                         int64_t planes, int32_t height, int32_t width, const float* window11_host, const float* scales,
                         float* grad_img1, void* stream);

/* ---- held-out evaluation: per-image squared error, L1 and SSIM in one pass ------------------------------------------
 * img, ref: float[images][channels][height][width].  For every image, out[3 i ..] = (mean (a - b)^2, mean |a - b|, mean
 * SSIM(a, b)) over its channels * height * width elements, in double; SSIM as in gcp_ssim_l1_forward (11-tap window in
 * HOST memory, reflect padding, c1, c2).  flags: a set of GCP_METRICS_* bits; with GCP_METRICS_CLAMP img (only img: ref is
 * the photograph) is clamped to [0, 1] as it is read, so all three terms see the clamped value.  PSNR is
 * 10 log10(L^2 / out[3 i]) and is left to the caller.
 * Two kernels on `stream`, no device->host read, no allocation (capturable): one block per 32 x 16 tile writes its three
 * float sums to partial (float[3 * gcp_ssim_blocks(images * channels, height, width)], written before it is read); one
 * block per image adds that image's partials in double in a fixed order.  No atomics: the same bits on every run, and an
 * image's numbers do not depend on what else is in the batch.
 * GCP_ERR_INVALID_ARGUMENT before any HIP call: images < 0, channels <= 0, height or width < 6, a NULL window, an unknown
 * flag bit; with images > 0 a NULL array or more than 2^31 - 1 blocks.  images == 0 is a no-op after the scalar checks. */
#define GCP_METRICS_CLAMP 1
int gcp_image_metrics(const float* img, const float* ref, int64_t images, int32_t channels, int32_t height, int32_t width,
                      const float* window11_host, float c1, float c2, int32_t flags, float* partial, double* out, void* stream);

/* ---- per-camera exposure compensation fused into the loss and the metrics ------------------------------------------------
 * img, ref: float[images][3][height][width] (three channels are implied); exposure: DEVICE float[images][3][4], one colour
 * affine per image.  The loss and the metrics are those above of y against ref, with
 *   y_c = E[c][0] x_0 + E[c][1] x_1 + E[c][2] x_2 + E[c][3]
 * formed by one fixed chain of fused multiply-adds as the tiles are staged; y is never written to memory, and E = [I | 0]
 * gives the bits of the plain entry points.
 * gcp_ssim_l1_forward_exposure: partial and the three maps (with respect to y; all three or none) as gcp_ssim_l1_forward
 * with planes = 3 * images, so partial is float[gcp_ssim_blocks(3 * images, ...)][2] in the same order.
 * gcp_ssim_l1_backward_exposure: with g_c = scales[0] * dSum(SSIM)/dy_c + scales[1] * sign(y_c - b_c),
 *   grad_img[i][k] = sum_c E[i][c][k] g_c (may be NULL),
 *   grad_exposure[i][c][k] = sum over the pixels of image i of g_c x_k, [i][c][3] = sum of g_c (may be NULL; every entry
 *   is written otherwise).  One block per (image, tile) writes twelve float sums to partial_e (float[gcp_exposure_blocks()][12],
 *   needed with grad_exposure); one block per image adds them in double in a fixed order.  No atomics: the same bits on
 *   every run, and an image's gradients depend on that image alone.
 * gcp_image_metrics_exposure: gcp_image_metrics of y; with GCP_METRICS_CLAMP y (after the compensation) is clamped.
 * No allocation and no device->host read (capturable).  GCP_ERR_INVALID_ARGUMENT before any HIP call: images < 0, height or
 * width < 6, a NULL window, an unknown flag bit; with images > 0 more than 2^31 - 1 blocks, a NULL pointer among the
 * required arrays, a partial set of maps, grad_img and grad_exposure both NULL.  images == 0 is a no-op after the scalar
 * checks.  gcp_exposure_blocks: images * tiles, 0 on bad input. */
int64_t gcp_exposure_blocks(int64_t images, int32_t height, int32_t width);
int gcp_ssim_l1_forward_exposure(const float* img, const float* ref, const float* exposure, int64_t images, int32_t height,
                                 int32_t width, const float* window11_host, float c1, float c2, float* dm_dmu1, float* dm_de11,
                                 float* dm_de12, float* partial, void* stream);
int gcp_ssim_l1_backward_exposure(const float* img, const float* ref, const float* exposure, const float* dm_dmu1,
                                  const float* dm_de11, const float* dm_de12, int64_t images, int32_t height, int32_t width,
                                  const float* window11_host, const float* scales, float* grad_img /* may be NULL */,
                                  float* partial_e, float* grad_exposure /* may be NULL */, void* stream);
int gcp_image_metrics_exposure(const float* img, const float* ref, const float* exposure, int64_t images, int32_t height,
                               int32_t width, const float* window11_host, float c1, float c2, int32_t flags, float* partial,
                               double* out, void* stream);

/* ---- the caller's optimiser step ---------------------------------------------------------
 * torch.optim.Adam's update (no weight decay, no amsgrad; gs_model.py:43-47, :64-67) of one parameter tensor of n
 * floats, in place: exp_avg = beta1 exp_avg + (1 - beta1) grad; exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) grad^2;
 * param -= lr / (1 - beta1^step) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^step) + eps).  step counts from 1.
 * Hyper-parameters are doubles (1 - beta and the bias corrections are formed in double, as torch does, then rounded
 * once).  All four arrays 16-byte aligned. */
int gcp_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1,
                  double beta2, double eps, int64_t step, void* stream);

/* The same update of up to GCP_ADAM_MAX_TENSORS tensors in ONE call, with step counts and learning rates in device
 * memory (a captured call replays the step and rate of the replay, not of the capture) and an optional row mask
 * (the sparse / visibility-masked Adam of other 3DGS trainers).  Two launches on `stream`, no wait, no allocation.
 *   host arrays of length n_tensors: param, grad, exp_avg, exp_avg_sq (device pointers, 16-byte aligned, contiguous
 *     float32 [rows[t]][width[t]]), rows (>= 0), width (>= 1), step (device pointers to one int32 each: the number of
 *     steps already taken).  They are read during the call only.
 *   lr: DEVICE float[n_tensors].  scal: device float[2 n_tensors], scratch of the caller.
 *   visible: NULL, or device uint8[rows], non-zero = visible; every tensor of the call must then have the same `rows`.
 * Prologue kernel, one thread per tensor: step[t] += 1; bc1 = 1 - beta1^step, bc2 = 1 - beta2^step in double;
 * scal[2t] = (float)(lr[t] / bc1), scal[2t + 1] = (float)(1 / sqrt(bc2)): the two scalars gcp_adam_step forms on the host.
 * Main kernel: every block belongs to one tensor and grid-strides over that tensor's float4s with gcp_adam_step's arithmetic.
 * Element e of tensor t lies in row e / width[t].  An element of an invisible row keeps param, exp_avg and exp_avg_sq bit
 * for bit; a float4 whose four elements all lie in invisible rows is neither loaded nor stored; one that straddles a
 * visible and an invisible row is loaded whole, updated where visible and stored whole.  step[t] advances whatever the
 * mask holds, also for a tensor with rows == 0.
 * GCP_ERR_INVALID_ARGUMENT before any HIP call: n_tensors outside 0..GCP_ADAM_MAX_TENSORS, a beta outside [0, 1), and with
 * n_tensors > 0 a NULL host array, lr, scal or step[t], width < 1, rows < 0, rows * width beyond int64, a NULL or
 * misaligned tensor with elements to process, a mask with unequal rows.  n_tensors == 0 is a no-op. */
#define GCP_ADAM_MAX_TENSORS 8
int gcp_adam_step_multi(int32_t n_tensors, float* const* param, const float* const* grad, float* const* exp_avg,
                        float* const* exp_avg_sq, const int64_t* rows, const int32_t* width, int32_t* const* step,
                        const float* lr, float* scal, const uint8_t* visible, double beta1, double beta2, double eps,
                        void* stream);

/* ---- the caller's density control on the device (csrc/gcp_densify.hip) ---------------------
 * Split / clone / prune of gs_model.py:201-265 as one pass whose decisions are all taken from the state BEFORE it, each
 * Gaussian taking one action, and which carries the optimiser's moments of the surviving rows along.  Every entry point
 * validates before any HIP call (negative sizes, NULL with rows to process, a non-finite threshold or extent,
 * n_split < 1: GCP_ERR_INVALID_ARGUMENT); n_gauss == 0 or n_rows == 0 is a no-op.  No value-carrying atomics: results
 * are bit-identical whatever the launch shape.
 *
 * gcp_densify_accumulate: the screen-space statistic of one camera.  grad_xy f32[m,2] = d loss / d centre in list order
 * (8-byte aligned), index i64[m] = the list's Gaussian ids.  Per entry: norm_acc[id] += sqrtf(gx^2 + gy^2) with
 * gx = grad_xy[i][0] * scale_x, gy = grad_xy[i][1] * scale_y; view_count[id] += 1.  A Gaussian appears at most once in
 * a camera's list, so the update uses no atomics.  An id outside [0, n_gauss) is never written through: the entry is
 * skipped and the call still returns GCP_OK (the launch is asynchronous; nothing is read back).  n_bad (device int32, may
 * be NULL, zeroed by the caller) counts such ids for a caller that wants to refuse them; norm_acc == view_count == NULL
 * with n_bad: only that count, nothing accumulated — how gs_model.accumulate_screen_grads(validate=True) refuses a list as
 * a whole before it adds anything.
 *
 * gcp_densify_plan: with g = norm_acc / max(view_count, 1), s = max_k exp(log_scale_k) and
 * hot = view_count > 0 && g >= grad_threshold:
 *     split  hot && s >  dense_extent   n_split fresh children of scale s / (0.8 n_split); the parent disappears
 *     clone  hot && s <= dense_extent   2 rows: the survivor and one fresh copy
 *     keep   otherwise                  1 row
 * then the prune test on the OUTPUT rows: none is written if sigmoid(opacity_logit) < min_opacity or the rows' largest
 * scale (for children the reduced one) > prune_extent.  Writes count[n] (rows per Gaussian), action[n] (0 keep, 1 clone,
 * 2 split) and offset[n+1], the exclusive prefix sum of count: offset[n] = the number of output rows, the one value
 * the caller reads back.  A plan that could exceed int32 (n_gauss * max(n_split, 2) > INT32_MAX) is refused.
 * ws: gcp_densify_plan_workspace_bytes(n_gauss) bytes.
 *
 * gcp_densify_fill: for every output row r in offset[i] .. offset[i+1]: src_row[r] = i, kind[r] = 0 survivor (moments
 * carried) / 1 fresh copy / 2 split child.  A Gaussian's rows are contiguous, in Gaussian order; a split child's number
 * is r - offset[src_row[r]].
 *
 * gcp_densify_rows: dst[r, :] = src[src_row[r], :] for rows of `width` floats (mode 0, parameters), or that where
 * kind[r] == 0 and 0.0f elsewhere (mode 1, Adam moments).  Arrays 4-byte aligned; 16-byte accesses where width is a
 * multiple of 4 and both arrays are 16-byte aligned.  A src_row outside [0, n_src_rows) gives a row of zeros.
 *
 * gcp_densify_split: for rows with kind == 2, parent p = src_row[r], child c = r - offset[p]:
 *     mean_out[r] = mean[p] + R(q[p] / max(|q[p]|, 1e-8)) (sigma * z),  log_scale_out[r] = log(sigma / (0.8 n_split)),
 * sigma = exp(log_scale[p]), R as uitility.py:231-254 (x, y, z, w).  z: Philox4x32-10, key (seed_lo, seed_hi), counter
 * (p, c, 0, 0); outputs r0..r3 -> u_k = (r_k + 0.5) 2^-32 (ln u_k taken from 1 - u_k above 1/2, so the radius keeps float
 * accuracy up to r_k = 2^32 - 1; the angle 2 pi u_k from the float32 u_k, absolute error 2e-7); z0 = sqrt(-2 ln u0) cos(2 pi u1), z1 = sqrt(-2 ln u0)
 * sin(2 pi u1), z2 = sqrt(-2 ln u2) cos(2 pi u3).  Other rows are not touched.  mean / log_scale are the arrays BEFORE
 * the pass (n_gauss rows), mean_out / log_scale_out those after it (n_rows rows). */
int gcp_densify_accumulate(const float* grad_xy, const int64_t* index, int64_t m, float scale_x, float scale_y, float* norm_acc,
                           int32_t* view_count, int64_t n_gauss, int32_t* n_bad, void* stream);
size_t gcp_densify_plan_workspace_bytes(int64_t n_gauss);
int gcp_densify_plan(const float* norm_acc, const int32_t* view_count, const float* log_scale, const float* opacity_logit,
                     int64_t n_gauss, float grad_threshold, float dense_extent, float prune_extent, float min_opacity,
                     int32_t n_split, int32_t* count, uint8_t* action, int32_t* offset, void* ws, size_t ws_bytes, void* stream);
int gcp_densify_fill(const uint8_t* action, const int32_t* offset, int64_t n_gauss, int64_t n_rows, int32_t* src_row, uint8_t* kind,
                     void* stream);
int gcp_densify_rows(const float* src, int64_t n_src_rows, const int32_t* src_row, const uint8_t* kind, int64_t n_rows,
                     int32_t width, int32_t mode, float* dst, void* stream);
int gcp_densify_split(const float* mean, const float* quat_xyzw, const float* log_scale, const int32_t* src_row, const uint8_t* kind,
                      const int32_t* offset, int64_t n_gauss, int64_t n_rows, int32_t n_split, uint32_t seed_lo, uint32_t seed_hi,
                      float* mean_out, float* log_scale_out, void* stream);

/* ---- MCMC density control on the device (3DGS-MCMC, Kheradmand et al., NeurIPS 2024; csrc/gcp_mcmc.hip) -------------
 * Dead Gaussians are relocated onto live ones drawn with probability proportional to opacity, the scene grows to a row
 * count the HOST fixes, and a small opacity-gated noise moves the positions after every optimiser step.  No gradient
 * statistic, no threshold and no device->host read: n_rows is the caller's arithmetic, the total weight is read from
 * cum[n_gauss] on the device, and no entry point waits for the stream.  n_gauss = rows before the pass, n_rows >= n_gauss
 * rows after it; a SLOT is an output row r that draws a source: r >= n_gauss, or r < n_gauss and dead.  Every entry point
 * validates before any HIP call (a negative size, n_rows < n_gauss, n_gauss == 0 with n_rows > 0, n_rows > INT32_MAX,
 * n_gauss * w_max > INT32_MAX, w_max not a power of two in [1, 2^16], NULL with rows to process, a non-finite
 * min_opacity, amount, k or o0: GCP_ERR_INVALID_ARGUMENT); n_gauss == 0 (then n_rows == 0) is a no-op that touches
 * nothing.  The one atomic counts draws in an integer: results are bit-identical whatever the launch shape.
 *
 * gcp_mcmc_weights: o = sigmoid(opacity_logit) in float32; dead = !(o > min_opacity) (NaN is dead);
 * weight[i] = dead ? 0 : clamp((int)floorf(o * w_max), 1, w_max); cum[n_gauss + 1] = the exclusive prefix sum of weight,
 * cum[n_gauss] = T.  w_max: the caller passes the largest power of two <= 2^16 with n_gauss * w_max <= INT32_MAX, so
 * the draw is an exact integer one at 2^16 levels up to 32 767 Gaussians and 2^11 levels at 10^6.
 * ws: gcp_mcmc_workspace_bytes(n_gauss) bytes.
 *
 * gcp_mcmc_draw: zeroes times[n_gauss], then for every output row r < n_rows: a slot runs Philox4x32-10 with key
 * (seed_lo, seed_hi) and counter (r, 0, 0, 2), t = ((uint64)out[0] * T) >> 32, src_row[r] = the s with
 * cum[s] <= t < cum[s + 1] (an upper bound by binary search over cum[1..n_gauss]; never a dead row), times[s] += 1;
 * every other row gets src_row[r] = r.  T == 0 (everything dead): src_row[r] = r mod n_gauss, times stays 0.  Then
 * kind[r] = 0 (survivor: gcp_densify_rows mode 1 carries its moments) iff r < n_gauss && src_row[r] == r &&
 * times[r] == 0, else 1 (fresh: moments 0.0).  The rows themselves are gathered with gcp_densify_rows.
 *
 * gcp_mcmc_values: for every output row r with p = src_row[r], c = times[p] > 0 and n = min(c + 1, 51), in float64 from
 * the arrays BEFORE the pass (n_gauss rows): o = sigmoid(opacity_logit[p]), o' = 1 - (1 - o)^(1/n),
 *     D = sum_{i=1..n} sum_{k=0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1),
 * log_scale_out[r, :] = (float)(log_scale[p, :] + log(o / D)), opacity_out[r] = (float)logit(clamp(o', min_opacity,
 * 1 - 2^-23)): the source and every slot that drew it receive the same values.  Rows with c == 0 are not touched.
 *
 * gcp_mcmc_noise: in place on mean f32[n_gauss, 3], float32: o = sigmoid(opacity_logit), gate = 1 / (1 + expf(-k (o0 - o))),
 * z = the three normals of gcp_densify_split's mapping from Philox counter (i, 0, 0, 1), R = R(q / max(|q|, 1e-8)),
 * s = exp(log_scale): mean[i] += amount * gate * R (s^2 (.) (R^T z)).  quat_xyzw 16-byte aligned (rows are read whole).
 * 44 bytes read and 12 written per Gaussian. */
size_t gcp_mcmc_workspace_bytes(int64_t n_gauss);
int gcp_mcmc_weights(const float* opacity_logit, int64_t n_gauss, float min_opacity, int32_t w_max, int32_t* weight, int32_t* cum,
                     void* ws, size_t ws_bytes, void* stream);
int gcp_mcmc_draw(const int32_t* cum, int64_t n_gauss, int64_t n_rows, uint32_t seed_lo, uint32_t seed_hi, int32_t* src_row,
                  int32_t* times, uint8_t* kind, void* stream);
int gcp_mcmc_values(const float* opacity_logit, const float* log_scale, const int32_t* src_row, const int32_t* times, int64_t n_gauss,
                    int64_t n_rows, float min_opacity, float* opacity_out, float* log_scale_out, void* stream);
int gcp_mcmc_noise(float* mean, const float* quat_xyzw, const float* log_scale, const float* opacity_logit, int64_t n_gauss,
                   float amount, float k, float o0, uint32_t seed_lo, uint32_t seed_hi, void* stream);

/* Per-Gaussian contribution to one camera's image (gcp_contrib.hip): with the pair rule of gcp_blend_forward to the letter
 * — a pixel belongs to a Gaussian if it lies inside the Gaussian's integer box clamped to the frame, g = exp(-0.5 d Λ d^T),
 * T the exclusive product of 1 - o g over the earlier list entries whose box holds the pixel, w = T o g and w = 0 where
 * the inclusive product T (1 - o g) is exactly 0 —
 *   w_max[i] = max_p w,   w_sum[i] = sum_p w   over the pixels p of Gaussian i's box; both 0 for an empty box and for a
 * Gaussian the binning did not list (a capture-safe capacity that was too small).  Same bins as the blend: tile_off,
 * tile_start, tile_list of gcp_bin_tiles*, n_tile_pairs = K (or the capacity).  No atomics: every sum is taken in a fixed
 * order, two calls give the same bits.  n_gauss == 0: nothing is touched; n_tile_pairs == 0: both outputs are zeroed.
 * No stream synchronise, no read-back.  ws: gcp_blend_contrib_workspace_bytes(K) (8 bytes per entry). */
size_t gcp_blend_contrib_workspace_bytes(int64_t n_tile_pairs);
int gcp_blend_contrib(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv,
                      const float* opacity, int64_t n_gauss, int32_t width, int32_t height,
                      const int32_t* tile_off, int64_t n_tile_pairs, const int32_t* tile_start, const int32_t* tile_list,
                      float* w_max, float* w_sum, void* ws, size_t ws_bytes, void* stream);

/* Absolute screen-space gradient of one camera (gcp_absgrad.hip; AbsGS, gsplat's absgrad).  For every splat-pixel pair
 * (k, p) that gcp_blend_backward counts, with its T_k, g_k, c_k = <grad_image(p), l_k> (+ grad_depth_map(p) z_k) and suffix
 * recursion R_k (R = 0 behind the list; depth call: <grad_image, background> - grad_alpha_map where T_N != 0):
 *   m(k,p) = T_k o_k g_k (c_k - R_k) Λ_k (p - mean_k),   Λ (p - mean) = (A dx + C dy, B dx + D dy), vinv = [[A, B], [C, D]]
 * and m = 0 outside the box clamped to the frame and for a dropped pair.  grad_mean[k] of the backward is sum_p m(k,p);
 *   absgrad[k] = ( sum_p |m_x(k,p)|, sum_p |m_y(k,p)| ),  float [N,2]
 * — 0 for an empty box and for a Gaussian the binning did not list.  The arguments are the backward's inputs (the same
 * bins, `t_ckpt` of the matching forward); grad_depth_map, grad_alpha_map and background may be NULL (zero / black), every
 * other pointer is required.  No atomics: two calls give the same bits.  n_gauss == 0: nothing is touched;
 * n_tile_pairs == 0: absgrad is zeroed.  No stream synchronise, no read-back, no allocation.
 * ws: gcp_blend_absgrad_workspace_bytes(K) (8 bytes per entry). */
size_t gcp_blend_absgrad_workspace_bytes(int64_t n_tile_pairs);
int gcp_blend_absgrad(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv,
                      const float* opacity, const float* l_d, int64_t n_gauss, int32_t width, int32_t height,
                      const int32_t* tile_off, int64_t n_tile_pairs, const int32_t* tile_start, const int32_t* tile_list,
                      const float* t_ckpt, const float* grad_image, float* absgrad, void* ws, size_t ws_bytes, void* stream);
int gcp_blend_absgrad_depth(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv,
                            const float* opacity, const float* l_d, const float* depth, const float* background,
                            int64_t n_gauss, int32_t width, int32_t height, const int32_t* tile_off, int64_t n_tile_pairs,
                            const int32_t* tile_start, const int32_t* tile_list, const float* t_ckpt, const float* grad_image,
                            const float* grad_depth_map, const float* grad_alpha_map, float* absgrad, void* ws,
                            size_t ws_bytes, void* stream);

/* Depth distortion of one camera (gcp_distort.hip; the distortion loss of Mip-NeRF 360, 2DGS, gsplat's distloss).  Per pixel
 * p, over its kept pairs k = 1..n front to back with the pair rule of gcp_blend_forward to the letter (w_k = T_k o_k g_k, a
 * pair whose inclusive product is exactly 0 is dropped: w = 0, no gradient), z_k = depth[k] the per-Gaussian scalar
 * gcp_blend_forward_depth takes, A_k = sum_{j<=k} w_j and B_k = sum_{j<=k} w_j z_j:
 *   dist(p) = 2 sum_k w_k (z_k A_{k-1} - B_{k-1})      ( = sum_{i>j} 2 w_i w_j (z_i - z_j) )
 * — the order-based form: it equals sum_{i,j} w_i w_j |z_i - z_j| whenever z is non-decreasing in list order, as the camera
 * depth the list is sorted by is (ties contribute 0).  Like the depth map it is not divided by alpha and is in units of z.
 * In float32 neither kernel forms z_k A - B (a difference of numbers of size z A whose value has size dz A: a surface 1e-2
 * thick at depth 20 lost three digits): both carry s(z) = sum_j w_j |z - z_j| along the pixel's own contributing pairs by
 * differences of NEIGHBOURING depths, so every term is of the size of the spread of the pixel's own layers, whatever the offset.
 * The forward writes three maps of (H+1)(W+1) floats: dist, a_n = A_n and b_n = sum_j w_j (z_L - z_j), L the pixel's last
 * contributing pair — NOT B_n = sum w z: opaque state for the backward of the same bins and depths (a_n is NOT the alpha map:
 * behind an exactly opaque layer alpha = 1 while A_n is the sum in front of the dropped pair).  n_gauss == 0: the maps are zeroed.
 * The backward takes them back with t_ckpt of a checkpointed blend forward ON THE SAME BINS and G = grad_dist = dL/d dist;
 * with the inclusive suffix sum SA_k = sum_{j>=k} w_j it runs the blend backward's own recursion on
 *   c_k = 2 G s_k,  s_k = sum_j w_j |z_k - z_j|,   dL/dz_k = 2 G w_k (A_n - 2 SA_k + w_k)
 * s carried back to front as s_k = s_k' + (z_k' - z_k)(2 SA_k' - A_n) from s_L = b_n, k' the contributing pair behind k
 * (R = 0 behind the list, R_{k-1} = R_k + a_k (c_k - R_k), dL/do_k = T_k g_k (c_k - R_k), common = T_k a_k (c_k - R_k)) and
 * WRITES grad_mean [N,2], grad_vinv [N,4], grad_opacity [N], grad_depth [N]: the recursion is linear in c, so these add to
 * the gradients of gcp_blend_backward_depth.  0 for an empty box and for a Gaussian the binning did not list.
 * n_gauss == 0: nothing is touched; n_tile_pairs == 0: the four outputs are zeroed.  No atomics: two calls give the same
 * bits.  No stream synchronise, no read-back, no allocation.
 * ws: gcp_blend_distort_backward_workspace_bytes(K) (28 bytes per entry). */
int gcp_blend_distort_forward(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv,
                              const float* opacity, const float* depth, int64_t n_gauss, int32_t width, int32_t height,
                              const int32_t* tile_start, const int32_t* tile_list, float* dist_map, float* a_n, float* b_n,
                              void* stream);
size_t gcp_blend_distort_backward_workspace_bytes(int64_t n_tile_pairs);
int gcp_blend_distort_backward(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv,
                               const float* opacity, const float* depth, int64_t n_gauss, int32_t width, int32_t height,
                               const int32_t* tile_off, int64_t n_tile_pairs, const int32_t* tile_start,
                               const int32_t* tile_list, const float* t_ckpt, const float* a_n, const float* b_n,
                               const float* grad_dist, float* grad_mean, float* grad_vinv, float* grad_opacity,
                               float* grad_depth, void* ws, size_t ws_bytes, void* stream);

/* Median depth of one camera (gcp_median.hip; 2DGS's depth_ratio = 1, gsplat's 2DGS mode, RaDe-GS): the depth of the layer at
 * which the pixel's transmittance falls through 1/2.  The pair rule is gcp_blend_forward's to the letter, for pixel p of the
 * (H+1) x (W+1) frame over its list front to back: a pair must lie inside the integer box clamped to the frame,
 * g = exp(-1/2 d Λ d^T), T_k is the exclusive product of 1 - o g, w_k = T_k o_k g_k, and a pair whose inclusive product is
 * exactly 0 is dropped (w = 0).  A pair CONTRIBUTES iff w_k != 0 (the distortion's notion of a contributing pair).
 *   m(p)            = the LAST contributing pair k of p with T_k > 0.5   (strict)
 *   median(p)       = z_m          — a copy of depth[m], not an interpolation, NOT multiplied by alpha
 *   median_index(p) = the Gaussian's row in the call's arrays (what tile_list holds), int32
 *   median(p) = 0, median_index(p) = -1 where p has no contributing pair
 * — 2DGS's `if (T > 0.5) { median_depth = depth; median_contributor = ...; }`.  Where the pixel's transmittance crosses 1/2, m
 * is the layer that crosses it; where it never does (alpha < 1/2), the pixel's last contributing layer; behind an exactly
 * opaque dropped pair, the last contributing pair in front of it.  The forward uses the arithmetic of the forward blend,
 * contraction included: the T compared with 1/2 is the T the image was painted with.  It stops walking a tile's list once no
 * pixel of the tile is above 1/2, which changes no bit of either output.  It writes median_map (float) and median_index
 * (int32), (H+1)(W+1) each, and uses no checkpoints.  n_gauss == 0: median_map is 0 and median_index -1 everywhere.
 * Backward: median is piecewise constant in everything but z_m,
 *   dL/dz_g = sum_{p : median_index(p) = g} G(p),  G = grad_median = dL/d median;   zero to mean, vinv and opacity
 * summed per tile in pixel order into the Gaussian-major slot of the (tile, Gaussian) entry, then per Gaussian over its slots
 * in order: no float atomics, two calls give the same bits.  median_index: what the forward wrote ON THE SAME BINS (an index
 * that is not a row whose box reaches the pixel's tile is ignored).  It WRITES grad_depth [N]: 0 for a Gaussian no pixel
 * picked and for one the binning did not list.  n_gauss == 0: nothing is touched; n_tile_pairs == 0: grad_depth is zeroed.
 * No stream synchronise, no read-back, no allocation.
 * ws: gcp_blend_median_backward_workspace_bytes(K) (4 bytes per entry). */
int gcp_blend_median_forward(const int32_t* start_xy, const int32_t* end_xy, const float* mean_xy, const float* vinv,
                             const float* opacity, const float* depth, int64_t n_gauss, int32_t width, int32_t height,
                             const int32_t* tile_start, const int32_t* tile_list, float* median_map, int32_t* median_index,
                             void* stream);
size_t gcp_blend_median_backward_workspace_bytes(int64_t n_tile_pairs);
int gcp_blend_median_backward(const int32_t* start_xy, const int32_t* end_xy, int64_t n_gauss, int32_t width, int32_t height,
                              const int32_t* tile_off, int64_t n_tile_pairs, const int32_t* tile_start,
                              const int32_t* median_index, const float* grad_median, float* grad_depth, void* ws, size_t ws_bytes,
                              void* stream);

/* ---- the 3-D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024; csrc/gcp_filter3d.hip) ---------------------------
 * A stage in FRONT of the projection: every Gaussian is low-pass filtered in world space by an isotropic Gaussian of size
 * filter[i] = phi >= 0 (the caller forms it from the sampling rate: phi = sqrt(0.2) / rate in the published code) and its
 * opacity is scaled so that it keeps its mass.  One thread per Gaussian in a grid-stride loop of at most 4096 blocks of 256;
 * no atomics, one writer per output word, no arithmetic that depends on a thread's position: the same bits whatever the
 * launch shape.  No device->host read, no stream wait, no allocation.  Every entry point validates before any HIP call (a
 * negative size or one above INT32_MAX, a non-finite near_z or margin, margin < 0, NULL with rows to process:
 * GCP_ERR_INVALID_ARGUMENT); n_gauss == 0, and for the rate n_cams == 0, is a no-op that touches nothing and launches nothing.
 *
 * gcp_filter3d_rate: mean f32[n_gauss,3], P f32[n_cams,3,4] world->camera, K f32[n_cams,3,3], wh i32[n_cams,2] = (W, H) ->
 * rate f32[n_gauss].  For camera c, in float32 with every sum left to right: t = P_c [mean; 1], u = fx t.x / t.z + cx,
 * v = fy t.y / t.z + cy with fx = K[0][0], fy = K[1][1], cx = K[0][2], cy = K[1][2] (the skew K[0][1] is ignored).  The
 * camera SEES the Gaussian iff t.z > near_z and -margin W <= u <= (1 + margin) W and -margin H <= v <= (1 + margin) H (a NaN
 * is not seen); rate[i] = max over the seeing cameras of max(fx, fy) / t.z, 0 where none sees it.  Mip-Splatting's values:
 * near_z = 0.2, margin = 0.15.  The cameras are read through wave-uniform addresses, not staged: there is no chunk size.
 *
 * gcp_filter3d_apply: log_scale f32[n_gauss,3] (v), opacity_logit f32[n_gauss] (x), filter f32[n_gauss] (phi) ->
 * log_scale_out f32[n_gauss,3] (v'), opacity_out f32[n_gauss] (x').  With r_j = phi^2 e^(-2 v_j):
 *   v'_j = v_j + 1/2 log1p(r_j)                      (s'^2 = s^2 + phi^2)
 *   log c = -1/2 sum_j log1p(r_j)                    (c = sqrt(prod s^2 / prod s'^2) in (0, 1])
 *   x' = x + log c - log1p(e^x (1 - c))              (sigmoid(x') = sigmoid(x) c),  1 - c = -expm1(log c)
 * in float32.  A row with phi == 0 is copied bit for bit.  Finite for v in [-30, 10], phi in {0} u [1e-6, 1e2], x in
 * [-20, 20].  The outputs must not alias the inputs.  36 bytes per row.
 *
 * gcp_filter3d_apply_backward: the same three inputs and g_log_scale_out f32[n_gauss,3], g_opacity_out f32[n_gauss] (the
 * loss's gradients with respect to v', x') -> g_log_scale f32[n_gauss,3], g_opacity f32[n_gauss]; every row is written,
 * every intermediate is recomputed.  With u = e^x (1 - c):
 *   g_x = g_x' / (1 + u),   g_logc = g_x' (1 + e^x) / (1 + u),   g_v_j = g_v'_j / (1 + r_j) + g_logc (r_j / (1 + r_j)).
 * phi carries no gradient.  A row with phi == 0 passes the gradients through bit for bit.  52 bytes per row. */
int gcp_filter3d_rate(const float* mean, const float* P, const float* K, const int32_t* wh, int64_t n_gauss, int64_t n_cams,
                      float near_z, float margin, float* rate, void* stream);
int gcp_filter3d_apply(const float* log_scale, const float* opacity_logit, const float* filter, int64_t n_gauss,
                       float* log_scale_out, float* opacity_out, void* stream);
int gcp_filter3d_apply_backward(const float* log_scale, const float* opacity_logit, const float* filter,
                                const float* g_log_scale_out, const float* g_opacity_out, int64_t n_gauss, float* g_log_scale,
                                float* g_opacity, void* stream);

/* ---- lens distortion: photographs resampled into ideal pinhole cameras (csrc/gcp_undistort.hip) ------------------------
 * What `colmap image_undistorter` does before training, on the device and for a whole batch in one launch: image b of
 * `images`, taken through lens b, is resampled into the pinhole camera lens b names as its output, at the SAME size.
 *
 * lenses: f32[images][GCP_LENS_WORDS] on the device, one record per image:
 *   word 0..3    fx, fy, cx, cy     the source photograph's intrinsics, in pixels; pixel centres at + 0.5
 *   word 4..7    fx', fy', cx', cy' the output pinhole camera's
 *   word 8..13   k1..k6             radial coefficients
 *   word 14..15  p1, p2             tangential coefficients
 *   word 16      kind               GCP_LENS_PINHOLE, GCP_LENS_POLYNOMIAL or GCP_LENS_FISHEYE as a float; any other value
 *                                   is read as GCP_LENS_PINHOLE
 *   word 17..19  not read
 * With (x, y) normalised ideal coordinates and r^2 = x^2 + y^2:
 *   GCP_LENS_POLYNOMIAL  radial = (1 + k1 r^2 + k2 r^4 + k3 r^6) / (1 + k4 r^2 + k5 r^4 + k6 r^6),
 *                        x_d = x radial + 2 p1 x y + p2 (r^2 + 2 x^2),  y_d = y radial + 2 p2 x y + p1 (r^2 + 2 y^2)
 *                        (COLMAP's SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV; OpenCV's rational model)
 *   GCP_LENS_FISHEYE     theta = atan r, theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),
 *                        (x_d, y_d) = (x, y) theta_d / r, and (x, y) itself at r = 0; k5, k6, p1, p2 are not read
 *                        (COLMAP's OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE)
 *   GCP_LENS_PINHOLE     (x_d, y_d) = (x, y)
 * Output pixel (i, j) of image b, in float32 with the precise atanf, sqrtf and divisions:
 *   x = (i + 0.5 - cx') / fx', y = (j + 0.5 - cy') / fy';  (u, v) = (fx x_d + cx, fy y_d + cy), clamped to
 *   [0.5, width - 0.5] x [0.5, height - 0.5] (the source's edge is replicated; a NaN lands on the edge too);
 *   dst[b][c][j][i] = the bilinear interpolation of channel c at (u - 0.5, v - 0.5) between the four pixels around it.
 * gcp_undistort_u8:  src u8[images][height][width][3], the layout a JPEG decodes to; the result is divided by 255.
 * gcp_undistort_f32: src f32[images][3][height][width].
 * dst f32[images][3][height][width], every word written; it must not overlap src.
 *
 * One thread per output pixel in blocks of 64 x 4, the image in the grid's z dimension: at most 65535 images per grid, past
 * which a block walks on by that stride, so `images` is bounded only by what can be indexed.  The record is read through
 * wave-uniform addresses.  No atomics, no texture objects, no workspace, no device->host read; a pixel depends on its own
 * coordinates and its image's record only: the same bits whatever the batch, its order or the launch shape.
 * GCP_ERR_INVALID_ARGUMENT before any HIP call: images < 0, height or width < 1, height * width > INT32_MAX, height >
 * 4 * 65535 (the grid's y dimension), images * 12 * height * width > INT64_MAX, and with images > 0 a NULL src, lenses or
 * dst.  images == 0 is a no-op that launches nothing. */
#define GCP_LENS_WORDS 20
#define GCP_LENS_PINHOLE 0
#define GCP_LENS_POLYNOMIAL 1
#define GCP_LENS_FISHEYE 2
int gcp_undistort_u8(const uint8_t* src, const float* lenses, int64_t images, int32_t height, int32_t width, float* dst,
                     void* stream);
int gcp_undistort_f32(const float* src, const float* lenses, int64_t images, int32_t height, int32_t width, float* dst,
                      void* stream);

/* ---- normals: per-Gaussian normals and 2DGS's depth-normal consistency loss (csrc/gcp_normal.hip) -----------------------
 * gcp_normals_forward: for list entry j of one camera, i = index[j] (int64, no repeats; an entry outside [0, n_gauss) gets a
 *   zero normal and no gradient):  q^ = variance_q[i] / max(|q|, 1e-8) (xyzw, the projection's normalisation),
 *   k = argmin_a variance_scale[i][a] (the raw log scale; ties to the lowest a),  n_w = column k of R(q^),
 *   n_c = P[:, :3] n_w,  t_c = P[:, :3] mean[i] + P[:, 3]  (P f32[3][4] world->camera, its left block a rotation),
 *   normal[j] = n_c if n_c . t_c <= 0, else -n_c: the normal faces the camera.  aux[j] = k | (4 if negated), for the backward.
 * gcp_normals_backward: g_normal f32[n_list][3] -> g_q f32[n_gauss][4], through the column of R and the normalisation
 *   (the axis choice and the flip are piecewise constant: variance_scale and mean get no gradient).  Every row is written:
 *   the rows absent from the list are exact zeros (one memset node, then the kernel).
 * One thread per list entry, no grid cap, no atomics, no device->host read (capturable); the same bits whatever the launch
 * shape.  n_list may equal n_gauss (capture-safe lists, which keep the culled entries).  n_list == 0 is a no-op for the
 * forward; the backward still clears g_q.  GCP_ERR_INVALID_ARGUMENT: a negative count, one above INT32_MAX, a NULL pointer.
 *
 * gcp_normal_consistency_forward / _backward: depth D, alpha A f32[images][height][width], normal N f32[images][3][height][width],
 * K f32[images][3][3] ON THE DEVICE.  Per image and pixel p = (x, y):
 *   valid(p) = A(p) >= alpha_min and D(p) > 0;   z = D / A;   r(p) = ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1);   pt = z r;
 *   defined(p): p and (x +- 1, y), (x, y +- 1) are inside the frame and valid;
 *   c = (pt(x, y+1) - pt(x, y-1)) x (pt(x+1, y) - pt(x-1, y)),  n~ = c / |c|  (a fronto-parallel surface: (0, 0, -1));
 *   |c| > 0 where defined, since c . r = -(z(x+1,y) + z(x-1,y)) (z(x,y+1) + z(x,y-1)) / (fx fy);
 *   e(p) = 1 - a(p) N(p) . n~(p) where defined, a = A(p) held constant;  e(p) = 1 elsewhere.
 * forward: partial f32[gcp_normal_consistency_blocks(images, height, width)] receives one sum of e per 32 x 16 tile, image
 *   by image, tiles row-major — the caller adds them (in float64, in a fixed order) and divides by images * height * width;
 *   e_map f32[images][height][width] and depth_normal f32[images][3][height][width] (n~, 0 where not defined): NULL = not written.
 * backward: scale f32[1] on the device = dLoss / d(sum of e);  g_normal = -scale a n~ where defined;  g_depth, g_alpha through
 *   z of the four neighbours (none through the factor a), gathered per pixel from the up to four defined stencils that contain
 *   it; every word of the three outputs is written (0 where nothing reaches it).  Nothing is saved by the forward.
 * One launch per direction, no atomics, no workspace, no device->host read; an image's numbers depend on that image alone.
 * GCP_ERR_INVALID_ARGUMENT before any HIP call: images < 0, height or width < 1, height * width > INT32_MAX, alpha_min not
 * > 0, more than INT32_MAX tiles, a NULL required pointer.  images == 0 is a no-op. */
int gcp_normals_forward(const float* variance_q, const float* variance_scale, const float* mean, const float* P, const int64_t* index,
                        int64_t n_gauss, int64_t n_list, float* normal, uint8_t* aux, void* stream);
int gcp_normals_backward(const float* variance_q, const float* P, const int64_t* index, const uint8_t* aux, const float* g_normal,
                         int64_t n_gauss, int64_t n_list, float* g_q, void* stream);
int64_t gcp_normal_consistency_blocks(int64_t images, int32_t height, int32_t width);
int gcp_normal_consistency_forward(const float* depth, const float* alpha, const float* normal, const float* K, int64_t images,
                                   int32_t height, int32_t width, float alpha_min, float* e_map, float* depth_normal, float* partial,
                                   void* stream);
int gcp_normal_consistency_backward(const float* depth, const float* alpha, const float* normal, const float* K, int64_t images,
                                    int32_t height, int32_t width, float alpha_min, const float* scale, float* g_depth, float* g_alpha,
                                    float* g_normal, void* stream);

/* ---- mesh extraction: TSDF fusion of depth maps, marching tetrahedra (csrc/gcp_tsdf.hip) --------------------------------
 * The volume: nz x ny x nx lattice points, x fastest; point (i, j, k) sits at origin + voxel (i, j, k) in world coordinates.
 * State, float32 planes of that layout on the device: tsdf, weight, and optionally rgb f32[3][nz][ny][nx].  A fresh volume has
 * tsdf = 1, weight = 0, rgb = 0 (the caller fills them).
 *
 * gcp_tsdf_integrate: one launch integrates `cameras` cameras.  depth, alpha f32[cameras][height][width] as the blend paints
 * them (depth NOT divided by alpha), image f32[cameras][3][height][width] (read only with rgb), P f32[cameras][3][4]
 * world->camera, K f32[cameras][3][3], all ON THE DEVICE.  For a lattice point x_w, for c = 0 .. cameras - 1 in that order:
 *   p = R_c x_w + t_c;  z = p.z;                          skip unless z > 0
 *   u = fx p.x / z + cx;  v = fy p.y / z + cy             (pixel centres at +0.5 in K's coordinates)
 *   skip unless 0 <= u < width and 0 <= v < height        (compared in float before any conversion);  x = floor u, y = floor v
 *   a = alpha[c][y][x], D = depth[c][y][x];               skip unless a >= alpha_min and D > 0   (a NaN skips)
 *   d = D / a;                                            skip if depth_max > 0 and d > depth_max
 *   s = d - z;                                            skip if s < -trunc
 *   tau = min(1, s / trunc);  tsdf <- (tsdf w + tau) / (w + 1);  rgb likewise with image[c][:][y][x];  w <- w + 1
 * Open3D's projective z-depth TSDF with nearest-pixel lookup and unit weights.  One thread per lattice point, the state in
 * registers over the camera loop, float32 throughout: cameras 0 .. B-1 in one launch, one at a time or in any split give the
 * same bits.  No atomics, no workspace, no device->host read (capturable).
 * GCP_ERR_INVALID_ARGUMENT before any HIP call: a dimension < 2, nx ny nz >= 2^31, voxel or trunc not > 0 or not finite, a
 * non-finite origin, cameras < 0, and with cameras > 0: height or width < 1, height * width > INT32_MAX, a NULL tsdf, weight,
 * depth, alpha, P or K, rgb without image.  cameras == 0 is a no-op.
 *
 * gcp_mesh_count / gcp_mesh_write: the level set tsdf = iso as an indexed triangle mesh, by marching tetrahedra.  A cell is the
 * cube between (i, j, k) and (i+1, j+1, k+1); it is VALID when all 8 corners have weight > 0 (weight NULL: every cell).  A
 * cell is cut into the 6 Kuhn tetrahedra {c, c + e_a, c + e_a + e_b, c + (1,1,1)}, (a, b) = (x,y) (x,z) (y,x) (y,z) (z,x) (z,y)
 * in that order.  A corner is inside when f < iso.  Vertices live on lattice edges of 7 kinds from their lower end point, which
 * owns them: +x, +y, +z, +xy, +xz, +yz, +xyz.  An edge carries one vertex when its end points differ in side, both lie in the
 * grid and at least one valid cell contains it: at x_p + t (x_q - x_p), t = (iso - f_p) / (f_q - f_p), p the owner; colours are
 * interpolated the same way.  A tetrahedron with 1 or 3 inside corners gives 1 triangle, with 2 gives 2 (the quadrilateral
 * (a o0, a o1, b o1, b o0) split along its first and third vertex; a, b inside, o0, o1 outside, in corner order); counter-
 * clockwise seen from where f grows.  Zero-area triangles (t rounded to 0 or 1) are kept.  Vertices are ordered by (owner, kind),
 * faces by (cell, tetrahedron, triangle): the same bits on every run.  No unreferenced and no duplicated vertex.
 *   gcp_mesh_count fills ws (gcp_mesh_workspace_bytes(nx, ny, nz) bytes, 256-byte aligned) and writes the number of vertices
 *     and of faces to totals_host[0..1] — it synchronises the stream once for that read: NOT capturable.
 *     GCP_ERR_INVALID_ARGUMENT as well when 3 V or 3 F does not fit int32.
 *   gcp_mesh_write takes the same tsdf, dimensions, iso and the ws gcp_mesh_count filled, and writes vertices f32[V][3],
 *     faces int32[F][3] and, with rgb and colours given, colours f32[V][3].  V = 0 and F = 0 launch nothing.
 * GCP_ERR_INVALID_ARGUMENT before any HIP call: a dimension < 2, nx ny nz >= 2^31, voxel not > 0, a NaN iso, a NULL tsdf, ws or
 * totals_host, negative totals, NULL outputs with work to do, colours without rgb; GCP_ERR_WORKSPACE: ws too small or
 * misaligned.  gcp_mesh_workspace_bytes returns 0 for refused dimensions. */
int gcp_tsdf_integrate(float* tsdf, float* weight, float* rgb, int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y,
                       float origin_z, float voxel, float trunc, const float* depth, const float* alpha, const float* image,
                       const float* P, const float* K, int64_t cameras, int32_t height, int32_t width, float alpha_min,
                       float depth_max, void* stream);
size_t gcp_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int gcp_mesh_count(const float* tsdf, const float* weight, int32_t nx, int32_t ny, int32_t nz, float iso, void* ws, size_t ws_bytes,
                   int64_t* totals_host, void* stream);
int gcp_mesh_write(const float* tsdf, const float* rgb, int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z,
                   float voxel, float iso, const void* ws, size_t ws_bytes, int64_t n_vertices, int64_t n_faces, float* vertices,
                   int32_t* faces, float* colours, void* stream);

/* ---- mesh cleaning and vertex normals (csrc/gcp_meshclean.hip): what 2DGS, GOF, RaDe-GS and PGSR do through Open3D's
 * post_process_mesh after the fusion ----------------------------------------------------------------------------------------
 * The mesh: faces int32[F][3] over V vertices, ANY indexed triangle list (unreferenced vertices, repeated faces, faces that name
 * a vertex twice, ids in any order); 3 V and 3 F fit int32.  A face with an index outside [0, V) is never addressed through: every
 * kernel tests the three indices first and skips the whole face.  Integer work, or float32 in a pinned order: every output is a
 * function of the mesh alone, the same bits on every run.  No float atomic, no inter-block wait.
 *
 * gcp_mesh_components: two vertices belong together when a face names both — the shared-VERTEX rule.  (Open3D's
 * cluster_connected_triangles joins triangles over a shared EDGE; the two differ only where shells touch in a single vertex,
 * which the extraction above cannot produce: its output is a combinatorial manifold.)
 *   label int32[V]   the SMALLEST vertex index of the vertex's component
 *   size  int32[V]   at a component's label: the number of its faces (a face belongs to the component of its first vertex, which
 *                    is that of all three); 0 in every other row
 * Four launches: init; hook, one thread per face — a union-find in `label`, the larger root always hooked under the smaller with a
 * compare-and-swap, root walks with path halving, no other loop and no wait; flatten, one thread per vertex; count, one thread
 * per face, integer atomics aggregated per wave (it needs the final labels).  F = 0: the init alone.  V = 0: nothing.
 * Faces with an index outside [0, V) are IGNORED here and reported: status_dev (device int32, may be NULL) receives 1 if there
 * was one, else 0.  ws: gcp_mesh_components_workspace_bytes(V, F) bytes, 256-byte aligned.  No device->host read: capturable.
 *
 * gcp_mesh_select / gcp_mesh_compact: 2DGS's rule.  keep_largest = k >= 1, min_faces = m >= 1; c_k = the k-th largest component
 * face count, or the smallest count if there are fewer than k components; T = max(c_k, m); a component is kept iff its count
 * >= T.  Ties at the threshold are all kept: no tie-break, a function of the mesh alone.  A face is kept with its component, a
 * vertex iff a kept face names it — unreferenced vertices go.  T is found on the device (gcp_sort_pairs_u32 of `size`).
 *   gcp_mesh_select runs the components, the sort, the keep flags and two gcp_exclusive_scan_i32 into ws
 *     (gcp_mesh_clean_workspace_bytes(V, F) bytes, 256-byte aligned) and writes the kept counts V', F' to totals_host[0..1] — ONE
 *     host read of (status, V', F'), for which it synchronises the stream: NOT capturable.  GCP_ERR_INVALID_ARGUMENT from that
 *     read when a face index lies outside [0, V).  V = 0 or F = 0: nothing is kept, nothing is launched, totals 0.
 *   gcp_mesh_compact takes the same faces, V, F and the ws gcp_mesh_select filled, with V', F' as returned, and writes
 *     vertices_out f32[V'][3], faces_out int32[F'][3] with renumbered indices and, where given, colours_out / normals_out
 *     f32[V'][3] from colours / normals f32[V][3].  Vertices and faces keep their input order (by (owner, kind) and by (cell,
 *     tetrahedron, triangle) for the extraction's); kept rows are bit copies; with everything kept the outputs are the inputs bit
 *     for bit.  Outputs must not overlap inputs.  V' = F' = 0 launches nothing.
 *
 * gcp_mesh_vertex_normals: Open3D's compute_vertex_normals.  n_v = normalise(sum over the corners (f, j) that name v of
 * (b - a) x (c - a), (a, b, c) the vertices of f) — un-normalised cross products, hence area-weighted; zero-area faces add
 * nothing; a face counts once per corner that names v.  A zero or non-finite sum gives (0, 0, 0), never a NaN.  The extraction's
 * faces are counter-clockwise seen from where the field grows, so these normals point OUT of the surface, towards the cameras.
 * The order is pinned without atomics: the 3 F corners are stably sorted by vertex id (gcp_sort_pairs_u32, key_bits =
 * bit length of V, at most 30: the corners of a face with a bad index carry the key V and are left out), run starts come from the
 * sorted keys, one thread per vertex adds its faces in ascending corner index 3 f + j in float32, each cross product recomputed
 * from the three positions (nothing fused), the sum scaled by a power of two before |.| so that no square overflows or vanishes.
 * Every word of normals f32[V][3] is written.  ws: gcp_mesh_vertex_normals_workspace_bytes(V, F), 256-byte aligned.  No host
 * read: capturable.
 *
 * GCP_ERR_INVALID_ARGUMENT before any HIP call: V or F negative, 3 V or 3 F past int32, k < 1 or m < 1, a NULL totals_host, a
 * NULL pointer with work to do, V' > V or F' > F or negative, colours_out without colours, normals_out without normals.
 * GCP_ERR_WORKSPACE: ws too small or misaligned.  The _workspace_bytes functions return 0 for refused sizes. */
size_t gcp_mesh_components_workspace_bytes(int64_t n_vertices, int64_t n_faces);
int gcp_mesh_components(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* label, int32_t* size, int32_t* status_dev,
                        void* ws, size_t ws_bytes, void* stream);
size_t gcp_mesh_clean_workspace_bytes(int64_t n_vertices, int64_t n_faces);
int gcp_mesh_select(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int64_t keep_largest, int64_t min_faces, void* ws,
                    size_t ws_bytes, int64_t* totals_host, void* stream);
int gcp_mesh_compact(const int32_t* faces, int64_t n_faces, int64_t n_vertices, const float* vertices, const float* colours,
                     const float* normals, const void* ws, size_t ws_bytes, int64_t n_vertices_out, int64_t n_faces_out, float* vertices_out,
                     int32_t* faces_out, float* colours_out, float* normals_out, void* stream);
size_t gcp_mesh_vertex_normals_workspace_bytes(int64_t n_vertices, int64_t n_faces);
int gcp_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float* normals, void* ws,
                            size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Exact k nearest neighbours inside one cloud (gcp_knn.hip): what the initial scale of every Gaussian is made of (upstream
 * 3DGS: simple-knn's distCUDA2; the reference: uitility.py:68-78 `kyori2`, torch.cdist + topk in batches).
 *
 * The definition.  xyz f32[n][3], FINITE coordinates (a precondition: with a NaN or an infinity the call still ends and
 * still writes every word, but what it writes is not defined).  For points i != j
 *     d2(i, j) = (dx * dx + dy * dy) + dz * dz,   dx = x_i - x_j ...   in float32, in that association, nothing fused
 * — direct differences, not |a|^2 + |b|^2 - 2 a.b, so a cloud far from its origin loses nothing.  Row i of the outputs lists
 * the k smallest pairs (d2(i, j), j) over all j != i, ascending, lexicographic: among equal distances the lower index comes
 * first.  "Other" is by INDEX: a duplicate of point i at distance 0 is a neighbour, point i itself is not.
 *     index int32[n][k]   j, in the caller's numbering
 *     dist2 f32[n][k]     d2(i, j)
 * A row with fewer than k other points (n <= k) is padded with index = -1, dist2 = +inf.  Every word of both outputs is
 * written.  1 <= k <= 16, n < 2^31 - 1.
 * The result is a function of xyz and k alone — the same bits whatever the spatial order of the points, the stream or the
 * workspace's earlier contents; exact, not approximate (Morton order + two levels of exact boxes; pruning only on a float32
 * bound that is strictly greater than the current k-th best).  No atomics, no allocation, no device->host read: capturable.
 * ws: gcp_knn_workspace_bytes(n) bytes, any alignment.
 * GCP_ERR_INVALID_ARGUMENT before any HIP call: n < 0 or too large, k outside 1..16, and with n > 0 a NULL xyz, index, dist2
 * or ws; GCP_ERR_WORKSPACE: ws too small.  n == 0 is a no-op. */
size_t gcp_knn_workspace_bytes(int64_t n);
int gcp_knn(const float* xyz, int64_t n, int32_t k, int32_t* index, float* dist2, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GROUPED_CUMPROD_HIP_H */
