"""Reference for the tile binning (csrc/gcp_bin.hip) and the per-pixel lists (k_pixel_lists, csrc/gcp_walk.hip), and the
table of cases both are checked at.  numpy int64 only; nothing of the library is imported, so the reference cannot
share a mistake with it.  Semantics as csrc/gcp_tiles.hpp and include/grouped_cumprod_hip.h document them:

  * a box is the INCLUSIVE integer rectangle start..end, clipped to [0, W] x [0, H]; empty when x1 < x0 or y1 < y0;
  * tiles are 16 x 16 pixels, tile of a coordinate = coord >> 4, tiles_x = ceil((W + 1) / 16), tile id = ty * tiles_x + tx;
  * tile_off = exclusive prefix sum of the tile counts per Gaussian; tile_list = Gaussian ids per tile, ascending (= depth
    order); tile_start[t] = first entry whose tile id is >= t.

Everything is integer work: every comparison with these functions is exact.
"""
import numpy as np

TILE_LOG2 = 4
TILE = 1 << TILE_LOG2
SORT_CHUNK = 4096      # keys per radix-sort block (kSortChunk)
STAGE = 256            # list entries staged per round by the tile walks (kStage)
EMIT_WIDE = 128        # tile count from which a box is emitted by its whole wave (kEmitWide)
COUNT_GRID = 512 * 256  # Gaussians one sweep of k_tile_count's grid covers; above it the grid-stride loop iterates


def _i64(a):
    return np.asarray(a, dtype=np.int64).reshape(-1, 2)


def clip_boxes(start, end, W, H):
    """-> (x0, y0, x1, y1, live): the boxes clipped to the frame, and which of them are not empty."""
    s, e = _i64(start), _i64(end)
    x0, y0 = np.maximum(s[:, 0], 0), np.maximum(s[:, 1], 0)
    x1, y1 = np.minimum(e[:, 0], W), np.minimum(e[:, 1], H)
    return x0, y0, x1, y1, (x1 >= x0) & (y1 >= y0)


def tile_grid(W, H):
    return (W + 1 + TILE - 1) // TILE, (H + 1 + TILE - 1) // TILE


def sort_passes(n_tiles):
    """8-bit radix passes over the tile id: bits = ceil(log2(n_tiles)) (at least 1), rounded up to an even pass count."""
    bits = 1
    while (1 << bits) < n_tiles:
        bits += 1
    passes = (bits + 7) // 8
    return passes + (passes & 1)


def tile_shapes(start, end, W, H):
    """-> (tx0, ty0, ntx, nty) per Gaussian after clipping; ntx = nty = 0 for an empty box."""
    x0, y0, x1, y1, live = clip_boxes(start, end, W, H)
    tx0, ty0 = x0 >> TILE_LOG2, y0 >> TILE_LOG2
    ntx = np.where(live, (x1 >> TILE_LOG2) - tx0 + 1, 0)
    nty = np.where(live, (y1 >> TILE_LOG2) - ty0 + 1, 0)
    return tx0, ty0, ntx, nty


def _expand(first, width, count):
    """Per entry of the concatenated runs: (owner, row inside the owner's run-rectangle, column)."""
    n = count.shape[0]
    owner = np.repeat(np.arange(n, dtype=np.int64), count)
    i = np.arange(int(count.sum()), dtype=np.int64) - np.repeat(first, count)
    w = np.repeat(width, count)
    return owner, i // w, i % w


def bin_reference(start, end, W, H):
    """-> (tile_off[N+1], tile_start[n_tiles+1], tile_list[K], counts[N], tiles_x, tiles_y), all int64."""
    tiles_x, tiles_y = tile_grid(W, H)
    tx0, ty0, ntx, nty = tile_shapes(start, end, W, H)
    counts = ntx * nty
    tile_off = np.concatenate([np.zeros(1, np.int64), np.cumsum(counts)])
    g, row, col = _expand(tile_off[:-1], ntx, counts)
    tid = (ty0[g] + row) * tiles_x + tx0[g] + col
    order = np.lexsort((g, tid))  # by tile, then by Gaussian id: independent of the order the entries were written in
    tile_start = np.searchsorted(tid[order], np.arange(tiles_x * tiles_y + 1, dtype=np.int64), side="left").astype(np.int64)
    return tile_off, tile_start, g[order], counts, tiles_x, tiles_y


def pixel_lists_reference(start, end, W, H):
    """-> (box_off[N+1], pair_index[M], pair_gauss[M], pair_key[M], pixel_off[(H+1)*(W+1)+1]), all int64: the clipped boxes
    expanded Gaussian-major and row-major inside each box, stably sorted by the pixel key y * 10000 + x."""
    x0, y0, x1, y1, live = clip_boxes(start, end, W, H)
    bw = np.where(live, x1 - x0 + 1, 0)
    bh = np.where(live, y1 - y0 + 1, 0)
    size = bw * bh
    box_off = np.concatenate([np.zeros(1, np.int64), np.cumsum(size)])
    g, row, col = _expand(box_off[:-1], bw, size)
    y, x = y0[g] + row, x0[g] + col
    key = y * 10000 + x
    pair_index = np.argsort(key, kind="stable").astype(np.int64)
    per_pixel = np.bincount(y * (W + 1) + x, minlength=(H + 1) * (W + 1)).astype(np.int64)
    pixel_off = np.concatenate([np.zeros(1, np.int64), np.cumsum(per_pixel)])
    return box_off, pair_index, g[pair_index], key[pair_index], pixel_off


def overflow_capacities(tile_off, counts):
    """Capacities below K for the capture-safe route, by what they cut, from the reference prefix sums (K >= 2):
      below_k   K - 1;
      on_first  tile_off[g] of a non-empty g near N/2 with tile_off[g] >= 1: the bound lies exactly on g's first entry;
      cut       tile_off[g] + 1 of a g with two or more entries: the bound cuts g's box;
      cut_wide  the same for a g that the emit kernel treats as wide;
      nothing   1, when the first non-empty box has more than one entry: nothing can be listed."""
    n = counts.shape[0]
    K = int(tile_off[-1])
    caps = {"below_k": K - 1}
    by_distance = np.argsort(np.abs(np.arange(n) - n // 2), kind="stable")
    for kind, ok in (("on_first", (counts > 0) & (tile_off[:-1] >= 1)), ("cut", counts >= 2), ("cut_wide", counts >= EMIT_WIDE)):
        hit = by_distance[ok[by_distance]]
        if hit.size:
            caps[kind] = int(tile_off[hit[0]]) + (0 if kind == "on_first" else 1)
    first = np.flatnonzero(counts > 0)
    if first.size and counts[first[0]] > 1:
        caps["nothing"] = 1
    return caps


# ------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------
def _i32(start, end, W, H):
    return np.asarray(start, dtype=np.int32).reshape(-1, 2), np.asarray(end, dtype=np.int32).reshape(-1, 2), int(W), int(H)


def _random_boxes(rng, n, W, H, overhang, max_half):
    """Unclipped boxes: centres anywhere up to `overhang` pixels outside the frame, half-sizes 0..max_half per axis."""
    cx = rng.integers(-overhang, W + overhang + 1, n)
    cy = rng.integers(-overhang, H + overhang + 1, n)
    hx = rng.integers(0, max_half + 1, n)
    hy = rng.integers(0, max_half + 1, n)
    return np.stack([cx - hx, cy - hy], 1), np.stack([cx + hx, cy + hy], 1)


FRAME_HAND_ROLES = ("pixel_15", "pixel_16", "pixel_WH", "one_tile", "straddle", "start_negative", "end_beyond", "left",
                    "below", "inverted")


def _frame(W, H, seed):
    def build():
        hand = [((15, 15), (15, 15)), ((16, 16), (16, 16)), ((W, H), (W, H)),  # single pixels
                ((0, 0), (15, 15)),                                            # exactly one tile
                ((14, 13), (17, 16)),                                          # straddles 15|16 both ways
                ((-5, -5), (3, 2)),                                            # start outside
                ((W - 2, H - 1), (W + 40, H + 40)),                            # end outside
                ((-30, 2), (-10, 9)),                                          # wholly to the left
                ((1, H + 5), (9, H + 20)),                                     # wholly below
                ((9, 9), (4, 12))]                                             # inverted in x
        rng = np.random.default_rng(seed)
        rs, re = _random_boxes(rng, 300, W, H, 20, 9)
        start = np.concatenate([np.array([h[0] for h in hand]), rs])
        end = np.concatenate([np.array([h[1] for h in hand]), re])
        return _i32(start, end, W, H)
    return build


def _random_frame(W, H, n, overhang, max_half, seed):
    def build():
        rng = np.random.default_rng(seed)
        s, e = _random_boxes(rng, n, W, H, overhang, max_half)
        return _i32(s, e, W, H)
    return build


def _exact_k(K):
    """N = K + K // 3 + 1 boxes on 271x255, each inside one tile; K of them live at random positions, the rest inverted."""
    def build():
        W, H = 271, 255
        n = K + K // 3 + 1
        rng = np.random.default_rng(1000 + K)
        live = np.zeros(n, dtype=bool)
        live[rng.permutation(n)[:K]] = True
        tx, ty = rng.integers(0, 17, n), rng.integers(0, 16, n)
        a = np.sort(rng.integers(0, TILE, (n, 2)), axis=1)
        b = np.sort(rng.integers(0, TILE, (n, 2)), axis=1)
        start = np.stack([tx * TILE + a[:, 0], ty * TILE + b[:, 0]], 1)
        end = np.stack([tx * TILE + a[:, 1], ty * TILE + b[:, 1]], 1)
        end[~live, 0] = start[~live, 0] - 1 - rng.integers(0, 5, int((~live).sum()))  # inverted: no entry
        return _i32(start, end, W, H)
    return build


# Gaussian -> (ntx, nty) of the box AS GIVEN.  The frame is 128 tiles wide, so the 129-tile row of Gaussian 62 starts one
# tile left of it and is clipped to 128: wide at the threshold only because max(start, 0) was applied.
WIDE_SHAPES = {0: (127, 1), 1: (128, 1), 2: (1, 128), 3: (16, 8), 4: (43, 3), 31: (128, 1), 32: (8, 16), 62: (129, 1),
               63: (1, 127), 64: (11, 12)}
WIDE_N = 229  # one block: three whole waves and 37 lanes


def _wide():
    W = H = 2047
    n_t = 128
    rng = np.random.default_rng(77)
    start = np.zeros((WIDE_N, 2), np.int64)
    end = np.zeros((WIDE_N, 2), np.int64)
    for g in range(WIDE_N):
        if g in WIDE_SHAPES:
            ntx, nty = WIDE_SHAPES[g]
            tx0 = -1 if ntx > n_t else int(rng.integers(0, n_t - ntx + 1))
            ty0 = int(rng.integers(0, n_t - nty + 1))
        elif 128 <= g < 192:  # a whole wave of wide boxes, each one tile further along the diagonal
            ntx, nty = 16, 8
            tx0 = ty0 = g - 128
        else:
            ntx, nty = int(rng.integers(1, 4)), int(rng.integers(1, 4))
            tx0, ty0 = int(rng.integers(0, n_t - ntx + 1)), int(rng.integers(0, n_t - nty + 1))
        start[g] = (tx0 * TILE, ty0 * TILE)
        end[g] = ((tx0 + ntx) * TILE - 1, (ty0 + nty) * TILE - 1)
    start[WIDE_N - 1] = (-500, -500)  # 344 x 76 tiles as given, 128 x 44 inside the frame
    end[WIDE_N - 1] = (5000, 700)
    return _i32(start, end, W, H)


def _all_outside():
    W, H = 30, 17
    rng = np.random.default_rng(5)
    s, e = _random_boxes(rng, 50, W, H, 0, 6)
    side = np.arange(50) % 4
    shift = np.zeros((50, 2), np.int64)
    shift[side == 0, 0] = -(W + 20)   # left of the frame
    shift[side == 1, 0] = W + 20      # right
    shift[side == 2, 1] = -(H + 20)   # above
    shift[side == 3, 1] = H + 20      # below
    return _i32(s + shift, e + shift, W, H)


CASES = {
    "frame_0x0": _frame(0, 0, 11),
    "frame_15": _frame(15, 15, 12),
    "frame_16": _frame(16, 16, 13),
    "frame_30x17": _frame(30, 17, 14),
    "two_digits": _random_frame(271, 255, 3000, 30, 40, 21),
    "tiles_65536": _random_frame(4095, 4095, 5000, 30, 64, 22),
    "tiles_65792": _random_frame(4111, 4095, 5000, 30, 64, 23),
    "tiles_8k": _random_frame(7679, 4319, 6000, 30, 80, 24),
    "k_1": _exact_k(1),
    "k_4095": _exact_k(4095),
    "k_4096": _exact_k(4096),
    "k_4097": _exact_k(4097),
    "k_8192": _exact_k(8192),
    "k_8193": _exact_k(8193),
    "k_135169": _exact_k(135169),
    "wide": _wide,
    "deep_overhang": _random_frame(20, 18, 700, 6, 12, 31),
    "all_outside": _all_outside,
}

EXACT_K = {name: int(name[2:]) for name in CASES if name.startswith("k_")}
FRAME_SIZES = {"frame_0x0": (0, 0), "frame_15": (15, 15), "frame_16": (16, 16), "frame_30x17": (30, 17)}
PIXEL_LIST_CASES = ("frame_15", "frame_16", "frame_30x17", "deep_overhang", "all_outside")
BLEND_CASES = ("frame_30x17", "deep_overhang")

_built = {}


def case(name):
    """The case's inputs and both references, computed once per process and shared read-only."""
    if name not in _built:
        start, end, W, H = CASES[name]()
        for a in (start, end):
            a.setflags(write=False)
        ref = bin_reference(start, end, W, H)
        for a in ref[:4]:
            a.setflags(write=False)
        _built[name] = (start, end, W, H, ref)
    return _built[name]
