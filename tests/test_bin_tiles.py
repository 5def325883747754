"""What tests/test_bin_tiles_gpu.py rests on, checked without a GPU: the numpy reference of tests/bin_tiles_ref.py against
the brute-force definition, and every case of its table against the property it is named for — a case reshaped so that
it no longer reaches the tile, chunk or wave edge it was built for fails here."""
import numpy as np
import pytest
import torch

from tests import bin_tiles_ref as br

SMALL = [name for name in br.CASES if br.case(name)[0].shape[0] <= 3000 and br.case(name)[4][4] * br.case(name)[4][5] <= 300]


def test_the_small_cases_are_the_expected_ones():
    assert set(SMALL) == {"frame_0x0", "frame_15", "frame_16", "frame_30x17", "two_digits", "k_1", "deep_overhang", "all_outside"}


@pytest.mark.parametrize("name", SMALL)
def test_bin_reference_equals_the_definition_per_tile(name):
    start, end, W, H, (tile_off, tile_start, tile_list, counts, tiles_x, tiles_y) = br.case(name)
    assert (tiles_x, tiles_y) == ((W + 1 + 15) // 16, (H + 1 + 15) // 16)
    s, e = start.astype(np.int64), end.astype(np.int64)
    x0, y0 = np.maximum(s[:, 0], 0), np.maximum(s[:, 1], 0)
    x1, y1 = np.minimum(e[:, 0], W), np.minimum(e[:, 1], H)
    live = (x1 >= x0) & (y1 >= y0)
    per_gauss = np.zeros(start.shape[0], dtype=np.int64)
    total = 0
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            # the clipped box and the tile's pixels [16 tx, 16 tx + 15] x [16 ty, 16 ty + 15] share a pixel
            hit = live & (x0 <= 16 * tx + 15) & (x1 >= 16 * tx) & (y0 <= 16 * ty + 15) & (y1 >= 16 * ty)
            want = np.nonzero(hit)[0]  # ascending index = depth order
            t = ty * tiles_x + tx
            assert np.array_equal(tile_list[tile_start[t]:tile_start[t + 1]], want), (tx, ty)
            per_gauss += hit
            total += want.size
    assert tile_start[0] == 0 and tile_start[-1] == total == tile_list.size == tile_off[-1]
    assert np.array_equal(counts, per_gauss)
    assert np.array_equal(tile_off, np.concatenate([[0], np.cumsum(per_gauss)]))


@pytest.mark.parametrize("name", SMALL)
def test_pixel_lists_reference_equals_meshgrid_expansion_and_stable_sort(name):
    start, end, W, H, _ = br.case(name)
    box_off, pair_index, pair_gauss, pair_key, pixel_off = br.pixel_lists_reference(start, end, W, H)
    rect_g, rect_x, rect_y, sizes = [], [], [], []
    for g in range(start.shape[0]):
        lo_x, lo_y = max(int(start[g, 0]), 0), max(int(start[g, 1]), 0)
        xs = torch.arange(lo_x, max(min(int(end[g, 0]), W) + 1, lo_x))  # no pixel when the clipped range is inverted
        ys = torch.arange(lo_y, max(min(int(end[g, 1]), H) + 1, lo_y))
        yy, xx = torch.meshgrid(ys, xs, indexing="ij")  # empty when either range is
        rect_x.append(xx.flatten()); rect_y.append(yy.flatten()); rect_g.append(torch.full((xx.numel(),), g))
        sizes.append(xx.numel())
    rx, ry, rg = torch.cat(rect_x), torch.cat(rect_y), torch.cat(rect_g)
    key = ry * 10000 + rx
    sorted_key, index = torch.sort(key, stable=True)
    assert np.array_equal(box_off, np.concatenate([[0], np.cumsum(sizes)]))
    assert np.array_equal(pair_index, index.numpy())
    assert np.array_equal(pair_gauss, rg[index].numpy())
    assert np.array_equal(pair_key, sorted_key.numpy())
    per_pixel = torch.zeros((H + 1) * (W + 1), dtype=torch.int64).index_add_(0, ry * (W + 1) + rx, torch.ones_like(rx))
    assert np.array_equal(pixel_off, np.concatenate([[0], per_pixel.cumsum(0).numpy()]))


def test_the_table_holds_every_named_case():
    assert set(br.CASES) == {"frame_0x0", "frame_15", "frame_16", "frame_30x17", "two_digits", "tiles_65536", "tiles_65792",
                             "tiles_8k", "k_1", "k_4095", "k_4096", "k_4097", "k_8192", "k_8193", "k_135169", "wide",
                             "deep_overhang", "all_outside"}


@pytest.mark.parametrize("name", list(br.CASES))
def test_case_is_deterministic_int32_and_consistent(name):
    start, end, W, H, (tile_off, tile_start, tile_list, counts, tiles_x, tiles_y) = br.case(name)
    again = br.CASES[name]()
    assert start.dtype == end.dtype == np.int32 and start.shape == end.shape and start.shape[1] == 2
    assert np.array_equal(again[0], start) and np.array_equal(again[1], end) and again[2:] == (W, H)
    n_tiles = tiles_x * tiles_y
    assert tile_off.shape == (start.shape[0] + 1,) and tile_start.shape == (n_tiles + 1,)
    assert tile_list.size == tile_off[-1] == counts.sum() == tile_start[-1] < 2**31
    # ascending ids inside every tile list, every Gaussian as often as it has tiles
    inside = np.ones(tile_list.size, dtype=bool)
    inside[tile_start[:-1][tile_start[:-1] < tile_list.size]] = False
    assert bool((np.diff(tile_list)[inside[1:]] > 0).all())
    assert np.array_equal(np.bincount(tile_list, minlength=counts.size), counts)


@pytest.mark.parametrize("name,frame,n_tiles,passes", [
    ("frame_0x0", (0, 0), 1, 2), ("frame_15", (15, 15), 1, 2), ("frame_16", (16, 16), 4, 2), ("frame_30x17", (30, 17), 4, 2),
    ("two_digits", (271, 255), 17 * 16, 2), ("tiles_65536", (4095, 4095), 65536, 2), ("tiles_65792", (4111, 4095), 257 * 256, 4),
    ("tiles_8k", (7679, 4319), 129600, 4), ("wide", (2047, 2047), 128 * 128, 2), ("deep_overhang", (20, 18), 4, 2),
    ("all_outside", (30, 17), 4, 2)] + [(k, (271, 255), 272, 2) for k in br.EXACT_K])
def test_tile_count_and_pass_count(name, frame, n_tiles, passes):
    _, _, W, H, ref = br.case(name)
    assert (W, H) == frame and ref[4] * ref[5] == n_tiles
    # bin_fill: bits = ceil(log2(n_tiles)), 8 bits per pass, rounded up to an even number of passes
    bits = 1
    while (1 << bits) < n_tiles:
        bits += 1
    want = (bits + 7) // 8
    want += want & 1
    assert want == passes == br.sort_passes(n_tiles)


def test_the_second_digit_and_the_third_are_used():
    for name, first_unused in (("two_digits", 1 << 16), ("tiles_65536", 1 << 16), ("tiles_65792", 1 << 24), ("tiles_8k", 1 << 24)):
        _, _, _, _, (_, tile_start, tile_list, _, tx, ty) = br.case(name)
        listed = np.flatnonzero(np.diff(tile_start))  # ids of the tiles with entries
        assert listed.max() >= 256 and listed.max() < first_unused, name
        assert np.unique(listed >> 8).size > 1, name   # pass 2 sees more than digit 0
    for name, n_boxes in (("two_digits", 3000), ("tiles_65536", 5000), ("tiles_65792", 5000), ("tiles_8k", 6000)):
        assert br.case(name)[0].shape[0] == n_boxes
    listed = np.flatnonzero(np.diff(br.case("tiles_65792")[4][1]))
    assert listed.max() >= 65536                       # an entry whose key has a third digit
    listed = np.flatnonzero(np.diff(br.case("tiles_8k")[4][1]))
    assert listed.max() >= 65536
    assert br.case("tiles_65536")[4][0][-1] > br.SORT_CHUNK  # more than one sort block each
    assert br.case("tiles_8k")[4][0][-1] > br.SORT_CHUNK


@pytest.mark.parametrize("name", list(br.EXACT_K))
def test_exact_entry_counts(name):
    start, end, W, H, (tile_off, _, _, counts, _, _) = br.case(name)
    K = br.EXACT_K[name]
    n = start.shape[0]
    assert n == K + K // 3 + 1 and tile_off[-1] == K
    assert set(np.unique(counts)) <= {0, 1}             # every box inside one tile
    s, e = start.astype(np.int64), end.astype(np.int64)
    dead = counts == 0
    assert bool((e[dead, 0] < s[dead, 0]).all())         # the rest are inverted, not clipped away
    assert bool(((s[~dead] >= 0) & (e[~dead] <= [W, H]) & (s[~dead] >> 4 == e[~dead] >> 4)).all())


def test_exact_entry_counts_sit_on_the_chunk_edges():
    assert sorted(br.EXACT_K.values()) == [1, br.SORT_CHUNK - 1, br.SORT_CHUNK, br.SORT_CHUNK + 1, 2 * br.SORT_CHUNK,
                                           2 * br.SORT_CHUNK + 1, 33 * br.SORT_CHUNK + 1]
    assert br.case("k_135169")[0].shape[0] == 180226 > br.COUNT_GRID   # k_tile_count's grid-stride loop iterates
    assert all(br.case(name)[0].shape[0] < br.COUNT_GRID for name in br.CASES if name != "k_135169")


def test_wide_case():
    start, end, W, H, (tile_off, _, _, counts, tiles_x, tiles_y) = br.case("wide")
    assert (tiles_x, tiles_y) == (128, 128) and start.shape[0] == 229 == 3 * 64 + 37
    s, e = start.astype(np.int64), end.astype(np.int64)
    assert bool((s[:228] % 16 == 0).all() and ((e[:228] + 1) % 16 == 0).all())  # tile-aligned
    given = np.stack([(e[:, 0] + 1 - s[:, 0]) // 16, (e[:, 1] + 1 - s[:, 1]) // 16], 1)  # tile shapes as given
    table = {0: (127, 1), 1: (128, 1), 2: (1, 128), 3: (16, 8), 4: (43, 3), 31: (128, 1), 32: (8, 16), 62: (129, 1), 63: (1, 127),
             64: (11, 12)}
    assert table == br.WIDE_SHAPES
    for g, shape in table.items():
        assert tuple(given[g]) == shape, g
    assert all(tuple(given[g]) == (16, 8) for g in range(128, 192))
    assert np.array_equal(s[128:192], np.stack([np.arange(64) * 16] * 2, 1))   # one tile further each
    _, _, ntx, nty = br.tile_shapes(start, end, W, H)
    # the threshold from both sides: 127, 128 and 129 entries.  Gaussian 62's 129 tiles start one tile outside a frame
    # that is 128 tiles wide: 128 after the clip
    assert [int(counts[g]) for g in (0, 1, 2, 3, 4, 31, 32, 62, 63, 64)] == [127, 128, 128, 128, 129, 128, 128, 128, 127, 132]
    assert s[62, 0] == -16 and (int(ntx[62]), int(nty[62])) == (128, 1)
    assert (int(ntx[1]), int(nty[1])) == (128, 1) and (int(ntx[2]), int(nty[2])) == (1, 128)
    assert int((counts == 127).sum()) == 2
    wide = counts >= br.EMIT_WIDE
    assert int(wide.sum()) == 73
    assert int(wide[:64].sum()) >= 2 and int(wide[64:128].sum()) >= 1   # the ballot loop runs more than once in wave 0
    assert bool(wide[128:192].all())                                    # every lane of wave 2
    assert int(wide[192:].sum()) == 1 and bool(wide[228])               # one in the partial last wave ...
    assert tuple(s[228]) == (-500, -500) and tuple(e[228]) == (5000, 700)
    assert (int(ntx[228]), int(nty[228])) == (128, 44)                  # ... wide only through the clip
    rest = np.ones(229, dtype=bool)
    rest[list(table) + list(range(128, 192)) + [228]] = False
    assert bool(((ntx[rest] >= 1) & (ntx[rest] <= 3) & (nty[rest] >= 1) & (nty[rest] <= 3)).all())
    assert tile_off[-1] > br.SORT_CHUNK                                 # more than one 4096-entry sort block
    # a wide box crosses a sort-block edge
    assert bool(((tile_off[:-1][wide] // br.SORT_CHUNK) != ((tile_off[1:][wide] - 1) // br.SORT_CHUNK)).any())


def test_deep_overhang_case():
    start, end, W, H, (_, tile_start, _, counts, tiles_x, tiles_y) = br.case("deep_overhang")
    assert (W, H, tiles_x * tiles_y, start.shape[0]) == (20, 18, 4, 700)
    lens = np.diff(tile_start)
    # the second staging round of the tile walks (256 entries per round) runs, with remainders of two different lengths,
    # one of them longer than a wave; one list stays within a single round
    over = np.sort(lens[lens > br.STAGE] - br.STAGE)
    assert over.size >= 2 and over[0] >= 1 and over[-1] > over[0] and over[-1] > 64
    assert int(lens.min()) < br.STAGE
    s, e = start.astype(np.int64), end.astype(np.int64)
    live = counts > 0
    assert bool((live & ((s < 0).any(1) | (e > [W, H]).any(1))).any())  # live boxes that overhang the frame
    assert br.pixel_lists_reference(start, end, W, H)[0][-1] > 40000    # tens of thousands of pairs on 399 pixels


def test_all_outside_case():
    start, end, W, H, (tile_off, tile_start, tile_list, counts, _, _) = br.case("all_outside")
    assert (W, H, start.shape[0]) == (30, 17, 50)
    assert tile_off[-1] == 0 and tile_list.size == 0 and not tile_start.any() and not counts.any()
    assert bool((end >= start).all())                                   # none inverted: every one is clipped away
    assert br.pixel_lists_reference(start, end, W, H)[0][-1] == 0
    s, e = start.astype(np.int64), end.astype(np.int64)
    sides = [(e[:, 0] < 0), (s[:, 0] > W), (e[:, 1] < 0), (s[:, 1] > H)]
    assert all(bool(side.any()) for side in sides) and bool(np.logical_or.reduce(sides).all())


@pytest.mark.parametrize("name", list(br.FRAME_SIZES))
def test_frame_cases(name):
    start, end, W, H, (tile_off, _, _, counts, _, _) = br.case(name)
    assert (W, H) == br.FRAME_SIZES[name] and start.shape[0] == len(br.FRAME_HAND_ROLES) + 300
    s, e = start.astype(np.int64), end.astype(np.int64)
    role = {r: i for i, r in enumerate(br.FRAME_HAND_ROLES)}
    for r, xy in (("pixel_15", (15, 15)), ("pixel_16", (16, 16)), ("pixel_WH", (W, H))):
        assert tuple(s[role[r]]) == tuple(e[role[r]]) == xy
        assert counts[role[r]] == (1 if xy[0] <= W and xy[1] <= H else 0)
    assert tuple(s[role["one_tile"]]) == (0, 0) and tuple(e[role["one_tile"]]) == (15, 15) and counts[role["one_tile"]] == 1
    g = role["straddle"]
    assert bool((s[g] <= 15).all() and (e[g] >= 16).all()) and counts[g] == (W >= 14 and H >= 13) * (1 + (W >= 16)) * (1 + (H >= 16))
    assert tuple(s[role["start_negative"]]) == (-5, -5) and counts[role["start_negative"]] == 1
    assert tuple(e[role["end_beyond"]]) == (W + 40, H + 40) and bool((s[role["end_beyond"]] <= [W, H]).all())
    assert counts[role["end_beyond"]] == {"frame_0x0": 1, "frame_15": 1, "frame_16": 4, "frame_30x17": 1}[name]  # 14..16 x 15..16: 4 tiles
    assert e[role["left"], 0] < 0 and e[role["left"], 1] >= s[role["left"], 1] >= 0 and counts[role["left"]] == 0
    assert s[role["below"], 1] > H and e[role["below"], 0] >= s[role["below"], 0] >= 0 and counts[role["below"]] == 0
    assert e[role["inverted"], 0] < s[role["inverted"], 0] and counts[role["inverted"]] == 0
    # among the random ones too: empty, clipped and (by the hand-written one) inverted boxes; nothing was pre-clipped
    rnd = slice(len(br.FRAME_HAND_ROLES), None)
    outside = (s[rnd] < 0).any(1) | (e[rnd] > [W, H]).any(1)
    assert bool((e[rnd] >= s[rnd]).all())
    assert bool((outside & (counts[rnd] == 0)).any()) and bool((outside & (counts[rnd] > 0)).any())
    assert tile_off[-1] >= 2


def test_only_two_cases_have_fewer_than_two_entries():
    assert {name for name in br.CASES if br.case(name)[4][0][-1] < 2} == {"k_1", "all_outside"}


_BASIC = {"below_k", "on_first"}
OVERFLOW_KINDS = {"frame_0x0": _BASIC, "frame_15": _BASIC, "frame_16": _BASIC | {"cut"}, "frame_30x17": _BASIC | {"cut"},
                  "two_digits": _BASIC | {"cut", "nothing"}, "tiles_65536": _BASIC | {"cut", "nothing"},
                  "tiles_65792": _BASIC | {"cut", "nothing"}, "tiles_8k": _BASIC | {"cut", "nothing"},
                  "k_4095": _BASIC, "k_4096": _BASIC, "k_4097": _BASIC, "k_8192": _BASIC, "k_8193": _BASIC, "k_135169": _BASIC,
                  "wide": _BASIC | {"cut", "cut_wide", "nothing"}, "deep_overhang": _BASIC | {"cut", "nothing"}}


@pytest.mark.parametrize("name", list(OVERFLOW_KINDS))
def test_overflow_capacities(name):
    """The capacities of the capture-safe route's overflow checks exist where the case can have them and cut what they say."""
    _, _, _, _, (tile_off, _, _, counts, _, _) = br.case(name)
    K = int(tile_off[-1])
    caps = br.overflow_capacities(tile_off, counts)
    assert set(caps) == OVERFLOW_KINDS[name] and all(1 <= c < K for c in caps.values())
    assert caps["below_k"] == K - 1
    g = np.flatnonzero((tile_off[:-1] == caps["on_first"]) & (counts > 0))
    assert g.size == 1 and abs(int(g[0]) - counts.size // 2) <= counts.size // 4   # exactly on a first entry, near N / 2
    assert ("cut" in caps) == bool((counts >= 2).any())
    assert ("cut_wide" in caps) == bool((counts >= br.EMIT_WIDE).any()) == (name == "wide")
    assert ("nothing" in caps) == bool(counts[np.flatnonzero(counts)[0]] > 1)
    for kind, least in (("cut", 2), ("cut_wide", br.EMIT_WIDE)):
        cap = caps.get(kind, caps["below_k"])           # K - 1 cuts the last non-empty box or lies on its first entry
        g = np.searchsorted(tile_off, cap, side="right") - 1
        assert counts[g] >= (least if kind in caps else 1) and tile_off[g] <= cap < tile_off[g + 1]
        assert kind not in caps or tile_off[g] < cap
