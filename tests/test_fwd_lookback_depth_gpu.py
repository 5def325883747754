"""Depth of the forward scans' raw look-back, chunk by chunk: the forward counterpart of test_bwd_lookback_depth_gpu.py.

Wave 0 of a tile whose first element (scan order) continues a group takes the group's part behind the tile from the raw
inputs: chunk 0 (256 elements) comes with the tile's own loads, chunks 1 .. 15 in batches per dependent round trip (five
chunks in the forward scans and the reverse sum, three in the cumprod backward), and a group that fills all sixteen is
handed over to the descriptor tree.  Here the group entering a tile starts 1 .. 4096 elements behind the tile boundary:
every count of chunks on both sides of the batch edges for a batch of three (1 | 2-4 | 5-7 | 8-10 | 11-13 | 14-16) AND
of five (1 | 2-6 | 7-11 | 12-16), so the test does not depend on which constant the build has, and the hand-over.  The
tile's wave 0 holds a head (the group ends 300 elements into the tile), so the raw search is not abandoned for the tree.

For the running product, the running sum and the reverse sum (mirrored layout: it scans from the end of the array), at
16-byte-aligned views and at views offset by one element: BIT FOR BIT the same for every descriptor wait, bit for bit
the indexed scan of the same mode under the identity permutation (same tile routine, same association), exactly one
tile handed over, and within the suite's 1e-5 rule of the C oracle.  One case of the carry form, whose look-back folds
carry[k0] in after the batches."""
import functools

import pytest
import torch

from tests.util import TOL, assert_parity, make_values

pytestmark = pytest.mark.gpu

TILE = 4096
DEPTHS = [1, 255, 256, 257, 1024, 1025, 1536, 1537, 1792, 1793, 2560, 2561, 2816, 2817, 3328, 3329, 4095, 4096]
INSIDE = 300     # elements of the entering group inside the tile: a head in wave 0's 1024 (scan order)
PARTIAL = 1234
N = (3 * len(DEPTHS) + 2) * TILE + PARTIAL


def _mods():
    import grouped_cumprod as gc
    from oracle import c_oracle as co

    return gc, co


@functools.lru_cache(maxsize=2)
def _keys(reverse):
    """One list for all depths, never modified.  Forward: depth i owns tile 3 i + 2 (under test) and 3 i + 1 (what lies
    behind it in scan order); its group is [boundary - depth, boundary + INSIDE), boundary = the start of tile 3 i + 2.
    Reverse: the mirror image, tile 3 i + 1 under test and the group [boundary - INSIDE, boundary + depth) around the
    start of tile 3 i + 2.  Everything else is short groups (1 .. 160 elements).  Returns key (= inv), inv_len, spans."""
    _, co = _mods()
    g = torch.Generator().manual_seed(11)
    bounds = [(3 * i + 2) * TILE for i in range(len(DEPTHS))]
    spans = [(b - INSIDE, b + d) if reverse else (b - d, b + INSIDE) for b, d in zip(bounds, DEPTHS)]
    lens, pos = [], 0
    for lo, hi in spans + [(N, N)]:
        assert lo >= pos
        while pos < lo:  # short groups up to the next long one
            step = min(int(torch.randint(1, 161, (1,), generator=g)), lo - pos)
            lens.append(step)
            pos += step
        if hi > lo:
            lens.append(hi - lo)
            pos = hi
    lens = torch.tensor(lens)
    assert int(lens.sum()) == N
    key = torch.repeat_interleave(torch.arange(lens.numel(), dtype=torch.int32), lens)
    inv, inv_len = co.groups_from_key(key)
    assert torch.equal(inv, key)
    for (lo, hi), d in zip(spans, DEPTHS):  # the group is what the docstring says it is
        gid = int(inv[lo])
        assert int(inv_len[gid]) == hi and (gid == 0 or int(inv_len[gid - 1]) == lo) and hi - lo == d + INSIDE
    return key, inv_len, spans


@functools.lru_cache(maxsize=3)
def _case(mode):
    """(x, key, spans, oracle's fp32 result, condition scale or None) of one mode, computed once"""
    _, co = _mods()
    key, _, spans = _keys(mode == "cumsum_reverse")
    if mode == "cumprod":
        x = make_values(N, 5, "near1")
        return x, key, spans, co.cumprod_forward(x, key), None  # a product of factors in [0, 1]: absolute bound
    x = make_values(N, 8, "normal")
    if mode == "cumsum":
        return x, key, spans, co.cumsum_forward(x, key), co.cumsum_forward_f64(x.abs(), key)
    scale = co.cumsum_forward_f64(x.abs().flip(0).contiguous(), key.flip(0).contiguous()).flip(0)
    return x, key, spans, co.cumsum_reverse(x, key), scale


def _put(t, device, offset):  # offset 1: a view that is not 16-byte aligned
    buf = torch.zeros(t.numel() + offset, dtype=t.dtype, device=device)
    buf[offset:] = t.to(device)
    return buf[offset:]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("mode", ["cumprod", "cumsum", "cumsum_reverse"])
def test_every_chunk_count_is_the_same_bits_for_every_wait_and_matches_the_oracle(device, mode, offset):
    gc, _ = _mods()
    plain = {"cumprod": gc.grouped_cumprod_forward, "cumsum": gc.grouped_cumsum_forward, "cumsum_reverse": gc.grouped_cumsum_reverse}[mode]
    indexed = {"cumprod": gc.grouped_cumprod_forward_indexed, "cumsum": gc.grouped_cumsum_forward_indexed,
               "cumsum_reverse": gc.grouped_cumsum_reverse_indexed}[mode]
    x, key, spans, want, scale = _case(mode)
    xd, kd = _put(x, device, offset), _put(key, device, offset)
    ident = _put(torch.arange(N, dtype=torch.int32), device, offset)
    try:
        ref = None
        for wait in (200, 0, -1):
            gc.set_lookback_wait_us(wait)
            y = torch.full_like(xd, float("nan"))
            plain(xd, kd, y)
            # depth 4096 fills the window: that tile, and no other, takes its carry from the tree or the follow-up kernel
            handed_over = gc.last_lookback_tiles(device) + gc.last_fallback_tiles(device)
            yi = torch.full_like(xd, float("nan"))
            indexed(xd, kd, ident, yi)
            torch.cuda.synchronize()
            assert not torch.isnan(y).any()
            assert handed_over == 1, (mode, offset, wait, handed_over)
            if ref is None:
                ref = y
            for (lo, hi), d in zip(spans, DEPTHS):  # per depth first: a failure names the chunk count
                assert torch.equal(y[lo:hi], ref[lo:hi]), (mode, d, offset, wait, int((y[lo:hi] != ref[lo:hi]).sum()))
                assert torch.equal(y[lo:hi], yi[lo:hi]), (mode, d, offset, wait, int((y[lo:hi] != yi[lo:hi]).sum()))
            assert torch.equal(y, ref), (mode, offset, wait, int((y != ref).sum()))
            assert torch.equal(y, yi), (mode, offset, wait, int((y != yi).sum()))
    finally:
        gc.set_lookback_wait_us(200)
    assert_parity(ref, want, scale, f"{mode} look-back depths, offset {offset}", tol=TOL)


def test_carry_form_folds_the_carry_in_behind_every_chunk_count(device):
    gc, co = _mods()
    x, key, _, _, _ = _case("cumprod")
    _, inv_len, _ = _keys(False)
    carry = 0.25 + 0.75 * torch.rand(inv_len.numel(), generator=torch.Generator().manual_seed(3))
    y = torch.full((N,), float("nan"), device=device)
    gc.grouped_cumprod_forward_carry(x.to(device), key.to(device), carry.to(device), y)
    want = co.cumprod_forward_f64(x, key) * carry.double()[key.long()]
    assert_parity(y, want.float(), want, "cumprod_carry look-back depths", tol=TOL)
