"""Depth of the backward's raw look-back, chunk by chunk.

Wave 0 of a tile whose first element (scan order: the backward runs from the end of the array) continues a group takes
the group's part behind the tile from the raw inputs: chunk 0 (256 elements) comes with the tile's own loads, chunks
1 .. 15 in batches of three per dependent round trip (five in the other scans), and a group that fills all sixteen is
handed over to the descriptor tree.  Here the group entering a tile starts 1 .. 4096 elements behind the tile boundary:
every count of chunks on both sides of the batch boundaries (1 | 2-4 | 5-7 | 8-10 | ...), and the hand-over.  The tile's
wave 0 holds a head (the group ends 300 elements into the tile), so the raw search is not abandoned for the tree.

Checked as in test_bwd_persistent_gpu.py: BIT FOR BIT between the `inv_len` path and a run where every wave falls back
to the runs of `inv` (a dummy one-entry `inv_len`), for both alignments and every descriptor wait, and within the suite's
1e-5 * (1 + condition scale) of the C oracle."""
import functools

import pytest
import torch

from tests.util import TOL, assert_parity, make_values

pytestmark = pytest.mark.gpu

TILE = 4096
DEPTHS = [1, 255, 256, 257, 768, 769, 1024, 1792, 1793, 4095, 4096]
INSIDE = 300     # elements of the entering group inside the tile: a head in wave 0's 1024 (scan order)
PARTIAL = 1234


def _mods():
    import grouped_cumprod as gc
    from oracle import c_oracle as co

    return gc, co


@functools.lru_cache(maxsize=1)
def _host():
    """One list for all depths: depth i owns tiles 3 i + 1 (the tile under test) and 3 i + 2 (what lies behind it in scan
    order); the group is [boundary - INSIDE, boundary + depth) with boundary = the start of tile 3 i + 2.  Everything
    else is short groups (1 .. 160 elements).  Returns x, grad_out, key (= inv), inv_len, and the groups' bounds."""
    _, co = _mods()
    n = (3 * len(DEPTHS) + 2) * TILE + PARTIAL
    g = torch.Generator().manual_seed(11)
    spans = [((3 * i + 2) * TILE - INSIDE, (3 * i + 2) * TILE + d) for i, d in enumerate(DEPTHS)]
    lens, pos = [], 0
    for lo, hi in spans + [(n, n)]:
        while pos < lo:  # short groups up to the next long one
            step = min(int(torch.randint(1, 161, (1,), generator=g)), lo - pos)
            lens.append(step)
            pos += step
        if hi > lo:
            lens.append(hi - lo)
            pos = hi
    lens = torch.tensor(lens)
    assert int(lens.sum()) == n
    key = torch.repeat_interleave(torch.arange(lens.numel(), dtype=torch.int32), lens)
    inv, inv_len = co.groups_from_key(key)
    assert torch.equal(inv, key)
    for (lo, hi), d in zip(spans, DEPTHS):  # the group is what the docstring says it is
        gid = int(inv[lo])
        assert int(inv_len[gid]) == hi and (gid == 0 or int(inv_len[gid - 1]) == lo) and hi - (lo + INSIDE) == d
    x = make_values(n, 5, "near1")
    go = make_values(n, 8, "normal")
    return x, go, inv, inv_len, spans


def _put(t, device, offset):  # offset 1: a view that is not 16-byte aligned
    buf = torch.zeros(t.numel() + offset, dtype=t.dtype, device=device)
    buf[offset:] = t.to(device)
    return buf[offset:]


@pytest.mark.parametrize("offset", [0, 1])
def test_every_chunk_count_matches_the_runs_bitwise_and_the_oracle(device, offset):
    gc, co = _mods()
    x, go, inv, inv_len, spans = _host()
    xd, god, invd = (_put(t, device, offset) for t in (x, go, inv))
    ild = inv_len.to(device)
    dummy = torch.zeros(1, dtype=torch.int32, device=device)
    y = torch.empty_like(xd)
    gc.grouped_cumprod_forward(xd, invd, y)
    try:
        ref = None
        for wait in (200, 0, -1):
            gc.set_lookback_wait_us(wait)
            fast = torch.full_like(xd, float("nan"))
            gc.grouped_cumprod_backward(xd, y, god, invd, fast, ild)
            # depth 4096 fills the window: that tile, and no other, takes its carry from the tree or the follow-up kernel
            handed_over = gc.last_lookback_tiles(device) + gc.last_fallback_tiles(device)
            runs = torch.full_like(xd, float("nan"))
            gc.grouped_cumprod_backward(xd, y, god, invd, runs, dummy)
            torch.cuda.synchronize()
            assert not torch.isnan(fast).any()
            assert handed_over == 1, (offset, wait, handed_over)
            for (lo, hi), d in zip(spans, DEPTHS):  # per depth first: a failure names the chunk count
                assert torch.equal(fast[lo:hi], runs[lo:hi]), (d, offset, wait, int((fast[lo:hi] != runs[lo:hi]).sum()))
            assert torch.equal(fast, runs), (offset, wait, int((fast != runs).sum()))
            if ref is None:
                ref = fast
            assert torch.equal(fast, ref), (offset, wait, int((fast != ref).sum()))
    finally:
        gc.set_lookback_wait_us(200)
    yc = y.cpu()  # the API takes the cumprod as an operand: the oracle gets the one the kernel got
    want = co.cumprod_backward_f64(x, yc, go, inv).float()
    assert_parity(ref, want, co.cumprod_backward_f64(x, yc, go.abs(), inv), f"backward look-back depths, offset {offset}", tol=TOL)
