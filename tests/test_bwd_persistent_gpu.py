"""The backward scan over many tiles.  The other backward tests stop at 74 tiles; here 95 to 5000, each with a partial
tile on top: groups that run over many tiles, tiles with and without heads one after the other, waves with more than
255 ends (which fall back to the runs of `inv`), every descriptor-wait setting on the long groups, consecutive launches
on one workspace (descriptor-set parity), replay inside a captured graph, and the end of the array on both sides of
the point where wave 0's look-back chunk changes from two vector loads to guarded ones.

Every case is checked twice: BIT FOR BIT between the `inv_len` path and a run where every wave falls back to the runs of
`inv` (the comparison of test_bwd_group_ends_gpu.py), and within the suite's 1e-5 * (1 + condition scale) of the C oracle."""
import functools

import pytest
import torch

from tests.util import assert_parity, make_keys, make_values

pytestmark = pytest.mark.gpu

TILE = 4096
NTILES = [95, 96, 97, 767, 768, 769, 1553, 5000]
PARTIAL = 1234
DISTS = ["geo80", "mixed", "runs9000", "one_run", "all1"]
LONG = ("mixed", "runs9000", "one_run")  # groups longer than the raw look-back window: the descriptor tree


def _mods():
    import grouped_cumprod as gc
    from oracle import c_oracle as co

    return gc, co


@functools.lru_cache(maxsize=2)
def _host(ntiles, dist):
    """CPU operands of one case (shared by the two alignments): x, grad_out, key, inv, inv_len."""
    _, co = _mods()
    n = ntiles * TILE + PARTIAL
    key = make_keys(n, dist, ntiles + 5)
    inv, inv_len = co.groups_from_key(key)
    x = make_values(n, ntiles, "near1" if dist in LONG else "alpha")
    go = make_values(n, ntiles + 3, "normal")
    return x, go, key, inv, inv_len


def _device_operands(ntiles, dist, device, offset):
    gc, _ = _mods()
    x, go, key, inv, inv_len = _host(ntiles, dist)

    def put(t):  # offset 1: a view that is not 16-byte aligned
        buf = torch.zeros(t.numel() + offset, dtype=t.dtype, device=device)
        buf[offset:] = t.to(device)
        return buf[offset:]

    xd, invd = put(x), put(inv)
    y = torch.empty_like(xd)
    gc.grouped_cumprod_forward(xd, invd, y)
    return xd, y, put(go), put(key), invd, inv_len.to(device)


def _both(xd, y, god, keyd, invd, ild):
    gc, _ = _mods()
    fast = torch.full_like(xd, float("nan"))
    gc.grouped_cumprod_backward(xd, y, god, invd, fast, ild)
    runs = torch.full_like(xd, float("nan"))
    gc.grouped_cumprod_backward(xd, y, god, keyd, runs, torch.zeros(1, dtype=torch.int32, device=xd.device))
    return fast, runs


def _assert_oracle(got, ntiles, dist, y, what):
    _, co = _mods()
    x, go, _, inv, _ = _host(ntiles, dist)
    yc = y.cpu()  # the API takes the cumprod as an operand: the oracle gets the one the kernel got
    want = co.cumprod_backward_f64(x, yc, go, inv).float()
    assert_parity(got, want, co.cumprod_backward_f64(x, yc, go.abs(), inv), what)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("ntiles", NTILES)
def test_many_rounds_match_runs_bitwise_and_the_oracle(device, ntiles, dist, offset):
    gc, _ = _mods()
    ops = _device_operands(ntiles, dist, device, offset)
    waits = (200, 0, -1) if dist in LONG else (200,)
    try:
        ref = None
        for wait in waits:
            gc.set_lookback_wait_us(wait)
            fast, runs = _both(*ops)
            torch.cuda.synchronize()
            assert not torch.isnan(fast).any()
            assert torch.equal(fast, runs), (ntiles, dist, offset, wait, int((fast != runs).sum()))
            if ref is None:
                ref = fast
            assert torch.equal(fast, ref), (ntiles, dist, offset, wait, int((fast != ref).sum()))
    finally:
        gc.set_lookback_wait_us(200)
    _assert_oracle(ref, ntiles, dist, ops[1], f"backward {ntiles} tiles {dist} offset {offset}")


@pytest.mark.parametrize("dist", ["mixed", "one_run", "geo80"])
def test_back_to_back_launches_on_one_workspace(device, dist):
    """Consecutive launches publish into alternate descriptor sets (parity of the workspace's launch counter).  Three
    launches in a row, no synchronisation between them."""
    gc, _ = _mods()
    ntiles = 1553
    xd, y, god, keyd, invd, ild = _device_operands(ntiles, dist, device, 0)
    outs = [torch.full_like(xd, float("nan")) for _ in range(3)]
    for o in outs:
        gc.grouped_cumprod_backward(xd, y, god, invd, o, ild)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    _assert_oracle(outs[0], ntiles, dist, y, f"back to back {dist}")


@pytest.mark.parametrize("dist", ["mixed", "geo80"])
def test_replay_inside_a_captured_graph(device, dist):
    gc, _ = _mods()
    ntiles = 1553
    xd, y, god, keyd, invd, ild = _device_operands(ntiles, dist, device, 0)
    eager = torch.empty_like(xd)
    g = torch.empty_like(xd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gc.grouped_cumprod_backward(xd, y, god, invd, eager, ild)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        gc.grouped_cumprod_backward(xd, y, god, invd, g, ild)
    for _ in range(2):  # an odd and an even launch counter
        g.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g, eager), int((g != eager).sum())
    _assert_oracle(g, ntiles, dist, y, f"graph replay {dist}")


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("dist", ["one_run", "mixed", "geo80"])
@pytest.mark.parametrize("tail", [255, 256, 257])
def test_look_back_chunk_at_the_end_of_the_array(device, tail, dist, offset):
    """Wave 0 of the last full tile looks back into the partial tile behind it: 256 elements as two vector loads when
    the tail holds them all (tail >= 256), guarded loads otherwise.  Operands are views with NaN behind their last
    element: whatever is read there must not reach a result."""
    gc, co = _mods()
    n = 3 * TILE + tail
    key = make_keys(n, dist, tail)
    inv, inv_len = co.groups_from_key(key)
    x = make_values(n, tail, "near1")
    go = make_values(n, tail + 3, "normal")

    def put(t):
        buf = torch.full((offset + n + 512,), float("nan") if t.is_floating_point() else -7, dtype=t.dtype, device=device)
        buf[offset:offset + n] = t.to(device)
        return buf[offset:offset + n]

    xd, god, keyd, invd = put(x), put(go), put(key), put(inv)
    y = put(torch.zeros(n))
    gc.grouped_cumprod_forward(xd, invd, y)
    fast, runs = _both(xd, y, god, keyd, invd, inv_len.to(device))
    torch.cuda.synchronize()
    assert not torch.isnan(fast).any()
    assert torch.equal(fast, runs), (tail, dist, offset, int((fast != runs).sum()))
    yc = y.cpu()
    assert_parity(fast, co.cumprod_backward_f64(x, yc, go, inv).float(), co.cumprod_backward_f64(x, yc, go.abs(), inv),
                  f"backward tail {tail} {dist} offset {offset}")
