"""The follow-up kernel's workspace maintenance across launches of very different sizes on ONE workspace.

Every multi-tile scan ends with a small launch that counts the introspection flags of the descriptor set just used,
clears the OTHER set over the range its last user wrote, and advances the launch counter.  The
count and the clear are one sweep whose ranges differ whenever the previous launch had another size: here scans of 2, 3,
33, 257, 40 000 and 40 001 tiles (plus a partial one), each on a stretch of data of its own, follow each other
big -> small -> big and small -> big, so that every launch clears what a launch of another size left behind, and
publishes into a set that a launch of another size cleared.
Groups are 5 000 .. 13 000 elements long: longer than the raw look-back window, so results depend on the descriptors.

For all four scans (cumprod forward, cumsum forward, cumprod backward, reverse cumsum): every launch of the sequence
must equal, bit for bit, the same call on a fresh workspace, and report the same `last_lookback_tiles` /
`last_fallback_tiles`; and the same sequence, captured once, must replay inside a HIP graph."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 4096
PARTIAL = 777
BIG = 40001
# tiles -> first element of the case inside the shared operands.  Every size reads its own stretch (the starts are no
# multiple of a tile, so the group layout against the tile grid differs too): a descriptor left behind by a launch of
# another size is a WRONG descriptor in every mode, and the two big cases differ from each other as well.
START = {2: 1236, 3: 2468, 33: 3700, 257: 5000, BIG: 0, BIG - 1: 3000}
ORDERS = {
    "big_small_big": [BIG, 2, BIG - 1, 3, 33, BIG, 257, BIG - 1],
    "small_big": [2, 3, 33, 257, BIG],
}
MODES = ["cumprod_forward", "cumsum_forward", "cumprod_backward", "cumsum_reverse"]


def _gc():
    import grouped_cumprod as gc

    return gc


@pytest.fixture(scope="module")
def operands(device):
    """x, grad_out, inv (dense group ids: also the keys), the groups' ends, and the cumprod of x, for BIG tiles; every
    case is a stretch of them (START)."""
    gc = _gc()
    n = BIG * TILE + PARTIAL
    g = torch.Generator(device=device).manual_seed(3)
    lens = torch.randint(5000, 13000, (n // 5000 + 2,), device=device, generator=g)
    inv = torch.repeat_interleave(torch.arange(lens.numel(), device=device, dtype=torch.int32), lens)[:n].contiguous()
    ends = torch.cumsum(lens, 0).to(torch.int32)
    x = 1.0 - 1e-3 * torch.rand(n, device=device, generator=g)
    go = torch.randn(n, device=device, generator=g)
    y = torch.empty_like(x)
    gc.grouped_cumprod_forward(x, inv, y)
    torch.cuda.synchronize()
    return x, go, inv, ends, y


def _case(operands, ntiles):
    x, go, inv, ends, y = operands
    n, lo = ntiles * TILE + PARTIAL, START[ntiles]
    hi = lo + n
    assert hi <= x.numel()
    first, last = int(inv[lo]), int(inv[hi - 1])
    inv_len = (ends[first:last + 1] - lo).contiguous()  # the ends of the stretch's groups, relative to its start
    inv_len[-1] = n
    inv_s = (inv[lo:hi] - first).contiguous()           # dense ids from 0
    # (y: the backward takes the cumprod as an operand; any values do for a bit-for-bit comparison of two runs)
    return x[lo:hi], go[lo:hi], inv_s, inv_len, y[lo:hi]


def _run(mode, case, out, ws):
    gc = _gc()
    x, go, inv, inv_len, y = case
    if mode == "cumprod_forward":
        gc.grouped_cumprod_forward(x, inv, out, workspace=ws)
    elif mode == "cumsum_forward":
        gc.grouped_cumsum_forward(go, inv, out, workspace=ws)
    elif mode == "cumsum_reverse":
        gc.grouped_cumsum_reverse(go, inv, out, workspace=ws)
    else:
        gc.grouped_cumprod_backward(x, y, go, inv, out, inv_len, workspace=ws)


def _stats(ws):
    """(last_lookback_tiles, last_fallback_tiles) of the workspace's last launch (synchronises)"""
    from simplegaussiansplat_tk71_amd import _lib

    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    vals = []
    for fn in ("gcp_last_lookback_tiles", "gcp_last_fallback_tiles"):
        v = ctypes.c_int64(0)
        assert getattr(lib, fn)(ws.tensor.data_ptr(), stream, ctypes.byref(v)) == 0
        vals.append(v.value)
    return tuple(vals)


def _fresh(mode, operands, device, cache):
    """{ntiles: (output, stats)} of every size on a workspace of its own"""
    gc = _gc()
    for ntiles in sorted(START):
        if (mode, ntiles) not in cache:
            case = _case(operands, ntiles)
            out = torch.full_like(case[0], float("nan"))
            ws = gc.Workspace(device, case[0].numel())
            _run(mode, case, out, ws)
            cache[(mode, ntiles)] = (out, _stats(ws))
            assert not torch.isnan(out).any()
    return cache


@pytest.fixture(scope="module")
def fresh_cache():
    return {}


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("mode", MODES)
def test_sizes_in_turn_on_one_workspace_equal_a_fresh_workspace(device, operands, fresh_cache, mode, order):
    gc = _gc()
    fresh = _fresh(mode, operands, device, fresh_cache)
    ws = gc.Workspace(device, BIG * TILE + PARTIAL)
    walked = 0
    for i, ntiles in enumerate(ORDERS[order]):
        case = _case(operands, ntiles)
        out = torch.full_like(case[0], float("nan"))
        _run(mode, case, out, ws)
        stats = _stats(ws)
        want, want_stats = fresh[(mode, ntiles)]
        assert torch.equal(out, want), (mode, order, i, ntiles, int((out != want).sum()))
        assert stats == want_stats, (mode, order, i, ntiles, stats, want_stats)
        walked += stats[0] + stats[1]
    assert walked > 0, "no tile took its carry from the descriptor tree: the sequence did not exercise it"


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("mode", MODES)
def test_the_sequence_replays_inside_a_captured_graph(device, operands, fresh_cache, mode, order):
    gc = _gc()
    fresh = _fresh(mode, operands, device, fresh_cache)
    seq = ORDERS[order]
    cases = [_case(operands, t) for t in seq]
    outs = [torch.empty_like(c[0]) for c in cases]
    ws = gc.Workspace(device, BIG * TILE + PARTIAL)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(mode, cases[0], outs[0], ws)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for case, out in zip(cases, outs):
            _run(mode, case, out, ws)
    spare = torch.empty_like(cases[1][0])
    for replay in range(2):
        if replay and len(seq) % 2 == 0:  # an even sequence keeps the launch counter's parity: one eager launch flips it
            _run(mode, cases[1], spare, ws)
        for out in outs:
            out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for i, (ntiles, out) in enumerate(zip(seq, outs)):
            want, _ = fresh[(mode, ntiles)]
            assert torch.equal(out, want), (mode, order, replay, i, ntiles, int((out != want).sum()))
