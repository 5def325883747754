"""The cumprod backward that rebuilds param_cumprod inside the tile (scan MODE 4, gcp_cumprod_backward) against the one
that streams the given array (MODE 2, gcp_cumprod_backward_given), on the same operands, and both against fp64.

What differs between the two is where the y of a tile's own elements comes from: a segmented product scan of `param` per
1024-element wave range, in ascending address order, continued from one `anchor` float of the given y below the range
when a group enters it from there.  So the cases sit where that can go wrong: heads on, just before and just after the
wave edges (multiples of 1024) and tile edges (multiples of T), groups that straddle them, ranges that take their heads
from `inv` instead of `inv_len`, zeros in `param` next to the edges, the partial last tile, and the dword path.

Tolerance: tests/util.assert_parity's rule, 1e-5 * (1 + scale), scale = the fp64 backward of |grad_out| (the condition
scale of the sum), as in tests/test_scan_gpu.py::test_backward."""
import pytest
import torch

from tests.util import assert_parity, make_keys, make_values

pytestmark = pytest.mark.gpu

WAVE = 1024  # elements of one wave's range
TILE = 4096  # gc.tile_elems(), checked where it is used


def _mods():
    import grouped_cumprod as gc
    from oracle import c_oracle as co

    return gc, co


def _key_from_lens(n, lens):
    """keys whose runs have the given lengths, the last one cut or stretched to n"""
    out, total, i = [], 0, 0
    while total < n:
        ln = lens[i] if i < len(lens) else lens[-1]
        ln = min(ln, n - total)
        out.append(ln)
        total += ln
        i += 1
    ids = torch.arange(len(out))
    vals = ((ids * 7919) % 1000 + (ids % 2) * 1000003).to(torch.int32)  # equal keys recur in non-adjacent runs
    return torch.repeat_interleave(vals, torch.tensor(out))


def _run(device, x, cp, go, inv, inv_len, given, offsets=(0, 0, 0)):
    """one launch; offsets: elements by which param, grad_out and grad_in are moved off a 16-byte boundary"""
    gc, _ = _mods()
    n = x.numel()

    def put(t, off):
        buf = torch.empty(n + 4, dtype=t.dtype, device=device)
        view = buf[off : off + n]
        view.copy_(t)
        assert view.is_contiguous() and (view.data_ptr() % 16 != 0) == (off != 0)
        return view

    out = put(torch.full((n,), float("nan")), offsets[2])
    gc.grouped_cumprod_backward(put(x, offsets[0]), cp.to(device), put(go, offsets[1]), inv.to(device), out, inv_len.to(device),
                                given=given)
    return out


def _check(device, x, key, go, what, dummy_ends=False, offsets=(0, 0, 0)):
    """recompute against given, and both against fp64, on operands made from (x, key, go); returns the recomputed result"""
    _, co = _mods()
    inv, inv_len = co.groups_from_key(key)
    cp = co.cumprod_forward(x, key)
    want = co.cumprod_backward_f64(x, cp, go, inv)
    scale = co.cumprod_backward_f64(x, cp, go.abs(), inv)
    if dummy_ends:  # every range falls back to the runs of `inv`, which a key array has too
        inv, inv_len = key, torch.zeros(1, dtype=torch.int32)
    new = _run(device, x, cp, go, inv, inv_len, False, offsets)
    old = _run(device, x, cp, go, inv, inv_len, True, offsets)
    assert_parity(new, want, scale, f"{what}: recomputed y vs fp64")
    assert_parity(old, want, scale, f"{what}: given y vs fp64")
    assert_parity(new, old.cpu(), scale, f"{what}: recomputed vs given y")
    return new


def _n_three_tiles():
    gc, _ = _mods()
    assert gc.tile_elems() == TILE
    return 3 * TILE + 77


@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 3 * TILE + 77])
@pytest.mark.parametrize("dist", ["geo80", "poisson8"])
def test_sizes(device, n, dist):
    _n_three_tiles()
    key = make_keys(n, dist, seed=n + 17)
    _check(device, make_values(n, seed=n), key, make_values(n, seed=n + 3, kind="normal"), f"n={n} {dist}")


def _edge_lens():
    return {
        "head_on_every_wave_edge": [WAVE],                  # the anchor must be ignored everywhere
        "head_one_after_every_wave_edge": [WAVE + 1, WAVE],  # groups enter every range by one element
        "head_one_before_every_wave_edge": [WAVE - 1, WAVE],
        "straddling_every_edge": [WAVE // 2, WAVE],          # every wave and tile edge lies inside a group
        "groups_of_1": [1],                                  # more than 255 ends per range: heads from `inv`
        "groups_of_300": [300],
        "groups_of_5000": [5000],                            # longer than a tile: look-back and tree on the given y
        "one_group": [1 << 30],                              # the tree path
    }


@pytest.mark.parametrize("name", sorted(_edge_lens()))
@pytest.mark.parametrize("dummy_ends", [False, True], ids=["inv_len", "keys_as_inv"])
def test_heads_edges_and_run_lengths(device, name, dummy_ends):
    n = _n_three_tiles()
    key = _key_from_lens(n, _edge_lens()[name])
    kind = "near1" if name in ("groups_of_5000", "one_group") else "alpha"  # long products stay O(1)
    _check(device, make_values(n, seed=5, kind=kind), key, make_values(n, seed=8, kind="normal"), name, dummy_ends=dummy_ends)


@pytest.mark.parametrize("lens", [[300], [WAVE // 2, WAVE], [WAVE], [1 << 30]], ids=["300", "straddling", "on_edges", "one_group"])
def test_zeros_in_param_next_to_the_edges(device, lens):
    """A zero makes the recomputed y exactly 0 behind it inside its group, as the forward's is, on either side of a wave
    or tile edge (where the zero reaches the next range through the anchor), at element 0 and at the last element."""
    _, co = _mods()
    t, n = TILE, _n_three_tiles()
    key = _key_from_lens(n, lens)
    x = make_values(n, seed=2, kind="near1")
    zeros = [0, n - 1]
    for edge in (WAVE, 2 * WAVE, t, t + WAVE, 2 * t, 3 * t):
        zeros += [edge - 1, edge]
    # not both sides of one edge in one input: a zero just before an edge would hide the one just after it
    for pick in (zeros[0::2], zeros[1::2]):
        xz = x.clone()
        xz[torch.tensor(pick)] = 0.0
        go = make_values(n, seed=9, kind="normal")
        new = _check(device, xz, key, go, f"zeros at {pick}")
        # from a zero to the end of its group every y is exactly 0, and with it every term of those elements' sums
        cp = co.cumprod_forward(xz, key)
        inv, _ = co.groups_from_key(key)
        all_dead = co.cumprod_backward_f64(xz, (cp != 0).float(), torch.ones(n), inv) == 0  # no live term from here on
        assert bool(all_dead.any()) and bool((new.cpu()[all_dead] == 0).all())


@pytest.mark.parametrize("offsets", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)], ids=["param", "grad_out", "grad_in", "all"])
def test_views_one_element_off_a_16_byte_boundary(device, offsets):
    n = _n_three_tiles()
    key = _key_from_lens(n, [300, 5, 1500, 64])
    x, go = make_values(n, seed=4), make_values(n, seed=6, kind="normal")
    new = _check(device, x, key, go, f"offsets {offsets}", offsets=offsets)
    assert torch.equal(new, _check(device, x, key, go, "aligned"))  # the dword path does the same arithmetic


def test_two_calls_give_the_same_bits(device):
    _, co = _mods()
    n = _n_three_tiles()
    for lens in ([300], [5000], [1 << 30]):
        key = _key_from_lens(n, lens)
        x, go = make_values(n, seed=12, kind="near1"), make_values(n, seed=13, kind="normal")
        inv, inv_len = co.groups_from_key(key)
        cp = co.cumprod_forward(x, key)
        a = _run(device, x, cp, go, inv, inv_len, False)
        b = _run(device, x, cp, go, inv, inv_len, False)
        assert torch.equal(a, b)


def test_error_vs_fp64_is_no_worse_than_the_sequential_fp32_path(device):
    """tests/test_golden_gpu.py's rule on a smaller scene: rms error against fp64 <= 1.25 x the sequential fp32 port's."""
    _, co = _mods()
    from simplegaussiansplat_tk71_amd import synthetic

    p = synthetic.make_pairs(200, 300, 20.0, deep=True, seed=7)
    cp = co.cumprod_forward(p.x, p.key)
    b64 = co.cumprod_backward_f64(p.x, cp, p.grad_out, p.inv)
    b32 = co.cumprod_backward(p.x, cp, p.grad_out, p.inv, p.inv_len)
    rms = lambda a: float(((a.double() - b64) ** 2).mean().sqrt())  # noqa: E731
    e_cpu = rms(b32)
    for given in (False, True):
        e_gpu = rms(_run(device, p.x, cp, p.grad_out, p.inv, p.inv_len, given).cpu())
        print(f"rms error vs fp64: given={given} gpu {e_gpu:.3g} cpu-fp32 {e_cpu:.3g}")
        assert e_gpu <= 1.25 * e_cpu + 1e-12, (given, e_gpu, e_cpu)


def test_given_serves_a_per_group_multiple_of_the_product(device):
    """The sum is linear in y: with y scaled by a factor c per group (what the carry forward produces), the kernel that
    reads the given y returns c times the plain result."""
    _, co = _mods()
    n = _n_three_tiles()
    key = _key_from_lens(n, [300, 5, 1500, 64, 5000])
    x, go = make_values(n, seed=21, kind="near1"), make_values(n, seed=22, kind="normal")
    inv, inv_len = co.groups_from_key(key)
    cp = co.cumprod_forward(x, key)
    c = (0.25 + 1.5 * torch.rand(inv_len.numel(), generator=torch.Generator().manual_seed(3)))[inv.long()]
    plain64 = co.cumprod_backward_f64(x, cp, go, inv)
    scale = co.cumprod_backward_f64(x, cp, go.abs(), inv)
    got = _run(device, x, cp * c, go, inv, inv_len, True)
    assert_parity(got, c.double() * plain64, c.double() * scale, "given y = c * product")
    plain = _run(device, x, cp, go, inv, inv_len, True)
    assert_parity(got, c.double() * plain.cpu().double(), c.double() * scale, "given y = c * product vs c * plain launch")
