"""csrc/gcp_bin.hip and k_pixel_lists (csrc/gcp_walk.hip) against the numpy reference of tests/bin_tiles_ref.py, entry by
entry, at the tile, chunk and wave edges its case table is built for (tests/test_bin_tiles.py shows, without a GPU, that
every case reaches its edge and that the reference equals the brute-force definition).  Integer work: every comparison is
exact."""
import numpy as np
import pytest
import torch

from tests import bin_tiles_ref as br

pytestmark = pytest.mark.gpu

NAMES = list(br.CASES)
OVERFLOW = [(name, kind) for name in NAMES if br.case(name)[4][0][-1] >= 2
            for kind in br.overflow_capacities(br.case(name)[4][0], br.case(name)[4][3])]

_on_device = {}


def _inputs(name, device):
    """(start, end) of the case on the device, uploaded once."""
    if name not in _on_device:
        start, end = br.case(name)[:2]
        _on_device[name] = (torch.tensor(start, device=device), torch.tensor(end, device=device))
    return _on_device[name]


def _same(got, want):
    """An int32 device tensor equals an int64 numpy reference, element by element."""
    assert got.dtype == torch.int32
    return tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy().astype(np.int64), want)


@pytest.mark.parametrize("name", NAMES)
def test_exact_route(device, name):
    from simplegaussiansplat_tk71_amd import raster

    _, _, W, H, (tile_off, tile_start, tile_list, _, tiles_x, tiles_y) = br.case(name)
    start, end = _inputs(name, device)
    bins = raster.bin_tiles(start, end, W, H)
    assert (bins.tiles_x, bins.tiles_y, bins.n_tile_pairs) == (tiles_x, tiles_y, int(tile_off[-1]))
    assert _same(bins.tile_off, tile_off)
    assert _same(bins.tile_start, tile_start)
    assert _same(bins.tile_list, tile_list)


@pytest.mark.parametrize("name", NAMES)
def test_capture_safe_route_with_sufficient_capacity(device, name):
    from simplegaussiansplat_tk71_amd import raster

    _, _, W, H, (tile_off, tile_start, tile_list, _, _, _) = br.case(name)
    start, end = _inputs(name, device)
    K = int(tile_off[-1])
    for cap in (max(K, 1), K + 1, K + 4097):
        bins = raster.bin_tiles(start, end, W, H, capacity=cap)
        assert bins.info.tolist() == [K, 0], cap
        assert _same(bins.tile_off, tile_off), cap
        assert _same(bins.tile_start, tile_start), cap
        assert _same(bins.tile_list[:K], tile_list), cap


@pytest.mark.parametrize("name,kind", OVERFLOW)
def test_capture_safe_route_with_insufficient_capacity(device, name, kind):
    """The Gaussians whose entries end at or below the capacity are listed exactly as if the others did not exist; the
    first one that does not fit is left out with everything behind it."""
    from simplegaussiansplat_tk71_amd import raster

    s, e, W, H, (tile_off, _, _, counts, _, _) = br.case(name)
    start, end = _inputs(name, device)
    cap = br.overflow_capacities(tile_off, counts)[kind]
    assert 1 <= cap < tile_off[-1]
    n_kept = int((tile_off[1:] <= cap).sum())
    listed = int(tile_off[n_kept])
    _, part_start, part_list, _, _, _ = br.bin_reference(s[:n_kept], e[:n_kept], W, H)
    assert part_list.size == listed
    bins = raster.bin_tiles(start, end, W, H, capacity=cap)
    assert bins.info.tolist() == [listed, 1]
    assert _same(bins.tile_off, tile_off)
    assert _same(bins.tile_start, part_start)
    assert _same(bins.tile_list[:listed], part_list)


@pytest.mark.parametrize("name", NAMES)
def test_fill_on_the_callers_prefix_sum(device, name):
    from simplegaussiansplat_tk71_amd import raster

    _, _, W, H, (tile_off, tile_start, tile_list, _, _, _) = br.case(name)
    start, end = _inputs(name, device)
    counted = torch.tensor(tile_off, dtype=torch.int32, device=device)
    bins = raster.bin_tiles(start, end, W, H, counted=(counted, int(tile_off[-1])))
    assert bins.n_tile_pairs == int(tile_off[-1])
    assert _same(bins.tile_start, tile_start)
    assert _same(bins.tile_list, tile_list)


def test_capture_safe_route_with_more_than_int32_entries(device):
    """80 000 boxes over a whole 3840x2160 frame: 2.6e9 entries, the int32 prefix sums have wrapped.  Nothing is listed
    and the overflow is flagged; the emit, sort and bounds kernels run on empty input."""
    from simplegaussiansplat_tk71_amd import raster

    n = 80_000
    start = torch.zeros(n, 2, dtype=torch.int32, device=device)
    end = torch.tensor([[3839, 2159]], dtype=torch.int32, device=device).repeat(n, 1)
    bins = raster.bin_tiles(start, end, 3839, 2159, capacity=4096)
    assert bins.info.tolist() == [0, 1] and bins.overflowed()
    assert bins.tile_start.numel() == 240 * 135 + 1 and not bool(bins.tile_start.any())


@pytest.mark.parametrize("name", br.PIXEL_LIST_CASES)
def test_pixel_lists(device, name):
    from simplegaussiansplat_tk71_amd import raster

    s, e, W, H, _ = br.case(name)
    start, end = _inputs(name, device)
    box_off, pair_index, pair_gauss, pair_key, pixel_off = br.pixel_lists_reference(s, e, W, H)
    pl = raster.pixel_lists(raster.bin_tiles(start, end, W, H), start, end)
    assert _same(pl.pixel_off, pixel_off)
    assert _same(pl.box_off, box_off)
    assert _same(pl.pair_gauss, pair_gauss)
    assert _same(pl.pair_index, pair_index)
    assert _same(pl.pair_key, pair_key)


@pytest.mark.parametrize("name,max_half,seed", [("frame_30x17", 9, 41), ("deep_overhang", 12, 42)])
def test_every_kernel_clips_as_the_binning_does(device, name, max_half, seed):
    """Blend forward and backward on boxes that overhang the frame, lie outside it or are inverted, against the same
    boxes clipped on the host (empty ones replaced by an inverted box).  load_box is the only place a kernel reads
    start / end, so both runs see the same clipped boxes, the same counts and the same tile_off: every bit is equal."""
    from simplegaussiansplat_tk71_amd import raster

    s, e, W, H, (_, _, _, counts, _, _) = br.case(name)
    n = s.shape[0]
    x0, y0, x1, y1, live = br.clip_boxes(s, e, W, H)
    assert np.array_equal(live, counts > 0) and 0 < int(live.sum()) < n and not np.array_equal(x0, s[:, 0])
    clipped_start = np.where(live[:, None], np.stack([x0, y0], 1), 1).astype(np.int32)
    clipped_end = np.where(live[:, None], np.stack([x1, y1], 1), 0).astype(np.int32)
    # per-Gaussian parameters as tests.util.make_scene draws them, the mean at the centre of the box as given
    g = torch.Generator().manual_seed(seed)
    mean = torch.tensor((s.astype(np.int64) + e.astype(np.int64)) // 2, dtype=torch.int32)
    sx = 0.6 + 0.35 * max_half * torch.rand(n, generator=g)
    sy = 0.6 + 0.35 * max_half * torch.rand(n, generator=g)
    rho = 0.8 * (torch.rand(n, generator=g) - 0.5)
    cov = torch.stack([sx * sx, rho * sx * sy, rho * sx * sy, sy * sy], 1).reshape(-1, 2, 2)
    vinv = torch.linalg.inv(cov).to(torch.float32).contiguous()
    opacity = (0.05 + 0.9 * torch.rand(n, 1, generator=g)).to(torch.float32)
    l_d = (0.05 + 0.95 * torch.rand(n, 3, generator=g)).to(torch.float32)
    wimg = torch.randn(H + 1, W + 1, 3, generator=g).to(device)
    rest = tuple(t.to(device) for t in (mean, vinv, opacity, l_d))
    out = []
    for start, end in (_inputs(name, device), (torch.tensor(clipped_start, device=device), torch.tensor(clipped_end, device=device))):
        bins = raster.bin_tiles(start, end, W, H)
        img, ck = raster.blend_forward(bins, start, end, *rest, with_checkpoints=True)
        grads = raster.blend_backward(bins, start, end, *rest, ck, wimg)
        out.append((bins.tile_off, bins.tile_start, bins.tile_list, img, *grads))
    assert len(out[0]) == 8
    for given, clipped, what in zip(out[0], out[1], ("tile_off", "tile_start", "tile_list", "image", "grad_mean", "grad_vinv",
                                                     "grad_opacity", "grad_l_d")):
        assert torch.equal(given, clipped), what
    assert float(out[0][3].abs().sum()) > 0.0
    dead = torch.tensor(~live, device=device)
    for grad, what in zip(out[0][4:], ("grad_mean", "grad_vinv", "grad_opacity", "grad_l_d")):
        assert float(grad.abs().sum()) > 0.0, what
        assert not bool(grad[dead].any()), what
