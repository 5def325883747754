"""The backward scan takes its group ends from `inv_len` wherever (inv, inv_len) describe a wave's range exactly, and
falls back to the runs of `inv` elsewhere (include/grouped_cumprod_hip.h, gcp_cumprod_backward).  Both sources must
give the same bits: the fast path is compared BIT FOR BIT with a run where every wave falls back (inv = the pixel key,
inv_len = zeros(1), which fails the range check everywhere)."""
import pytest
import torch

from tests.util import make_keys, make_values

pytestmark = pytest.mark.gpu

DISTS = ["poisson8", "geo80", "runs3000", "runs9000", "one_run", "mixed", "all1"]
SIZES = [1000, 4096, 3 * 4096, 5 * 4096 + 1234, 300_017]


def _mods():
    import grouped_cumprod as gc
    from oracle import c_oracle as co

    return gc, co


def _inputs(n, dist, seed, device, offset=0):
    """(x, cumprod, grad_out, key, inv, inv_len) on the device; offset 1 gives views that are not 16-byte aligned."""
    gc, co = _mods()
    key = make_keys(n, dist, seed)
    inv, inv_len = co.groups_from_key(key)

    def put(t):
        buf = torch.zeros(n + offset, dtype=t.dtype, device=device)
        buf[offset:] = t.to(device)
        return buf[offset:]

    x = put(make_values(n, seed, "near1" if dist in ("runs3000", "runs9000", "one_run", "mixed") else "alpha"))
    y = torch.empty_like(x)
    gc.grouped_cumprod_forward(x, put(inv), y)
    go = put(make_values(n, seed + 3, "normal"))
    return x, y, go, put(key), put(inv), inv_len.to(device)


def _both(x, y, go, key, inv, inv_len):
    gc, _ = _mods()
    fast = torch.full_like(x, float("nan"))
    gc.grouped_cumprod_backward(x, y, go, inv, fast, inv_len)
    runs = torch.full_like(x, float("nan"))
    gc.grouped_cumprod_backward(x, y, go, key, runs, torch.zeros(1, dtype=torch.int32, device=x.device))
    return fast, runs


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dist", DISTS)
def test_group_ends_match_runs_bitwise(device, dist, n, offset):
    fast, runs = _both(*_inputs(n, dist, n + 11, device, offset))
    assert not torch.isnan(fast).any()
    assert torch.equal(fast, runs), (dist, n, offset, int((fast != runs).sum()))


@pytest.mark.parametrize("dist", ["one_run", "runs9000", "mixed", "geo80"])
def test_group_ends_under_every_descriptor_wait(device, dist):
    """The raw look-back window, the descriptor walk and the follow-up kernel's re-run (wait 200 / 0 / -1 us) take the
    same flag source: all settings and both sources agree bit for bit."""
    gc, _ = _mods()
    args = _inputs(3_000_017, dist, 31, device)
    try:
        ref = None
        for wait in (200, 0, -1):
            gc.set_lookback_wait_us(wait)
            fast, runs = _both(*args)
            assert torch.equal(fast, runs), (dist, wait, int((fast != runs).sum()))
            if ref is None:
                ref = fast
            assert torch.equal(fast, ref), (dist, wait)
    finally:
        gc.set_lookback_wait_us(200)


def test_group_ends_cfg3(device):
    """The benchmark's full-size pair list (166 M pairs, 2.07 M groups)."""
    gc, _ = _mods()
    from simplegaussiansplat_tk71_amd import synthetic

    p = synthetic.make_config("cfg3", seed=1, device=device)
    y = torch.empty_like(p.x)
    gc.grouped_cumprod_forward(p.x, p.key, y)
    fast, runs = _both(p.x, y, p.grad_out, p.key, p.inv, p.inv_len)
    assert torch.equal(fast, runs), int((fast != runs).sum())


def test_grouped_cumprod_autograd_unchanged(device):
    """GroupedCumprod.backward passes the pixel keys as `inv` with a one-entry dummy `inv_len`: every wave falls back,
    so its gradient equals the fast path's.  Key values far outside [0, n_groups) must never index `inv_len`."""
    import cuda_kernel

    gc, co = _mods()
    n = 200_003
    base = make_keys(n, "geo80", 5)
    inv, inv_len = co.groups_from_key(base)
    for key in (base, base + 2_000_000_000, -1 - base):
        x0 = make_values(n, 6).to(device)
        go = make_values(n, 7, "normal").to(device)
        x = x0.clone().requires_grad_(True)
        y = cuda_kernel.GroupedCumprod.apply(x, key.to(device))
        (g,) = torch.autograd.grad(y, x, go)
        want = torch.empty_like(x0)
        gc.grouped_cumprod_backward(x0, y.detach(), go, inv.to(device), want, inv_len.to(device))
        torch.cuda.synchronize()
        assert torch.equal(g, want), int((g != want).sum())
