"""The guarded-allocation harness has teeth (no GPU: CPU tensors stand in for device memory).

Stand-in "package modules" are built here with `types.ModuleType`; their wrappers look `torch` up in the module's globals at
call time, as the package's own do, so `guarded` serves them from the arena.
"""
import types

import pytest
import torch

from tests.guarded_alloc import GUARD_BYTES, Arena, TorchProxy, guarded, same_bits


def _module(source):
    m = types.ModuleType("standin")
    m.torch = torch
    exec(source, m.__dict__)
    return m


STANDIN = _module('''
def fill(n):
    out = torch.empty(n, dtype=torch.float32)
    out.copy_(torch.arange(n, dtype=torch.float32) + 1.0)
    return out


def with_workspace(n):
    out = torch.empty(n, dtype=torch.float32)
    ws = torch.empty(4 * n + 16, dtype=torch.uint8)
    ws.fill_(3)
    out.copy_(ws[:n].float())
    return out


def stray(n, elem):
    """Writes element `elem` of the output's own storage, wherever that lies around the output."""
    out = torch.empty(n, dtype=torch.float32)
    out.fill_(1.0)
    torch.as_strided(out, (1,), (1,), out.storage_offset() + elem).fill_(7.0)
    return out


def never(n, dtype):
    return torch.empty(n, dtype=dtype)


def prefix(n, k, dtype):
    out = torch.empty(n, dtype=dtype)
    out[:k] = 1
    return out


def typed():
    assert isinstance(torch.empty(3), torch.Tensor) and torch.float32.is_floating_point
    return torch.cuda.is_available(), torch.arange(3).sum().item()
''')


@pytest.fixture
def arena(monkeypatch):
    a = Arena()
    guarded(monkeypatch, a, STANDIN)
    return a


def test_guard_is_64_kib_and_keeps_torchs_alignment():
    assert GUARD_BYTES >= 1 << 16 and GUARD_BYTES % 512 == 0
    with pytest.raises(AssertionError):
        Arena(guard_bytes=1 << 15)
    with pytest.raises(AssertionError):
        Arena(guard_bytes=(1 << 16) + 64)
    a = Arena()
    t = a.empty(5, dtype=torch.float32)
    raw = a.blocks[0].raw
    assert t.data_ptr() - raw.data_ptr() == GUARD_BYTES and raw.numel() == 2 * GUARD_BYTES + 20
    assert t.data_ptr() % 16 == 0 and bool((raw == 0xA5).all())


def test_well_behaved_wrappers_pass(arena):
    out = STANDIN.fill(1000)
    assert torch.equal(out, torch.arange(1000, dtype=torch.float32) + 1.0)
    out2 = STANDIN.with_workspace(77)
    assert len(arena.blocks) == 3 and arena.blocks[2].nbytes == 4 * 77 + 16  # exactly the size asked for
    assert arena.check() == []
    assert arena.unwritten(out) == 0 and arena.unwritten(out2) == 0


@pytest.mark.parametrize("n,elem,side,first", [
    (10, -1, "before", -4),                 # one element before the start
    (10, 10, "after", 40),                  # one past the end
    (10, 10 + 60 * 256, "after", 40 + 60 * 1024),  # 60 KiB past the end
    (4097, 4097, "after", 4 * 4097),
])
def test_stray_writes_are_reported_with_side_and_offset(arena, n, elem, side, first):
    STANDIN.fill(3)
    STANDIN.stray(n, elem)
    found = arena.check()
    # 7.0f is the bytes 00 00 E0 40: all four differ from the paint
    assert found == [{"order": 1, "dtype": torch.float32, "shape": (n,), "side": side, "first": first, "last": first + 3}]


def test_stray_write_reports_all_damaged_bytes():
    a = Arena()
    t = a.empty(10, dtype=torch.float32)
    torch.as_strided(t, (2,), (1,), t.storage_offset() + 10).fill_(7.0)
    torch.as_strided(t, (1,), (1,), t.storage_offset() - 3).fill_(7.0)
    assert a.check() == [
        {"order": 0, "dtype": torch.float32, "shape": (10,), "side": "before", "first": -12, "last": -9},
        {"order": 0, "dtype": torch.float32, "shape": (10,), "side": "after", "first": 40, "last": 47},
    ]


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.bool, torch.uint8])
def test_unwritten_outputs_are_counted(arena, dtype):
    out = STANDIN.never(37, dtype)
    assert arena.unwritten(out) == 37
    out = STANDIN.prefix(37, 30, dtype)
    assert arena.unwritten(out) == 7
    assert arena.unwritten(out[:30]) == 0 and arena.unwritten(out[29:]) == 7
    assert arena.check() == []


@pytest.mark.parametrize("offset", [0, 4, 8, 12])
def test_offset_bytes_places_the_block_off_alignment(offset):
    a = Arena(offset_bytes=offset)
    t = a.empty(100, dtype=torch.float32)
    assert t.data_ptr() % 16 == offset
    u = Arena().zeros(9, dtype=torch.float32, offset_bytes=offset)
    assert u.data_ptr() % 16 == offset and not u.any()
    # the skipped bytes count as guard
    t.fill_(1.0)
    if offset:
        torch.as_strided(t, (1,), (1,), t.storage_offset() - 1).fill_(7.0)
        assert [(f["side"], f["first"], f["last"]) for f in a.check()] == [("before", -4, -1)]
    with pytest.raises(AssertionError):
        Arena().empty(8, dtype=torch.int64, offset_bytes=4)


def test_every_allocation_form_of_the_package_is_accepted():
    """The forms below are the ones a search of simplegaussiansplat_tk71_amd/*.py for torch.(empty|zeros|ones|full)(_like)?(
    finds (file: example)."""
    a = Arena()
    p = TorchProxy(a)
    dev = torch.device("cpu")
    n, tail, shape = 7, (2, 2), (5, 6)
    like = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    got = [
        p.empty(n, dtype=torch.int32, device=dev),                      # raster: torch.empty(n + 1, dtype=..., device=dev)
        p.empty(n, 2, dtype=torch.int32, device=dev),                   # raster: torch.empty(m, 2, dtype=..., device=dev)
        p.empty(n, *tail, dtype=torch.float32, device=dev),             # raster: torch.empty(n, *tail, dtype=..., device=dev)
        p.empty(*shape, 3, dtype=torch.float32, device=dev),            # raster: torch.empty(*shape, 3, ...)
        p.empty(shape, dtype=torch.float32, device=dev),                # raster / projection: torch.empty(shape_tuple, ...)
        p.empty((n, *like.shape[1:]), dtype=torch.float32, device=dev),  # density / lens: torch.empty((m, *t.shape[1:]), ...)
        p.empty((n, 1), dtype=torch.float32, device=dev),               # filter3d
        p.empty(n, 3, dtype=torch.float64, device=dev),                 # loss.image_metrics
        p.empty(n, dtype=torch.uint8, device=dev),                      # workspaces, keep masks
        p.empty(n, dtype=torch.int64, device=dev),                      # projection: boxsize, index
        p.empty(n, dtype=torch.float32, pin_memory=False),              # optim: host staging (pin_memory=True on a ROCm host)
        p.empty(()),                                                    # a scalar block
        p.zeros(n, dtype=torch.float32, device=dev),                    # filter3d, gs_model
        p.zeros(*shape, 3, dtype=torch.float32, device=dev),            # raster: zero grad_image
        p.zeros(n, 3, 4, dtype=torch.float32, device=dev),              # exposure
        p.zeros((n, 1), device=dev, dtype=torch.float32),               # gs_model: keywords in the other order
        p.zeros(shape, dtype=torch.float32, device=dev),                # mesh.TSDFVolume
        p.zeros((3, *shape), dtype=torch.float32, device=dev),          # mesh.TSDFVolume rgb
        p.zeros(1, dtype=torch.int32, device=dev),                      # density, cuda_kernel
        p.zeros(0, dtype=torch.bool, device=dev),                       # cuda_kernel: empty mask
        p.zeros(0, 2, dtype=torch.int32, device=dev),                   # raster.rects_to_boxes of an empty list
        p.zeros(n, dtype=torch.int16, device=dev),                      # gs_model
        p.zeros(n + 2, dtype=torch.int64),                              # sharding: host, no device
        p.ones(shape, dtype=torch.float32, device=dev),                 # mesh.TSDFVolume tsdf
        p.full((n,), 8.0, device=dev),                                  # synthetic
        p.empty_like(like),                                             # everywhere
        p.zeros_like(like),                                             # optim, exposure
        p.ones_like(like > 2),                                          # gs_model (bool)
        p.full_like(like, float("inf")),                                # filter3d
        p.full_like(like, 0.25),                                        # gs_model
    ]
    want = [
        ((7,), torch.int32), ((7, 2), torch.int32), ((7, 2, 2), torch.float32), ((5, 6, 3), torch.float32), ((5, 6), torch.float32),
        ((7, 3), torch.float32), ((7, 1), torch.float32), ((7, 3), torch.float64), ((7,), torch.uint8), ((7,), torch.int64),
        ((7,), torch.float32), ((), torch.float32), ((7,), torch.float32), ((5, 6, 3), torch.float32), ((7, 3, 4), torch.float32),
        ((7, 1), torch.float32), ((5, 6), torch.float32), ((3, 5, 6), torch.float32), ((1,), torch.int32), ((0,), torch.bool),
        ((0, 2), torch.int32), ((7,), torch.int16), ((9,), torch.int64), ((5, 6), torch.float32), ((7,), torch.float32),
        ((2, 3), torch.float32), ((2, 3), torch.float32), ((2, 3), torch.bool), ((2, 3), torch.float32), ((2, 3), torch.float32),
    ]
    assert [(tuple(t.shape), t.dtype) for t in got] == want
    assert all(t.is_contiguous() and t.device == dev for t in got)
    assert len(a.blocks) == len(got) - 2  # size 0: ordinary empty tensors
    for t in got[12:23]:
        assert not t.any()
    assert bool((got[23] == 1).all()) and bool((got[24] == 8).all()) and bool(got[27].all())
    assert bool(torch.isinf(got[28]).all()) and bool((got[29] == 0.25).all()) and not got[26].any()
    # zeros and its relatives fill only the middle
    assert a.check() == []
    assert a.unwritten(got[0]) == 7 and a.unwritten(got[25]) == 6


def test_unknown_keywords_are_refused():
    p = TorchProxy(Arena())
    with pytest.raises(TypeError, match="requires_grad"):
        p.empty(3, dtype=torch.float32, requires_grad=True)
    with pytest.raises(TypeError, match="layout"):
        p.zeros_like(torch.zeros(3), layout=torch.strided)
    with pytest.raises(TypeError, match="out"):
        p.full((3,), 1.0, out=torch.zeros(3))


def test_the_proxy_forwards_everything_else_and_the_patch_is_undone(monkeypatch):
    a = Arena()
    with monkeypatch.context() as mp:
        proxy = guarded(mp, a, STANDIN)
        assert STANDIN.torch is proxy and proxy.float32 is torch.float32 and proxy.Tensor is torch.Tensor
        assert proxy.cuda is torch.cuda and proxy.autograd.Function is torch.autograd.Function
        assert STANDIN.typed() == (torch.cuda.is_available(), 3)
        assert len(a.blocks) == 1
    assert STANDIN.torch is torch
    STANDIN.fill(4)
    assert len(a.blocks) == 1
    with pytest.raises(AssertionError):
        guarded(monkeypatch, a, torch.nn)  # never torch's own modules


def test_same_bits_is_bitwise():
    z = torch.zeros(3)
    assert same_bits(z, z.clone()) and not same_bits(z, -z)  # -0.0 == 0.0 but the bits differ
    nan = torch.full((2,), float("nan"))
    assert same_bits(nan, nan.clone()) and not same_bits(z, z.double()) and not same_bits(z, z[:2])
    assert same_bits(torch.zeros(0), torch.zeros(0))
