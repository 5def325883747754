"""Guarded allocations: every block a wrapper allocates sits in the middle of a buffer painted 0xA5, so a store next to
an output or a workspace, an output element the kernel skipped and a result that depends on what the buffer held before
all become visible ("Write guards").  Plain torch, CPU tensors as well as device tensors.

    arena = Arena()
    guarded(monkeypatch, arena, raster)      # raster's global name `torch` now allocates from the arena
    out = raster.exclusive_scan_i32(x)
    assert arena.check() == [] and arena.unwritten(out) == 0

The harness reads and writes only buffers it allocated itself.
"""
import math

import torch

GUARD_BYTES = 1 << 16   # each side; wider than one 4096-element float32 scan tile and than any vector store
PAINT = 0xA5
_WORD = {1: (torch.uint8, 0xA5), 2: (torch.int16, 0xA5A5 - (1 << 16)), 4: (torch.int32, 0xA5A5A5A5 - (1 << 32))}
_KNOWN = {"dtype", "device", "pin_memory", "offset_bytes"}
ALLOCATORS = ("empty", "zeros", "ones", "full", "empty_like", "zeros_like", "ones_like", "full_like")


class Block:
    def __init__(self, order, raw, lo, nbytes, dtype, shape):
        self.order, self.raw, self.lo, self.nbytes, self.dtype, self.shape = order, raw, lo, nbytes, dtype, shape

    def __repr__(self):
        return f"block #{self.order} {self.dtype} {tuple(self.shape)}"


class Arena:
    """Allocator of guarded blocks.  A call that names no device allocates on the CPU, as torch's does; `offset_bytes`: the
    default placement of the middle past its aligned position (per call: `offset_bytes=`)."""

    def __init__(self, guard_bytes=GUARD_BYTES, offset_bytes=0):
        assert guard_bytes >= GUARD_BYTES and guard_bytes % 512 == 0, "guard: at least 64 KiB and a multiple of 512 bytes"
        self.device = torch.device("cpu")
        self.guard = guard_bytes
        self.offset_bytes = offset_bytes
        self.blocks = []

    # ---- allocation -------------------------------------------------------------------------------------------------
    @staticmethod
    def _shape(size):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        return tuple(int(s) for s in size)

    def _alloc(self, shape, kwargs, like=None):
        unknown = set(kwargs) - _KNOWN
        if unknown:
            raise TypeError(f"guarded allocation: unknown keyword(s) {sorted(unknown)}")
        dtype = kwargs.get("dtype") or (like.dtype if like is not None else torch.get_default_dtype())
        device = kwargs.get("device")
        device = torch.device(device) if device is not None else (like.device if like is not None else self.device)
        offset = kwargs.get("offset_bytes", self.offset_bytes)
        assert offset in (0, 4, 8, 12), "offset_bytes: 0, 4, 8 or 12"
        n = math.prod(shape)
        if n == 0:
            return torch.empty(shape, dtype=dtype, device=device)
        nbytes = n * torch.empty(0, dtype=dtype).element_size()
        assert offset % torch.empty(0, dtype=dtype).element_size() == 0, "offset_bytes: not a multiple of the element size"
        lo = self.guard + offset  # the skipped bytes count as guard
        raw = torch.full((lo + nbytes + self.guard,), PAINT, dtype=torch.uint8, device=device,
                         pin_memory=bool(kwargs.get("pin_memory", False)))
        assert raw.data_ptr() % 16 == 0
        self.blocks.append(Block(len(self.blocks), raw, lo, nbytes, dtype, shape))
        return raw[lo:lo + nbytes].view(dtype).view(shape)

    def empty(self, *size, **kwargs):
        return self._alloc(self._shape(size), kwargs)

    def full(self, size, fill_value, **kwargs):
        t = self._alloc(self._shape((size,)), kwargs)
        return t.fill_(fill_value) if t.numel() else t

    def zeros(self, *size, **kwargs):
        return self.full(self._shape(size), 0, **kwargs)

    def ones(self, *size, **kwargs):
        return self.full(self._shape(size), 1, **kwargs)

    def empty_like(self, t, **kwargs):
        assert t.is_contiguous(), "guarded *_like: a dense source only (the package passes no other)"
        return self._alloc(tuple(t.shape), kwargs, like=t)

    def full_like(self, t, fill_value, **kwargs):
        out = self.empty_like(t, **kwargs)
        return out.fill_(fill_value) if out.numel() else out

    def zeros_like(self, t, **kwargs):
        return self.full_like(t, 0, **kwargs)

    def ones_like(self, t, **kwargs):
        return self.full_like(t, 1, **kwargs)

    def copy(self, t, **kwargs):
        """A guarded block with the bits of `t` (how a test places its inputs)."""
        out = self._alloc(tuple(t.shape), kwargs, like=t)
        if out.numel():
            out.copy_(t.detach())
        return out

    # ---- inspection -------------------------------------------------------------------------------------------------
    def check(self):
        """One record per block and side whose guard bytes are not all 0xA5; byte offsets count from the block's first
        byte (negative in the front guard, >= nbytes behind it)."""
        found = []
        for b in self.blocks:
            for side, part, base in (("before", b.raw[:b.lo], -b.lo), ("after", b.raw[b.lo + b.nbytes:], b.nbytes)):
                hit = (part != PAINT).nonzero().flatten()
                if hit.numel():
                    found.append({"order": b.order, "dtype": b.dtype, "shape": b.shape, "side": side,
                                  "first": base + int(hit[0]), "last": base + int(hit[-1])})
        return found

    def unwritten(self, t):
        """Number of 32-bit words of `t` that still hold the paint (16-bit words / bytes for 2- / 1-byte dtypes)."""
        if t.numel() == 0:
            return 0
        dtype, paint = _WORD[min(t.element_size(), 4)]
        return int((_bytes(t).view(dtype) == paint).sum())


class TorchProxy:
    """Stands in for the module `torch` in a package module's globals: the allocation functions go to the arena,
    everything else (dtypes, torch.cuda, torch.Tensor, every operator) is torch's own."""

    def __init__(self, arena):
        self.__dict__["_arena"] = arena

    def __getattr__(self, name):
        if name in ALLOCATORS:
            return getattr(self.__dict__["_arena"], name)
        return getattr(torch, name)


def guarded(monkeypatch, arena, *modules):
    """The listed package modules allocate from `arena` until pytest undoes the patch; `torch` itself is untouched."""
    proxy = TorchProxy(arena)
    for m in modules:
        assert m.__name__.split(".")[0] != "torch" and isinstance(getattr(m, "torch", None), type(torch)), m
        monkeypatch.setattr(m, "torch", proxy)
    return proxy


def _bytes(t):
    """The elements of `t` in order as a dense uint8 vector (a copy: a one-element view may keep any stride)."""
    src = t.detach().reshape(-1)
    if src.dtype == torch.bool:
        src = src.view(torch.uint8)  # same size: any stride; a bool copy would turn every non-zero byte into 1
    return torch.empty(src.numel(), dtype=src.dtype, device=src.device).copy_(src).view(torch.uint8)


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(_bytes(a), _bytes(b))
