"""gcp_adam_step_multi (csrc/gcp_optim.hip) without a GPU: the float64 helper the GPU tests measure against is pinned to
torch.optim.Adam, and the entry point's argument validation returns before any HIP call.  Where a refusal needs non-NULL
"device" addresses, 16-byte aligned host buffers stand in: the call must return before anything could read them."""
import ctypes

import pytest
import torch

from tests import adam_torch as at

OK, INVALID = 0, 1  # GCP_OK, GCP_ERR_INVALID_ARGUMENT
NAN, INF = float("nan"), float("inf")


def test_the_helper_with_all_rows_visible_bounds_float32_torch_adam():
    worst = [0.0] * 3
    for i, (step, lr) in enumerate((s, l) for s in (1, 2, 7, 1000, 30000) for l in (1.6e-4, 1e-2, 1.0)):
        gen = torch.Generator().manual_seed(i)
        tensors = [at.state(67, w, gen) for w in at.WIDTHS]
        for (p, g, m, v), (want, bounds, on) in zip(tensors, at.masked_adam(tensors, [step] * 5, [lr] * 5, torch.ones(67, dtype=torch.uint8))):
            assert bool(on.all())
            worst = list(map(max, worst, at.worst(at.torch_step(p, g, m, v, step, lr), want, bounds, what=("float32 torch", step, lr))))
    assert 0.0 < max(worst) <= 1.0
    print(f"float32 torch.optim.Adam, worst error / bound (p, m, v): {worst[0]:.3f} {worst[1]:.3f} {worst[2]:.3f}")


def test_the_helper_leaves_masked_rows_and_matches_the_unmasked_step_elsewhere():
    gen = torch.Generator().manual_seed(3)
    tensors = [at.state(67, w, gen) for w in at.WIDTHS]
    dense = at.masked_adam(tensors, [7] * 5, [1e-2] * 5)
    for name, mask in at.masks(67, 255).items():
        for (p, g, m, v), (want, bounds, on), (dense_want, dense_bounds, _) in zip(tensors, at.masked_adam(tensors, [7] * 5, [1e-2] * 5, mask), dense):
            assert torch.equal(on, mask != 0), name
            for got, old, full, b, fb in zip(want, (p, m, v), dense_want, bounds, dense_bounds):
                assert torch.equal(got[~on], old[~on].double()) and float(b[~on].sum()) == 0.0, name  # untouched, exactly
                assert torch.equal(got[on], full[on]) and torch.equal(b[on], fb[on]), name
    assert [int(m.ne(0).sum()) for m in at.masks(1025).values()] == [1025, 0, 513, 1, 1, 513, 425]


@pytest.fixture(scope="module")
def lib():
    from simplegaussiansplat_tk71_amd import _lib

    return _lib.load()


class Call:
    """A valid gcp_adam_step_multi call over `widths` x `rows`, whose fields a test spoils one at a time."""

    def __init__(self, widths=(3, 4), rows=8):
        self.k = len(widths)
        self.buffers = [ctypes.create_string_buffer(4096 + 16) for _ in range(8)]  # stand-ins for device memory: never read
        aligned = [(ctypes.addressof(b) + 15) // 16 * 16 for b in self.buffers]
        self.param, self.grad, self.exp_avg, self.exp_avg_sq = ([aligned[j] + 1024 * t for t in range(self.k)] for j in range(4))
        self.step = [aligned[4] + 4 * t for t in range(self.k)]
        self.lr, self.scal, self.visible = aligned[5], aligned[6], None
        self.rows, self.width = [rows] * self.k, list(widths)
        self.n_tensors, self.beta1, self.beta2 = self.k, 0.9, 0.999

    def __call__(self, lib):
        arr = lambda kind, vals: None if vals is None else (kind * len(vals))(*vals)  # noqa: E731
        return lib.gcp_adam_step_multi(self.n_tensors, arr(ctypes.c_void_p, self.param), arr(ctypes.c_void_p, self.grad),
                                       arr(ctypes.c_void_p, self.exp_avg), arr(ctypes.c_void_p, self.exp_avg_sq),
                                       arr(ctypes.c_int64, self.rows), arr(ctypes.c_int32, self.width), arr(ctypes.c_void_p, self.step),
                                       self.lr, self.scal, self.visible, self.beta1, self.beta2, 1e-8, None)


def _refused(lib, **spoil):
    call = Call()
    for name, value in spoil.items():
        if isinstance(value, tuple):  # (index, value): one entry of a host array
            getattr(call, name)[value[0]] = value[1]
        else:
            setattr(call, name, value)
    return call(lib)


def test_the_entry_point_is_bound_and_declared(lib):
    import re

    from simplegaussiansplat_tk71_amd import _build, _lib

    with open(_build.INCLUDE + "/grouped_cumprod_hip.h") as f:
        header = f.read()
    assert "gcp_adam_step_multi" in _lib.SIGNATURES and hasattr(lib, "gcp_adam_step_multi")
    assert re.search(r"\bgcp_adam_step_multi\(", header) and re.search(r"#define GCP_ADAM_MAX_TENSORS 8\b", header)
    assert lib.gcp_abi_version() == 4


def test_nothing_to_do_is_a_no_op(lib):
    assert lib.gcp_adam_step_multi(0, None, None, None, None, None, None, None, None, None, None, 0.9, 0.999, 1e-8, None) == OK
    assert lib.gcp_adam_step_multi(0, None, None, None, None, None, None, None, None, None, None, 0.0, 0.0, 1e-8, None) == OK
    assert lib.gcp_last_hip_error() == 0


def test_every_refusal_returns_before_any_hip_call(lib):
    for n in (-1, 9, 2 ** 31 - 1, -(2 ** 31)):
        assert _refused(lib, n_tensors=n) == INVALID, n
        assert lib.gcp_adam_step_multi(n, None, None, None, None, None, None, None, None, None, None, 0.9, 0.999, 1e-8, None) == INVALID, n
    for bad in (1.0, 1.5, -0.1, -1e-300, INF, -INF, NAN):
        assert _refused(lib, beta1=bad) == INVALID and _refused(lib, beta2=bad) == INVALID, bad
        assert lib.gcp_adam_step_multi(0, None, None, None, None, None, None, None, None, None, None, bad, 0.999, 1e-8, None) == INVALID, bad
    for name in ("param", "grad", "exp_avg", "exp_avg_sq"):
        assert _refused(lib, **{name: None}) == INVALID, name             # the host array itself
        for t in (0, 1):
            assert _refused(lib, **{name: (t, None)}) == INVALID, (name, t)  # a NULL tensor with elements to process
            for off in (4, 8, 12, 1):  # misaligned
                call = Call()
                getattr(call, name)[t] += off
                assert call(lib) == INVALID, (name, t, off)
    for name in ("rows", "width", "step", "lr", "scal"):
        assert _refused(lib, **{name: None}) == INVALID, name
    for t in (0, 1):
        assert _refused(lib, step=(t, None)) == INVALID, t
        for w in (0, -1, -(2 ** 31)):
            assert _refused(lib, width=(t, w)) == INVALID, (t, w)
        for r in (-1, -(2 ** 40), -(2 ** 63)):
            assert _refused(lib, rows=(t, r)) == INVALID, (t, r)
        assert _refused(lib, rows=(t, 2 ** 62)) == INVALID, t  # rows * width past int64
    # a mask: every tensor needs the same number of rows
    mask = Call().lr
    assert _refused(lib, visible=mask, rows=(0, 7)) == INVALID and _refused(lib, visible=mask, rows=(1, 9)) == INVALID
    assert _refused(lib, visible=mask, rows=(1, 0)) == INVALID
    # a step count is advanced for an empty tensor too: its pointer is still required, its arrays are not
    call = Call()
    call.rows, call.param, call.step[1] = [0, 0], [None, None], None
    assert call(lib) == INVALID
    assert lib.gcp_last_hip_error() == 0


def test_the_model_and_the_example_take_the_adam_argument():
    """Without a GPU: the three modes and nothing else; a CPU model keeps torch.optim.Adam and cannot be "sparse"; the other
    modes ignore `train_step`'s mask."""
    import inspect

    from examples import train_cameras
    from simplegaussiansplat_tk71_amd import gs_model as gm

    gen = torch.Generator().manual_seed(0)
    args = lambda: (torch.randn(6, 3, generator=gen), torch.randn(6, 4, generator=gen), torch.randn(6, 3, generator=gen),  # noqa: E731
                    torch.randn(6, 1, generator=gen))
    assert gm.ADAM_MODES == ("tensor", "fused", "sparse")
    assert inspect.signature(gm.GS_model_with_param.__init__).parameters["adam"].default == "tensor"
    assert inspect.signature(train_cameras.train).parameters["adam"].default == "tensor"
    assert inspect.signature(gm.HipAdam.__init__).parameters["fused"].default is False
    for bad in ("dense", "", None, "Sparse"):
        with pytest.raises(ValueError):
            gm.GS_model_with_param(*args(), adam=bad)
    with pytest.raises(RuntimeError):
        gm.GS_model_with_param(*args(), adam="sparse")
    for mode in ("tensor", "fused"):
        model = gm.GS_model_with_param(*args(), adam=mode)
        assert model.adam == mode and isinstance(model._optimizer, torch.optim.Adam)
        before = model.mean.detach().clone()
        model.mean.grad = torch.ones_like(model.mean)
        model.train_step(visible=torch.zeros(6, dtype=torch.bool))  # ignored
        assert model.mean.grad is None and not torch.equal(model.mean.detach(), before)
    with pytest.raises(RuntimeError):  # the fused step has no CPU path
        p = torch.zeros(4, 3, requires_grad=True)
        p.grad = torch.ones(4, 3)
        gm.HipAdam([{"params": p, "lr": 0.1}], fused=True).step()
