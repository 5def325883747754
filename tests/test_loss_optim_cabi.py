"""The loss and Adam entry points (gcp_ssim_*, gcp_adam_step; csrc/gcp_loss.hip, csrc/gcp_optim.hip) without a GPU: their
argument validation returns before any HIP call.  Only scalars, NULL pointers and the real host window are passed: a
check that broke would otherwise launch on whatever address stood in for a device array."""
import pytest

OK, INVALID = 0, 1  # GCP_OK, GCP_ERR_INVALID_ARGUMENT
N = None  # a NULL pointer
NAN, INF = float("nan"), float("inf")

# (height, width) of tests/test_loss_gpu.py: every tile class of k_ssim_l1_bwd (32 x 16 tiles, 5-pixel halo)
SHAPES = [(39, w) for w in (6, 7, 11, 12, 32, 33, 38, 69, 70, 71, 103)] + [(h, 71) for h in (6, 11, 16, 17, 22, 37, 38, 55)] + [(6, 6)]


@pytest.fixture(scope="module")
def lib():
    from simplegaussiansplat_tk71_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def window():
    from simplegaussiansplat_tk71_amd import loss

    return loss._host_window(11, 1.5)  # host memory: the entry points copy it into the kernel arguments


def test_the_entry_points_are_bound_and_declared(lib):
    import re

    from simplegaussiansplat_tk71_amd import _build, _lib

    names = ("gcp_adam_step", "gcp_ssim_blocks", "gcp_ssim_l1_forward", "gcp_ssim_l1_backward")
    with open(_build.INCLUDE + "/grouped_cumprod_hip.h") as f:
        header = f.read()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b%s\(" % name, header), name
    assert lib.gcp_status_string(INVALID) != lib.gcp_status_string(OK)


def test_adam_step_validates_before_any_hip_call(lib):
    def adam(n=0, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
        return lib.gcp_adam_step(N, N, N, N, n, lr, beta1, beta2, eps, step, N)

    assert adam() == OK  # nothing to update: a no-op, NULL tensors allowed
    assert adam(step=30000) == OK and adam(beta1=0.0, beta2=0.0) == OK
    for n in (-1, -(2 ** 40)):
        assert adam(n=n) == INVALID, n
    for step in (0, -1, -(2 ** 40)):
        assert adam(step=step) == INVALID, step
    for bad in (1.0, 1.5, -0.1, -1e-300, INF, -INF, NAN):
        assert adam(beta1=bad) == INVALID and adam(beta2=bad) == INVALID, bad
    for n in (1, 3, 4, 2 ** 24 + 4, 2 ** 40):  # NULL tensors with something to update
        assert adam(n=n) == INVALID, n
        assert adam(n=n, step=0) == INVALID and adam(n=n, beta1=NAN) == INVALID


@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_ssim_l1_validates_before_any_hip_call(lib, window, direction):
    def call(planes=0, height=16, width=16, win=window):
        if direction == "forward":
            return lib.gcp_ssim_l1_forward(N, N, planes, height, width, win, 1e-4, 9e-4, N, N, N, N, N)
        return lib.gcp_ssim_l1_backward(N, N, N, N, N, planes, height, width, win, N, N, N)

    assert call() == OK  # no planes: a no-op, NULL images allowed
    assert call(height=6, width=6) == OK and call(height=39, width=71) == OK
    for planes in (-1, -(2 ** 40)):
        assert call(planes=planes) == INVALID, planes
    for small in (5, 1, 0, -1, -(2 ** 31)):  # smaller than the reflection of an 11-tap window needs
        assert call(height=small) == INVALID and call(width=small) == INVALID and call(height=small, width=small) == INVALID, small
    assert call(win=N) == INVALID and call(planes=3, win=N) == INVALID
    for planes in (1, 3, 2 ** 40):  # NULL images with planes to read
        assert call(planes=planes) == INVALID, planes
        assert call(planes=planes, height=6, width=6) == INVALID


def test_ssim_blocks_counts_rounded_up_tiles_per_plane(lib):
    for h, w in SHAPES:
        tiles = -(-w // 32) * -(-h // 16)
        for planes in (1, 3, 6):
            assert lib.gcp_ssim_blocks(planes, h, w) == planes * tiles, (planes, h, w)
        assert lib.gcp_ssim_blocks(0, h, w) == 0
    assert lib.gcp_ssim_blocks(1, 16, 32) == 1 and lib.gcp_ssim_blocks(1, 17, 33) == 4
    assert lib.gcp_ssim_blocks(2 ** 33, 16, 32) == 2 ** 33  # 64-bit: the launch, not the count, refuses a grid this large
    for planes, h, w in ((-1, 16, 16), (1, 0, 16), (1, 16, 0), (1, -16, 16), (1, 16, -16), (-1, -1, -1), (1, 0, 0)):
        assert lib.gcp_ssim_blocks(planes, h, w) == 0, (planes, h, w)
