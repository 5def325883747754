"""Held-out evaluation without a GPU: gcp_image_metrics (csrc/gcp_loss.hip) is bound and declared and validates before any
HIP call — only scalars, NULL pointers and the real host window are passed —, `split_cameras` follows the llffhold
convention, the example's new arguments default to off, and two gloo ranks gather their shares of a metrics vector."""
import inspect
import os
import re
import socket

import pytest
import torch

OK, INVALID = 0, 1  # GCP_OK, GCP_ERR_INVALID_ARGUMENT
N = None  # a NULL pointer


@pytest.fixture(scope="module")
def lib():
    from simplegaussiansplat_tk71_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def window():
    from simplegaussiansplat_tk71_amd import loss

    return loss._host_window(11, 1.5)  # host memory: the entry point copies it into the kernel arguments


def test_the_entry_point_is_bound_and_declared(lib):
    from simplegaussiansplat_tk71_amd import _build, _lib

    with open(_build.INCLUDE + "/grouped_cumprod_hip.h") as f:
        header = f.read()
    assert "gcp_image_metrics" in _lib.SIGNATURES and hasattr(lib, "gcp_image_metrics")
    assert re.search(r"\bgcp_image_metrics\(", header)
    assert re.search(r"^#define GCP_METRICS_CLAMP 1$", header, re.M) and _lib.METRICS_CLAMP == 1
    assert lib.gcp_abi_version() == _lib.ABI_VERSION == 4  # a new symbol, nothing existing changed


def test_image_metrics_validates_before_any_hip_call(lib, window):
    def call(images=0, channels=3, height=16, width=32, win=window, flags=0):
        return lib.gcp_image_metrics(N, N, images, channels, height, width, win, 1e-4, 9e-4, flags, N, N, N)

    assert call() == OK and call(flags=1) == OK  # no image: a no-op, NULL arrays allowed
    assert call(height=6, width=6) == OK and call(height=39, width=71, channels=1) == OK
    for images in (-1, -(2 ** 40)):
        assert call(images=images) == INVALID, images
    for channels in (0, -1, -(2 ** 31)):
        assert call(channels=channels) == INVALID and call(images=2, channels=channels) == INVALID, channels
    for small in (5, 1, 0, -1, -(2 ** 31)):  # smaller than the reflection of an 11-tap window needs
        assert call(height=small) == INVALID and call(width=small) == INVALID and call(height=small, width=small) == INVALID, small
    assert call(win=N) == INVALID and call(images=3, win=N) == INVALID
    for flags in (2, 3, 4, -1, 2 ** 30, -(2 ** 31)):  # an unknown bit, with and without the known one
        assert call(flags=flags) == INVALID and call(images=1, flags=flags) == INVALID, flags
    for images in (1, 3, 2 ** 20):  # NULL arrays with images to read
        assert call(images=images) == INVALID and call(images=images, flags=1) == INVALID, images
        assert call(images=images, height=6, width=6) == INVALID
    # more than 2^31 - 1 blocks: by the image count alone, by images x channels, by planes x tiles
    assert call(images=2 ** 40) == INVALID and call(images=2 ** 62, channels=2 ** 30) == INVALID
    assert call(images=2 ** 30, channels=3, height=6, width=6) == INVALID
    assert call(images=2 ** 20, channels=3, height=1080, width=1920) == INVALID


def test_image_metrics_and_evaluate_refuse_cpu_tensors():
    from simplegaussiansplat_tk71_amd import gs_model as gm

    a = torch.rand(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gm.image_metrics(a, a)
    assert gm.ImageMetrics._fields == ("mse", "l1", "ssim", "psnr")


def test_split_cameras_follows_the_llffhold_convention():
    from simplegaussiansplat_tk71_amd.gs_model import split_cameras

    names = ["c.png", "a.png", "e.png", "b.png", "d.png", "j.png", "f.png", "i.png", "g.png", "h.png"]  # unsorted
    by_name = sorted(range(10), key=lambda i: names[i])
    for every in (0, 1, 3, 8, 10, 11, 1000):
        train, test = split_cameras(names, every)
        assert isinstance(train, list) and isinstance(test, list)
        assert not set(train) & set(test) and sorted(train + test) == list(range(10)), every  # disjoint, cover the list
        want = [j for i, j in enumerate(by_name) if every and i % every == 0]
        assert test == want, every
        assert train == [j for j in by_name if j not in want], every
    assert split_cameras(names, 0) == (by_name, [])
    assert split_cameras(names, 1) == ([], by_name)
    assert split_cameras(names, 8)[1] == [names.index("a.png"), names.index("i.png")]
    assert split_cameras(names, 11)[1] == [names.index("a.png")]  # larger than the list: the first camera alone
    assert split_cameras(names)[1] == split_cameras(names, 8)[1]  # the default
    assert split_cameras([], 8) == ([], [])
    assert split_cameras(list(range(8)), 4) == ([1, 2, 3, 5, 6, 7], [0, 4])
    with pytest.raises(ValueError):
        split_cameras(names, -1)


def test_the_example_keeps_evaluation_off_by_default():
    from examples import train_cameras

    params = inspect.signature(train_cameras.train).parameters
    assert params["test_every"].default == 0 and params["eval_every"].default == 0 and params["evals"].default is None
    with open(train_cameras.__file__) as f:
        text = f.read()
    for flag in ("--test-every", "--eval-every", "--eval-json"):
        assert flag in text, flag


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


TOTAL = 7


def _whole():
    from simplegaussiansplat_tk71_amd import gs_model as gm

    g = torch.Generator().manual_seed(11)
    mse = torch.rand(TOTAL, generator=g, dtype=torch.float64) * 1e-2
    mse[3] = 0.0  # an image identical to its target: psnr inf
    return gm.ImageMetrics(mse, torch.rand(TOTAL, generator=g, dtype=torch.float64), torch.rand(TOTAL, generator=g, dtype=torch.float64),
                           gm.psnr_from_mse(mse))


def _gather_worker(rank, world, port, q):
    import torch.distributed as dist

    from simplegaussiansplat_tk71_amd import gs_model as gm

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        index = list(range(TOTAL))[rank::world]
        share = gm.ImageMetrics(*(t[index] for t in _whole()))
        out = gm.gather_metrics(share, index, TOTAL)
        q.put((rank, [t.clone() for t in out]))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_two_rank_gloo_gather_equals_the_concatenation():
    import torch.multiprocessing as mp

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    got = [q.get(timeout=150) for _ in range(world)]
    for pr in procs:
        pr.join(60)
        assert pr.exitcode == 0
    want = _whole()
    assert want.psnr[3].item() == float("inf")
    for rank, fields in got:
        for name, have, expect in zip(want._fields, fields, want):
            assert have.dtype == torch.float64 and have.shape == (TOTAL,), (rank, name)
            assert torch.equal(have, expect), (rank, name)  # bit for bit: every image was measured by one rank
