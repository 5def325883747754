"""Float splat centres, covariance dilation and colour clamp (gcp_splat_*, csrc/gcp_splat.hip) without a GPU: argument
validation, which returns before any HIP call, the register / scratch report of every kernel of the file, and the Python
layer's refusals."""
import math
import re
import subprocess

import pytest
import torch

N = None  # a NULL pointer
TILE_LOGIT = math.log(0.04 / 0.96)


def _forward(lib, n_gauss=0, sh_degree=2, n_basis=9, sh_frame=0, cov_eps=0.3, mean_offset=0.5, clamp_colour=1):
    return lib.gcp_splat_forward(*[N] * 7, n_gauss, sh_degree, n_basis, sh_frame, 16, 16, 1.0, cov_eps, mean_offset, clamp_colour, *[N] * 5)


def _backward(lib, n_gauss=0, sh_degree=2, n_basis=9, sh_frame=0, cov_eps=0.3, clamp_colour=1):
    return lib.gcp_splat_backward(*[N] * 7, n_gauss, sh_degree, n_basis, sh_frame, *[N] * 5, cov_eps, clamp_colour, *[N] * 7)


def test_abi_version_is_unchanged_and_the_entry_points_are_bound():
    from simplegaussiansplat_tk71_amd import _lib

    lib = _lib.load()
    assert lib.gcp_abi_version() == _lib.ABI_VERSION == 4
    for name in ("gcp_splat_forward", "gcp_splat_gather", "gcp_splat_backward"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


@pytest.mark.parametrize("call", [_forward, _backward], ids=["forward", "backward"])
def test_forward_and_backward_validate_before_any_hip_call(call):
    from simplegaussiansplat_tk71_amd import _lib

    lib = _lib.load()
    assert call(lib) == 0  # no Gaussians: a no-op after the checks
    assert call(lib, cov_eps=0.0, clamp_colour=0) == 0
    for frame in (0, 1):
        assert call(lib, sh_degree=3, n_basis=16, sh_frame=frame) == 0
        assert call(lib, sh_degree=4, n_basis=25, sh_frame=frame) == 1
        assert call(lib, sh_degree=3, n_basis=15, sh_frame=frame) == 1
    assert call(lib, sh_degree=-1) == 1
    assert call(lib, sh_frame=2) == 1 and call(lib, sh_frame=-1) == 1
    for bad in (-1e-6, float("nan"), float("inf"), -float("inf")):
        assert call(lib, cov_eps=bad) == 1, bad
    for bad in (2, -1):
        assert call(lib, clamp_colour=bad) == 1, bad
    assert call(lib, n_gauss=-1) == 1
    assert call(lib, n_gauss=4) == 1  # NULL arrays with Gaussians to project


def test_forward_rejects_a_mean_offset_that_is_not_finite():
    from simplegaussiansplat_tk71_amd import _lib

    lib = _lib.load()
    assert _forward(lib, mean_offset=0.0) == 0 and _forward(lib, mean_offset=-0.5) == 0
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert _forward(lib, mean_offset=bad) == 1, bad


def test_gather_validates_pointers_and_alignment_before_any_hip_call():
    import ctypes

    from simplegaussiansplat_tk71_amd import _lib

    lib = _lib.load()
    assert lib.gcp_splat_gather(N, N, 0, *[N] * 12) == 0  # nothing kept: a no-op
    assert lib.gcp_splat_gather(N, N, -1, *[N] * 12) == 1
    assert lib.gcp_splat_gather(N, N, 4, *[N] * 12) == 1
    # host memory stands in for the arrays: every call below must return before anything would read it
    buf = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(buf) + 63) & ~63

    def gather(record=0, mean_xy=0, vinv=0, depth=True):
        p = [base + 256 * k for k in range(12)]  # record perm | start end mean boxsize vinv alpha l_d depth index row_of
        p[0] += record
        p[4] += mean_xy
        p[6] += vinv
        return lib.gcp_splat_gather(p[0], p[1], 4, p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9] if depth else None, p[10], p[11], None, None)

    assert gather(record=4) == 1 and gather(record=8) == 1
    assert gather(vinv=8) == 1
    assert gather(mean_xy=4) == 1
    for missing in range(12):
        if missing == 9:
            continue  # depth may be NULL
        p = [base + 256 * k for k in range(12)]
        p[missing] = None
        assert lib.gcp_splat_gather(p[0], p[1], 4, *p[2:], None, None) == 1, missing


def test_splat_kernels_hold_their_occupancy_without_scratch(tmp_path):
    """The bounds of tests/test_sh3_cabi.py for the kernels of gcp_project.hip, on those of gcp_splat.hip: the same staging
    (37 888 B of LDS at 9 coefficients: four blocks per CU, <= 128 VGPRs; 59 392 B at 16: two blocks, <= 256), no scratch, no
    spills.  None of the kernels may carry `k_project` in its name: the census tests of that file count those."""
    from simplegaussiansplat_tk71_amd import _build

    src = [s for s in _build.SRCS if s.endswith("gcp_splat.hip")][0]
    assert any(h.endswith("gcp_project.hpp") for h in _build.HDRS)  # the source hash covers the shared device code
    out = tmp_path / "splat.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    res = subprocess.run([_build.find_hipcc(), *flags, "-I", _build.INCLUDE, "-S", "--cuda-device-only", "-o", str(out), src],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", out.read_text())
    report = {name: (int(scratch), int(vgpr), int(spills)) for name, scratch, vgpr, spills in kernels}
    print(report)
    assert not [k for k in report if "k_project" in k]
    assert all("k_splat" in k for k in report)
    # template arguments in the mangled name: I Li<MAXDEG>E Lb<WORLD>E E
    degree3 = sorted(k for k in report if re.search(r"k_splat_(fwd|bwd)ILi3E", k))
    degree2 = sorted(k for k in report if k not in degree3)
    assert len(degree3) == 2 + 2, degree3        # fwd, bwd x 2 frames
    assert len(degree2) == 2 + 2 + 1, degree2    # fwd, bwd x 2 frames, the gather
    assert sum("k_splat_fwd" in k for k in report) == 4 and sum("k_splat_bwd" in k for k in report) == 4
    assert sum("k_splat_gather" in k for k in report) == 1
    for k, (scratch, vgpr, spills) in report.items():
        assert scratch == 0 and spills == 0, (k, scratch, spills)
    for k in degree2:
        assert report[k][1] <= 128, (k, report[k])
    for k in degree3:
        assert report[k][1] <= 256, (k, report[k])


def _cpu_world(n=8):
    g = torch.Generator().manual_seed(0)
    P = torch.eye(3, 4)[None].clone()
    P[0, 2, 3] = 3.0
    K = torch.tensor([[[30.0, 0.0, 16.0], [0.0, 30.0, 12.0], [0.0, 0.0, 1.0]]])
    return [torch.randn(n, 3, generator=g), torch.randn(n, 4, generator=g), torch.zeros(n, 3) - 3, torch.zeros(n, 1), torch.zeros(n, 9, 3)], P, K


@pytest.mark.parametrize("options", [{"centres": "subpixel"}, {"cov_dilation": 0.3}, {"clamp_colour": True}], ids=lambda o: next(iter(o)))
def test_cpu_tensors_are_rejected(options):
    from simplegaussiansplat_tk71_amd import gs_model as gm

    args, P, K = _cpu_world()
    with pytest.raises(RuntimeError, match="no CPU path"):
        gm.camera_inputs(*args, P, K, [[32, 24]], TILE_LOGIT, **options)


@pytest.mark.parametrize("options", [{"centres": "float"}, {"centres": None}, {"cov_dilation": -0.1}, {"cov_dilation": float("nan")},
                                     {"cov_dilation": float("inf")}, {"cov_dilation": "0.3"}, {"clamp_colour": 1}],
                         ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_bad_options_raise_value_error_before_anything_touches_the_gpu(options):
    """CPU tensors: a call that got as far as the projection would raise RuntimeError ("no CPU path") instead."""
    from simplegaussiansplat_tk71_amd import gs_model as gm

    args, P, K = _cpu_world()
    with pytest.raises(ValueError):
        gm.camera_inputs(*args, P, K, [[32, 24]], TILE_LOGIT, **options)
    with pytest.raises(ValueError):
        gm.GS_model_with_param(*args[:4], **options)


def test_model_stores_the_options_and_from_ply_passes_them_through(tmp_path):
    from simplegaussiansplat_tk71_amd import gs_model as gm

    args, _, _ = _cpu_world()
    model = gm.GS_model_with_param(*args[:4])
    assert (model.centres, model.cov_dilation, model.clamp_colour) == ("pixel", None, False)
    model = gm.GS_model_with_param(*args[:4], centres="subpixel", cov_dilation=0.3, clamp_colour=True, sh_frame="world")
    assert (model.centres, model.cov_dilation, model.clamp_colour) == ("subpixel", 0.3, True)
    path = tmp_path / "scene.ply"
    model.save_ply(path, convention="raw")
    back = gm.GS_model_with_param.from_ply(path, "cpu", convention="raw", sh_frame="world", centres="subpixel", cov_dilation=0.3)
    assert (back.centres, back.cov_dilation, back.clamp_colour) == ("subpixel", 0.3, False)
