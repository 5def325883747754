"""The absolute screen-space gradient (gcp_blend_absgrad / gcp_blend_absgrad_depth, csrc/gcp_absgrad.hip) without a GPU: the
entry points are declared, exported and bound under the unchanged ABI version, their argument validation returns before any
HIP call, the option `screen_grad` defaults to "signed" and refuses what it cannot serve, and the kernels compile without
scratch or spills at the occupancy of the blend backward or better."""
import ctypes
import inspect
import math
import re
import subprocess

import pytest
import torch

N = None  # a NULL pointer
NAMES = ("gcp_blend_absgrad_workspace_bytes", "gcp_blend_absgrad", "gcp_blend_absgrad_depth")
OK, INVALID, WORKSPACE = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from simplegaussiansplat_tk71_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def host():
    """Host memory standing in for device arrays: every call that gets it must return before anything would read it."""
    buf = ctypes.create_string_buffer(8192)
    base = (ctypes.addressof(buf) + 63) & ~63
    return buf, [base + 256 * k for k in range(20)]


def test_abi_version_is_unchanged_and_the_entry_points_are_declared_exported_and_bound(lib):
    from simplegaussiansplat_tk71_amd import _build, _lib

    assert lib.gcp_abi_version() == _lib.ABI_VERSION == 4
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert any(s.endswith("gcp_absgrad.hip") for s in _build.SRCS)
    with open(_build.INCLUDE + "/grouped_cumprod_hip.h") as f:
        header = f.read()
    assert re.search(r"#define GCP_ABI_VERSION 4\b", header)
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name  # declared, and (hasattr above: dlsym found it) exported


def test_workspace_size(lib):
    for k in (-5, 0, 1, 31, 32, 33, 1000, 10 ** 6 + 7):
        b = lib.gcp_blend_absgrad_workspace_bytes(k)
        assert b % 256 == 0 and b >= 8 * max(k, 0) and b > 0, k
    assert lib.gcp_blend_absgrad_workspace_bytes(10 ** 6) < 8 * 10 ** 6 + 256


# start end mean vinv opacity l_d | tile_off tile_start tile_list t_ckpt grad_image | absgrad ws
def _colour(lib, p, n=4, width=31, height=23, k=6, ptrs=None, ws_bytes=4096):
    a = list(p[:13]) if ptrs is None else ptrs
    return lib.gcp_blend_absgrad(a[0], a[1], a[2], a[3], a[4], a[5], n, width, height, a[6], k, a[7], a[8], a[9], a[10], a[11], a[12],
                                 ws_bytes, None)


# start end mean vinv opacity l_d depth | tile_off tile_start tile_list t_ckpt grad_image | absgrad ws | background grad_depth grad_alpha
def _depth(lib, p, n=4, width=31, height=23, k=6, ptrs=None, ws_bytes=4096):
    a = list(p[:17]) if ptrs is None else ptrs
    return lib.gcp_blend_absgrad_depth(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[14], n, width, height, a[7], k, a[8], a[9], a[10], a[11],
                                       a[15], a[16], a[12], a[13], ws_bytes, None)


@pytest.mark.parametrize("call, required", [(_colour, 13), (_depth, 14)], ids=["colour", "depth"])
def test_absgrad_validates_before_any_hip_call(lib, host, call, required):
    p = host[1]
    total = 13 if call is _colour else 17
    tile_list = 8 if call is _colour else 9
    assert call(lib, p, n=0, ptrs=[N] * total, ws_bytes=0) == OK  # no Gaussians: a no-op
    assert call(lib, p, n=0) == OK
    for bad in ({"n": -1}, {"k": -1}, {"width": -1}, {"height": -1}, {"n": 0, "k": -1}, {"k": 2 ** 31}):
        assert call(lib, p, **bad) == INVALID, bad
    assert call(lib, p, n=-1, ptrs=[N] * total) == INVALID
    for missing in range(required):
        a = list(p[:total])
        a[missing] = N
        assert call(lib, p, ptrs=a) == INVALID, missing
    a = list(p[:total])
    a[tile_list] = N  # the tile list: not needed where there is no entry — but then the call would launch: a short workspace answers first
    assert call(lib, p, k=0, ptrs=a, ws_bytes=0) == WORKSPACE
    if call is _depth:  # background, grad_depth and grad_alpha may be NULL: such a call gets as far as the workspace check
        a = list(p[:total])
        a[14] = a[15] = a[16] = N
        assert call(lib, p, ptrs=a, ws_bytes=0) == WORKSPACE
    need = lib.gcp_blend_absgrad_workspace_bytes(6)
    assert call(lib, p, ws_bytes=need - 1) == WORKSPACE and call(lib, p, ws_bytes=0) == WORKSPACE
    assert call(lib, p, k=1000, ws_bytes=lib.gcp_blend_absgrad_workspace_bytes(1000) - 256) == WORKSPACE


def test_python_layers_export_the_new_names_and_refuse_cpu_tensors():
    import cuda_kernel as ck
    from simplegaussiansplat_tk71_amd import raster

    assert "absgrad_buffer" in ck.__all__ and callable(ck.absgrad_buffer)
    for fn, name in ((ck.render, "absgrad"), (raster.blend_absgrad, "grad_image"), (raster.blend_absgrad_depth, "background")):
        assert name in inspect.signature(fn).parameters
    assert inspect.signature(ck.render).parameters["absgrad"].default is None
    z = torch.zeros(3, 2, dtype=torch.int32)
    buf = ck.absgrad_buffer(z)
    assert buf.shape == (3, 2) and buf.dtype == torch.float32 and not buf.any()
    with pytest.raises(RuntimeError, match="no CPU path"):
        raster.blend_absgrad(None, z, z, z, torch.zeros(3, 2, 2), torch.zeros(3, 1), torch.zeros(3, 3), torch.zeros(8), torch.zeros(9, 9, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        raster.blend_absgrad_depth(None, z, z, z, torch.zeros(3, 2, 2), torch.zeros(3, 1), torch.zeros(3, 3), torch.zeros(3), torch.zeros(8), None)


def _cpu_model(n=5, **kw):
    from simplegaussiansplat_tk71_amd import gs_model as gm

    q = torch.zeros(n, 4)
    q[:, 3] = 1
    return gm.GS_model_with_param(torch.randn(n, 3), q, torch.full((n, 3), math.log(0.05)), torch.zeros(n, 1), **kw)


def test_screen_grad_defaults_and_refusals():
    from examples.train_cameras import train
    from simplegaussiansplat_tk71_amd import density
    from simplegaussiansplat_tk71_amd import gs_model as gm

    assert inspect.signature(gm.GS_model_with_param.__init__).parameters["screen_grad"].default == "signed"
    assert inspect.signature(train).parameters["screen_grad"].default == "signed"
    assert gm.DENSIFY_ON == density.DENSIFY_ON == ("position", "screen")
    assert gm.SCREEN_GRADS is density.SCREEN_GRADS and density.SCREEN_GRADS == ("signed", "abs")
    assert _cpu_model().screen_grad == "signed"
    assert _cpu_model(densify_on="screen", centres="subpixel", screen_grad="abs").screen_grad == "abs"
    with pytest.raises(ValueError, match="densify_on='screen'"):
        _cpu_model(screen_grad="abs")  # densify_on="position"
    with pytest.raises(ValueError, match="densify_on='screen'"):
        _cpu_model(screen_grad="abs", densify_on="position", centres="subpixel")
    with pytest.raises(ValueError, match="centres='subpixel'"):
        _cpu_model(screen_grad="abs", densify_on="screen", centres="pixel")
    for bad in ("absolute", "ABS", None, 1):
        with pytest.raises(ValueError, match="screen_grad"):
            _cpu_model(densify_on="screen", centres="subpixel", screen_grad=bad)
    with pytest.raises(ValueError, match="screen_grad"):
        train(torch.zeros(4, 3), torch.zeros(1, 3, 4), torch.eye(3)[None], torch.tensor([[16, 16]]), None, centres="subpixel",
              densify_on="screen", screen_grad="both")


def test_from_ply_passes_the_option_through(tmp_path):
    from simplegaussiansplat_tk71_amd import gs_model as gm

    path = str(tmp_path / "scene.ply")
    _cpu_model(sh_frame="world").save_ply(path)
    model = gm.GS_model_with_param.from_ply(path, centres="subpixel", densify_on="screen", screen_grad="abs")
    assert model.screen_grad == "abs" and model.densify_on == "screen"
    assert gm.GS_model_with_param.from_ply(path).screen_grad == "signed"
    with pytest.raises(ValueError, match="densify_on='screen'"):
        gm.GS_model_with_param.from_ply(path, screen_grad="abs")


def test_absgrad_kernels_use_no_scratch(tmp_path):
    """k_absgrad_tile / k_absgrad_tile_depth at the occupancy of k_blend_bwd or better (<= 80 VGPRs: six waves per SIMD, the
    bar tests/test_cabi.py sets for the blend kernels; measured 44 / 44: eight), k_absgrad_reduce at eight (<= 64; measured
    22).  No scratch, no spills."""
    from simplegaussiansplat_tk71_amd import _build

    src = [s for s in _build.SRCS if s.endswith("gcp_absgrad.hip")][0]
    out = tmp_path / "absgrad.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    res = subprocess.run([_build.find_hipcc(), *flags, "-I", _build.INCLUDE, "-S", "--cuda-device-only", "-o", str(out), src],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", out.read_text())
    report = {name: (int(scratch), int(vgpr), int(spills)) for name, scratch, vgpr, spills in kernels}
    print(report)
    assert len(report) == 3 and all("k_absgrad_" in k for k in report)
    for frag in ("k_blend_fwd", "k_blend_bwd", "k_grad_reduce", "k_contrib"):  # other tests count kernels by these names
        assert not any(frag in k for k in report), frag
    for frag, cap in (("k_absgrad_tileE", 80), ("k_absgrad_tile_depth", 80), ("k_absgrad_reduce", 64)):
        found = [k for k in report if frag in k]
        assert len(found) == 1, frag
        scratch, vgpr, spills = report[found[0]]
        assert scratch == 0 and spills == 0 and vgpr <= cap, (found[0], scratch, vgpr, spills)
