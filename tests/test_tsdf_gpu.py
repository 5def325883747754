"""TSDF integration (csrc/gcp_tsdf.hip: k_tsdf_integrate, mesh.TSDFVolume) on the GPU against the float64 statements of
tests/mesh_ref.py, on the inputs of tests/mesh_cases.py: three ring cameras at 24 x 16, analytic maps of a sphere, volumes of
nz x ny x nx = 5 x 7 x 13 (two blocks of 256 lattice points, the second partial) and 2 x 3 x 70 (rows longer than a wave).
weight is compared exactly; tsdf and rgb within 1e-5 max(1, (|d| + |z|) / trunc): the project's 1e-5 on the condition scale of
the subtraction d - z divided by trunc.  A lattice point at which a float64 decision of some camera is marginal (mesh_ref.
integrate) is left out; tests/test_mesh_cabi.py holds that to at most 1 % per case.  The kernel has no grid cap: one thread per
lattice point, so there is no stride loop to cover."""
import pytest
import torch

from tests import mesh_cases as mc

pytestmark = pytest.mark.gpu


def fused(case, device, split=None):
    """The case's cameras integrated into a fresh volume: all in one launch (split None) or in the given groups."""
    from simplegaussiansplat_tk71_amd.mesh import TSDFVolume

    inp = mc.tsdf_inputs(case)
    vol = TSDFVolume(case["origin"], case["voxel"], case["dims"], case["trunc"], device, colour=case["colour"])
    depth, alpha, image, P, K = (inp[k].to(device) for k in ("depth", "alpha", "image", "P", "K"))
    for lo, hi in split or [(0, depth.shape[0])]:
        vol.integrate(depth[lo:hi], alpha[lo:hi], P[lo:hi], K[lo:hi], image=image[lo:hi] if case["colour"] else None,
                      alpha_min=mc.ALPHA_MIN, depth_max=case["depth_max"])
    torch.cuda.synchronize(device)
    return vol


@pytest.mark.parametrize("case", mc.TSDF_CASES, ids=lambda c: c["id"])
def test_integration_against_float64(device, case):
    vol = fused(case, device)
    (tsdf, weight, rgb), marginal, scale = mc.tsdf_reference(case)
    keep = ~marginal
    assert keep.double().mean().item() >= 0.99
    nx, ny, nz = case["dims"]
    assert vol.tsdf.shape == vol.weight.shape == (nz, ny, nx) and vol.tsdf.dtype == torch.float32
    got_w, got_f = vol.weight.cpu().double(), vol.tsdf.cpu().double()
    assert torch.equal(got_w[keep], weight[keep])
    err = ((got_f - tsdf).abs() / scale)[keep].max().item()
    print(f"{case['id']}: tsdf error / scale {err:.3e}, largest scale {scale.max().item():.1f}, left out {int(marginal.sum())}")
    assert err <= 1e-5
    assert torch.equal(got_f[keep & (weight == 0)], torch.ones_like(got_f)[keep & (weight == 0)])  # untouched points stay fresh
    if case["colour"]:
        err = ((vol.rgb.cpu().double() - rgb).abs() / scale)[:, keep].max().item()
        print(f"{case['id']}: rgb error / scale {err:.3e}")
        assert err <= 1e-5
    else:
        assert vol.rgb is None
    if case.get("expect_behind"):  # the float-before-int comparison: points behind camera 0 and points with 0 < z < 1e-4
        inp = mc.tsdf_inputs(case)
        assert inp["behind"] > 0 and inp["grazing"] > 0 and not marginal.any()
        assert torch.equal(got_w, weight)


@pytest.mark.parametrize("case", mc.TSDF_CASES[:2], ids=lambda c: c["id"])
def test_any_split_of_the_cameras_gives_the_same_bits(device, case):
    whole = fused(case, device)
    for split in ([(0, 1), (1, 2), (2, 3)], [(0, 2), (2, 3)], None):
        other = fused(case, device, split)
        assert torch.equal(other.tsdf, whole.tsdf) and torch.equal(other.weight, whole.weight) and torch.equal(other.rgb, whole.rgb)


def test_no_camera_and_reset(device):
    case = mc.TSDF_CASES[0]
    vol = fused(case, device)
    before = (vol.tsdf.clone(), vol.weight.clone(), vol.rgb.clone())
    empty = torch.zeros(0, 1, mc.HEIGHT, mc.WIDTH, device=device)
    vol.integrate(empty, empty, torch.zeros(0, 3, 4, device=device), torch.zeros(0, 3, 3, device=device),
                  image=torch.zeros(0, 3, mc.HEIGHT, mc.WIDTH, device=device))
    assert all(torch.equal(a, b) for a, b in zip(before, (vol.tsdf, vol.weight, vol.rgb)))
    inp = mc.tsdf_inputs(case)
    blank = torch.zeros(1, 1, mc.HEIGHT, mc.WIDTH, device=device)  # a camera that sees nothing: alpha = 0 everywhere
    vol.integrate(blank, blank, inp["P"][:1].to(device), inp["K"][:1].to(device), image=torch.zeros(1, 3, mc.HEIGHT, mc.WIDTH, device=device))
    assert all(torch.equal(a, b) for a, b in zip(before, (vol.tsdf, vol.weight, vol.rgb)))
    with pytest.raises(RuntimeError, match="colour volume needs image"):
        vol.integrate(blank, blank, inp["P"][:1].to(device), inp["K"][:1].to(device))
    with pytest.raises(RuntimeError, match="must live on"):
        vol.integrate(blank, blank, inp["P"][:1], inp["K"][:1].to(device), image=torch.zeros(1, 3, mc.HEIGHT, mc.WIDTH, device=device))
    vol.reset()
    assert bool((vol.tsdf == 1).all()) and bool((vol.weight == 0).all()) and bool((vol.rgb == 0).all())


def test_integration_is_capturable(device):
    """No device->host read, no allocation: the launch records into a HIP graph and replays to the same bits."""
    from simplegaussiansplat_tk71_amd.mesh import TSDFVolume

    case = mc.TSDF_CASES[0]
    whole = fused(case, device)
    inp = mc.tsdf_inputs(case)
    depth, alpha, image, P, K = (inp[k].to(device).contiguous() for k in ("depth", "alpha", "image", "P", "K"))
    vol = TSDFVolume(case["origin"], case["voxel"], case["dims"], case["trunc"], device)
    stream = torch.cuda.Stream(device)
    stream.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(stream):
        vol.integrate(depth, alpha, P, K, image=image, alpha_min=mc.ALPHA_MIN)  # warm-up outside the capture
    torch.cuda.current_stream(device).wait_stream(stream)
    vol.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        vol.integrate(depth, alpha, P, K, image=image, alpha_min=mc.ALPHA_MIN)
    vol.reset()
    graph.replay()
    torch.cuda.synchronize(device)
    assert torch.equal(vol.tsdf, whole.tsdf) and torch.equal(vol.weight, whole.weight) and torch.equal(vol.rgb, whole.rgb)
