"""Degree-3 SH and the world-frame entry points of the projection (gcp_project_*, csrc/gcp_project.hip) without a GPU:
argument validation, which returns before any HIP call, and the register / scratch report of every projection kernel."""
import re
import subprocess

N = None  # a NULL pointer


def _forward(lib, n_gauss, sh_degree, n_basis):
    return lib.gcp_project_forward(*[N] * 7, n_gauss, sh_degree, n_basis, 16, 16, 1.0, *[N] * 5)


def _forward_sh(lib, n_gauss, sh_degree, n_basis, sh_frame):
    return lib.gcp_project_forward_sh(*[N] * 7, n_gauss, sh_degree, n_basis, sh_frame, 16, 16, 1.0, *[N] * 5)


def test_forward_accepts_degree_3_and_validates_before_any_hip_call():
    from simplegaussiansplat_tk71_amd import _lib

    lib = _lib.load()
    assert _forward(lib, 0, 3, 16) == 0  # degree 3 with its 16 coefficients: nothing to do for no Gaussians
    assert _forward(lib, 0, 4, 25) == 1
    assert _forward(lib, 0, 3, 15) == 1
    assert _forward(lib, 0, -1, 16) == 1
    assert _forward(lib, 0, 1, 16) == 0  # the active degree may be below what is stored
    for frame in (0, 1):
        assert _forward_sh(lib, 0, 3, 16, frame) == 0
        assert _forward_sh(lib, 0, 4, 25, frame) == 1
        assert _forward_sh(lib, 0, 3, 15, frame) == 1
    assert _forward_sh(lib, 0, 3, 16, 2) == 1
    assert _forward_sh(lib, 0, 3, 16, -1) == 1
    assert _forward_sh(lib, 4, 3, 16, 1) == 1  # NULL arrays with Gaussians to project


def test_backward_accepts_degree_3_and_validates_before_any_hip_call():
    from simplegaussiansplat_tk71_amd import _lib

    lib = _lib.load()

    def plain(sh_degree, n_basis, n_gauss=0):
        return lib.gcp_project_backward(*[N] * 7, n_gauss, sh_degree, n_basis, *[N] * 10)

    def depth(sh_degree, n_basis, n_gauss=0):
        return lib.gcp_project_backward_depth(*[N] * 7, n_gauss, sh_degree, n_basis, *[N] * 11)

    def framed(sh_degree, n_basis, sh_frame, n_gauss=0):
        return lib.gcp_project_backward_sh(*[N] * 7, n_gauss, sh_degree, n_basis, sh_frame, *[N] * 11)

    for call in (plain, depth, lambda d, nb, n=0: framed(d, nb, 0, n), lambda d, nb, n=0: framed(d, nb, 1, n)):
        assert call(3, 16) == 0
        assert call(4, 25) == 1
        assert call(3, 15) == 1
        assert call(3, 16, 4) == 1  # NULL arrays
    assert framed(3, 16, 2) == 1
    assert framed(2, 9, -1) == 1


def test_projection_kernels_hold_their_occupancy_without_scratch(tmp_path):
    """A 256-thread block stages 10 + 3 n_basis floats per Gaussian in LDS: 37 888 B at 9 coefficients, four blocks per CU =
    4 waves per SIMD, which 128 VGPRs allow; 59 392 B at 16, two blocks = 2 waves per SIMD whatever the register count, so
    up to 256 VGPRs cost nothing.  Instantiations a degree <= 2 call launches: k_project_fwd, k_project_bwd,
    k_project_bwd_depth (camera frame), k_project_fwd_sh<2, true>, k_project_bwd_sh<2, true, *> (world frame), and the two
    gathers.  Degree 3: k_project_fwd_sh<3, *>, k_project_bwd_sh<3, *, *>.  None may use scratch or spill."""
    from simplegaussiansplat_tk71_amd import _build

    src = [s for s in _build.SRCS if s.endswith("gcp_project.hip")][0]
    out = tmp_path / "project.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    res = subprocess.run([_build.find_hipcc(), *flags, "-I", _build.INCLUDE, "-S", "--cuda-device-only", "-o", str(out), src],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    kernels = re.findall(r"\.name:\s+(\S*k_project\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", out.read_text())
    report = {name: (int(scratch), int(vgpr), int(spills)) for name, scratch, vgpr, spills in kernels}
    # template arguments in the mangled name: I Li<MAXDEG>E Lb<WORLD>E [Lb<DEPTH>E] E
    degree3 = sorted(k for k in report if re.search(r"k_project_(fwd|bwd)_shILi3E", k))
    degree2 = sorted(k for k in report if k not in degree3)
    assert len(degree3) == 2 + 4, degree3          # fwd x 2 frames, bwd x 2 frames x with / without depth
    assert len(degree2) == 5 + 1 + 2, degree2      # fwd, 2 gathers, bwd, bwd_depth | world: fwd | bwd x with / without depth
    assert sum("k_project_fwd_shILi2ELb1E" in k for k in degree2) == 1 and sum("k_project_bwd_shILi2ELb1E" in k for k in degree2) == 2
    print({k: report[k] for k in degree2 + degree3})
    for k, (scratch, vgpr, spills) in report.items():
        assert scratch == 0 and spills == 0, (k, scratch, spills)
    for k in degree2:
        assert report[k][1] <= 128, (k, report[k])
    for k in degree3:
        assert report[k][1] <= 256, (k, report[k])
