"""Density control on the device (gcp_densify_*, csrc/gcp_densify.hip) without a GPU: the entry points are bound, their
argument validation returns before any HIP call, and every kernel of the file compiles without scratch or spills."""
import ctypes
import re
import subprocess

import pytest

N = None  # a NULL pointer
NAMES = ("gcp_densify_accumulate", "gcp_densify_plan_workspace_bytes", "gcp_densify_plan", "gcp_densify_fill", "gcp_densify_rows",
         "gcp_densify_split")
BAD_FLOATS = (float("nan"), float("inf"), -float("inf"))


@pytest.fixture(scope="module")
def lib():
    from simplegaussiansplat_tk71_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def host():
    """Host memory standing in for device arrays: every call that gets it must return before anything would read it."""
    buf = ctypes.create_string_buffer(8192)
    base = (ctypes.addressof(buf) + 63) & ~63
    return buf, [base + 256 * k for k in range(16)]


def test_abi_version_is_unchanged_and_the_entry_points_are_bound(lib):
    from simplegaussiansplat_tk71_amd import _build, _lib

    assert lib.gcp_abi_version() == _lib.ABI_VERSION == 4
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert any(s.endswith("gcp_densify.hip") for s in _build.SRCS)


def test_accumulate_validates_before_any_hip_call(lib, host):
    p = host[1]
    acc = lambda m=4, n=8, sx=1.0, sy=1.0, grad=p[0], index=p[1], norm=p[2], views=p[3], bad=None: lib.gcp_densify_accumulate(  # noqa: E731
        grad, index, m, sx, sy, norm, views, n, bad, None)
    assert acc(m=0, grad=N, index=N, norm=N, views=N) == 0  # an empty list: a no-op
    assert acc(m=-1) == 1 and acc(n=-1) == 1
    for bad in BAD_FLOATS:
        assert acc(sx=bad) == 1 and acc(sy=bad) == 1, bad
    for missing in ("grad", "index", "norm", "views"):
        assert acc(**{missing: N}) == 1, missing
    assert acc(norm=N, views=N) == 1          # the count-only form needs n_bad
    assert acc(index=N, norm=N, views=N, bad=p[4]) == 1
    assert acc(grad=p[0] + 4) == 1            # rows are read as float2


def test_plan_validates_before_any_hip_call(lib, host):
    p = host[1]

    def plan(n=4, thr=0.5, dense=0.1, prune=1.0, min_op=0.005, n_split=2, ptrs=None, ws_bytes=4096):
        a = list(p[:8]) if ptrs is None else ptrs  # norm views log_scale opacity | count action offset ws
        return lib.gcp_densify_plan(a[0], a[1], a[2], a[3], n, thr, dense, prune, min_op, n_split, a[4], a[5], a[6], a[7], ws_bytes, None)

    assert plan(n=-1) == 1
    assert plan(n_split=0) == 1 and plan(n_split=-3) == 1
    for bad in BAD_FLOATS:
        for k in ("thr", "dense", "prune", "min_op"):
            assert plan(**{k: bad}) == 1, (k, bad)
            assert plan(n=0, **{k: bad}) == 1, (k, bad)
    for missing in range(8):
        a = list(p[:8])
        a[missing] = N
        assert plan(ptrs=a) == 1, missing
    assert plan(ws_bytes=0) == 2              # GCP_ERR_WORKSPACE
    # totals that could not fit the int32 prefix sum: refused on the bound n * max(n_split, 2)
    assert plan(n=2 ** 30) == 1 and plan(n=2 ** 29, n_split=5) == 1
    assert lib.gcp_densify_plan_workspace_bytes(0) % 256 == 0 and lib.gcp_densify_plan_workspace_bytes(-5) == lib.gcp_densify_plan_workspace_bytes(0)
    b = lib.gcp_densify_plan_workspace_bytes(1_000_000)
    assert b % 256 == 0 and 4 * (1_000_000 // 2048) <= b < 8192


def test_fill_rows_and_split_validate_before_any_hip_call(lib, host):
    p = host[1]
    fill = lambda n=4, m=6, a=p[0], off=p[1], src=p[2], kind=p[3]: lib.gcp_densify_fill(a, off, n, m, src, kind, None)  # noqa: E731
    assert fill(n=0, a=N, off=N, src=N, kind=N) == 0 and fill(m=0, a=N, off=N, src=N, kind=N) == 0
    assert fill(n=-1) == 1 and fill(m=-1) == 1 and fill(m=2 ** 31) == 1
    for missing in ("a", "off", "src", "kind"):
        assert fill(**{missing: N}) == 1, missing

    rows = lambda n=4, m=6, w=3, mode=0, src=p[0], row=p[1], kind=p[2], dst=p[3]: lib.gcp_densify_rows(  # noqa: E731
        src, n, row, kind, m, w, mode, dst, None)
    assert rows(m=0, src=N, row=N, kind=N, dst=N) == 0 and rows(w=0, src=N, row=N, kind=N, dst=N) == 0
    assert rows(n=-1) == 1 and rows(m=-1) == 1 and rows(w=-1) == 1 and rows(m=2 ** 31) == 1
    assert rows(mode=2) == 1 and rows(mode=-1) == 1
    for missing in ("src", "row", "kind", "dst"):
        assert rows(**{missing: N}) == 1, missing
    assert rows(src=p[0] + 2) == 1 and rows(dst=p[3] + 1) == 1  # floats are 4-byte aligned

    def split(n=4, m=6, n_split=2, ptrs=None):
        a = list(p[:8]) if ptrs is None else ptrs  # mean quat log_scale src_row kind offset | mean_out log_scale_out
        return lib.gcp_densify_split(*a[:6], n, m, n_split, 1, 2, a[6], a[7], None)

    assert split(m=0, ptrs=[N] * 8) == 0 and split(n=0, ptrs=[N] * 8) == 0
    assert split(n=-1) == 1 and split(m=-1) == 1 and split(n_split=0) == 1 and split(m=2 ** 31) == 1
    for missing in range(8):
        a = list(p[:8])
        a[missing] = N
        assert split(ptrs=a) == 1, missing


def test_densify_kernels_use_no_scratch(tmp_path):
    """Streaming kernels at eight waves per SIMD (<= 64 VGPRs): accumulate 18, plan 32, fill 28, the four row gathers 10, the
    split (ten Philox rounds, precise logf / log1pf / sincosf / expf inlined) 45; no scratch, no spills."""
    from simplegaussiansplat_tk71_amd import _build

    src = [s for s in _build.SRCS if s.endswith("gcp_densify.hip")][0]
    out = tmp_path / "densify.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    res = subprocess.run([_build.find_hipcc(), *flags, "-I", _build.INCLUDE, "-S", "--cuda-device-only", "-o", str(out), src],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", out.read_text())
    report = {name: (int(scratch), int(vgpr), int(spills)) for name, scratch, vgpr, spills in kernels}
    print(report)
    assert all("k_densify_" in k for k in report)
    for frag, copies in (("k_densify_accumulate", 1), ("k_densify_plan", 1), ("k_densify_fill", 1), ("k_densify_rows", 4), ("k_densify_split", 1)):
        assert sum(frag in k for k in report) == copies, frag
    for k, (scratch, vgpr, spills) in report.items():
        assert scratch == 0 and spills == 0, (k, scratch, spills)
        assert vgpr <= 64, (k, vgpr)
