"""Occupancy of the backward scan, read from the cross-compiled device code (no GPU), with the technique of
test_bwd_registers.py.

The backward is pinned to four waves per SIMD: four tiles per CU, so that a tile waiting for its group ends leaves three
others' loads in flight.  On gfx950 that is at most 128 registers per lane, VGPRs and AGPRs
together, and the pin only pays without scratch: a kernel that spills to hold 128 is slower than the 146-register one
at three waves.  What keeps it under the bound is the look-back batch of three chunks (five elsewhere); a change that
needs more registers shows up here as scratch, not as a failing functional test."""
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from simplegaussiansplat_tk71_amd import _build

    src = [s for s in _build.SRCS if s.endswith("gcp_scan.hip")][0]
    out = tmp_path_factory.mktemp("scan_occ") / "scan.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    res = subprocess.run([_build.find_hipcc(), *flags, "-I", _build.INCLUDE, "-S", "--cuda-device-only", "-o", str(out), src],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    return out.read_text()


def _scan_kernels(listing):
    """{mangled name: (scratch bytes per lane, VGPRs + AGPRs, spilled VGPRs, spilled SGPRs)} of every gcp_scan_main"""
    kernels = {}
    for block in listing.split("amdhsa.kernels:")[1].split("\n  - ")[1:]:  # one metadata entry per kernel
        field = lambda key: re.search(r"^(?:    )?\.%s:\s+(\S+)" % key, block, re.M).group(1)  # (the entry's own keys, not its args')
        if re.search(r"^    \.name:\s+\S*gcp_scan_main", block, re.M):
            kernels[field("name")] = (int(field("private_segment_fixed_size")), int(field("vgpr_count")) + int(field("agpr_count")),
                                      int(field("vgpr_spill_count")), int(field("sgpr_spill_count")))
    return kernels


def test_backward_holds_four_waves_per_simd_without_scratch(listing):
    kernels = _scan_kernels(listing)
    # gcp_scan_main<MODE, ALIGNED, CARRY, INDEXED, INPLACE>: MODE 2 is the cumprod backward, one kernel per alignment
    bwd = {k: v for k, v in kernels.items() if "gcp_scan_mainILi2E" in k}
    assert len(bwd) == 2, sorted(kernels)
    for name, (scratch, regs, spills, _) in bwd.items():
        print(name, "scratch", scratch, "registers", regs, "spilled VGPRs", spills)
        assert scratch == 0, (name, scratch)
        assert spills == 0, (name, spills)
        assert regs <= 128, (name, regs)  # 512 registers per SIMD lane / 4 waves


def test_the_pin_is_the_backwards_alone(listing):
    """The reverse sum, the indexed and the in-place scans are not pinned (they keep the code they had): none of them
    may have been squeezed into scratch by a pin that was meant for the backward."""
    kernels = _scan_kernels(listing)
    others = {k: v for k, v in kernels.items() if "gcp_scan_mainILi2E" not in k}
    assert len(others) >= 8, sorted(kernels)
    for name, (scratch, _, spills, _) in others.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
