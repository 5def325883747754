"""Occupancy of the forward scans and the reverse sum, read from the cross-compiled device code (no GPU), with the
technique of test_bwd_occupancy.py.

Nothing ships pinned beyond the parent's six waves per SIMD: eight and seven waves for the plain and carry forward
scans (<= 64 / <= 72 registers, look-back batch of three) were built and measured and are NOT faster than six
(profiles/r24_fwd_occupancy.md), so this test holds the bounds the kernels had before that round and the occupancy step
each of them sits on (that the plain forward scans are LAUNCHED at three blocks per CU, with dynamic LDS, is the host's
doing and leaves these figures alone):

  * the eight plain / carry forward kernels (MODE 0 / 1, both alignments, with and without carry): six waves, at most
    80 registers per lane, VGPRs and AGPRs together, no scratch, no spilled VGPR;
  * the four reverse-sum kernels (MODE 3, not indexed, not in place) are left to the register allocator and sit on the
    four-wave step: at most 128 registers, no scratch, no spilled VGPR (a pin to six, seven or eight puts them into
    scratch, with a look-back batch of five or of three);
  * the two backward kernels: four waves, at most 128 registers, no scratch."""
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: (scratch bytes per lane, VGPRs + AGPRs, spilled VGPRs)} of every gcp_scan_main"""
    from simplegaussiansplat_tk71_amd import _build

    src = [s for s in _build.SRCS if s.endswith("gcp_scan.hip")][0]
    out = tmp_path_factory.mktemp("scan_fwd_occ") / "scan.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    res = subprocess.run([_build.find_hipcc(), *flags, "-I", _build.INCLUDE, "-S", "--cuda-device-only", "-o", str(out), src],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    found = {}
    for block in out.read_text().split("amdhsa.kernels:")[1].split("\n  - ")[1:]:  # one metadata entry per kernel
        field = lambda key: re.search(r"^(?:    )?\.%s:\s+(\S+)" % key, block, re.M).group(1)  # (the entry's own keys, not its args')
        if re.search(r"^    \.name:\s+\S*gcp_scan_main", block, re.M):
            found[field("name")] = (int(field("private_segment_fixed_size")), int(field("vgpr_count")) + int(field("agpr_count")),
                                    int(field("vgpr_spill_count")))
    return found


def _held(kernels, pattern, count, max_registers):
    # gcp_scan_main<MODE, ALIGNED, CARRY, INDEXED, INPLACE>
    picked = {k: v for k, v in kernels.items() if re.search(pattern, k)}
    assert len(picked) == count, (pattern, sorted(kernels))
    for name, (scratch, regs, spills) in picked.items():
        print(name, "scratch", scratch, "registers", regs, "spilled VGPRs", spills)
        assert scratch == 0, (name, scratch)
        assert spills == 0, (name, spills)
        assert regs <= max_registers, (name, regs)


def test_plain_and_carry_forward_scans_hold_six_waves_per_simd_without_scratch(kernels):
    _held(kernels, r"gcp_scan_mainILi[01]ELb[01]ELb[01]ELb0ELb0EE", 8, 80)  # 512 registers per SIMD lane / 6 waves, in steps of 8


def test_reverse_sum_holds_four_waves_per_simd_without_scratch(kernels):
    _held(kernels, r"gcp_scan_mainILi3ELb[01]ELb[01]ELb0ELb0EE", 4, 128)


def test_backward_still_holds_four_waves_per_simd_without_scratch(kernels):
    _held(kernels, r"gcp_scan_mainILi2ELb[01]ELb0ELb0ELb0EE", 2, 128)
