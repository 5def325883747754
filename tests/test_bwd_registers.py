"""Register budget and order of issue of the backward scan, read from the cross-compiled device code (no GPU), like
test_cabi.py::test_streaming_scan_kernels_hold_their_registers_without_scratch.

The kernel streams 16 B per element at three waves per SIMD (<= 168 registers, VGPRs and AGPRs together, on gfx950) and
sits at 146; a change that pushes it over loses a wave per SIMD, or spills, without failing a functional test.  Its
speed also rests on what is issued before what at the head of a tile: the tile's twelve 16-byte
loads, then the two scalar loads of `inv`, then wave 0's look-back chunk as two more 16-byte loads that nothing waits
for on the spot.  A compiler or an edit that moves the scalar loads back in front costs 7 % with every other test green."""
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from simplegaussiansplat_tk71_amd import _build

    src = [s for s in _build.SRCS if s.endswith("gcp_scan.hip")][0]
    out = tmp_path_factory.mktemp("scan") / "scan.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    res = subprocess.run([_build.find_hipcc(), *flags, "-I", _build.INCLUDE, "-S", "--cuda-device-only", "-o", str(out), src],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    return out.read_text()


def test_backward_holds_three_waves_per_simd_and_the_forward_six(listing):
    kernels = {}
    for block in listing.split("amdhsa.kernels:")[1].split("\n  - ")[1:]:  # one metadata entry per kernel
        field = lambda key: re.search(r"^(?:    )?\.%s:\s+(\S+)" % key, block, re.M).group(1)  # (the entry's own keys, not its args')
        if re.search(r"^    \.name:\s+\S*gcp_scan_main", block, re.M):
            kernels[field("name")] = (int(field("private_segment_fixed_size")), int(field("vgpr_count")) + int(field("agpr_count")),
                                      int(field("vgpr_spill_count")))
    # gcp_scan_main<MODE, ALIGNED, CARRY, INDEXED, INPLACE>: MODE 2 is the cumprod backward, one kernel per alignment
    bwd = {k: v for k, v in kernels.items() if "gcp_scan_mainILi2E" in k}
    assert len(bwd) == 2, sorted(kernels)
    for name, (scratch, regs, spills) in bwd.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
        assert regs <= 168, (name, regs)  # 512 registers per SIMD lane / 3 waves, in allocation units of 8
    # the plain and carry forward scans (MODE 0 / 1, not indexed, not in place) stay at six waves per SIMD
    fwd = {k: v for k, v in kernels.items() if re.search(r"gcp_scan_mainILi[01]ELb[01]ELb[01]ELb0ELb0EE", k)}
    assert len(fwd) == 8, sorted(kernels)
    for name, (scratch, regs, spills) in fwd.items():
        assert scratch == 0 and spills == 0 and regs <= 80, (name, scratch, regs, spills)


def test_backward_issues_its_data_loads_before_the_group_lookups(listing):
    """Full tiles of the aligned backward kernel, in the order of the listing up to the first `ds_or_b32` (the bitmap of
    the group ends): twelve `global_load_dwordx4` of the tile; behind the first of them at least two single-dword
    scalar loads (`inv` at the two ends of the wave's range); two more `global_load_dwordx4` (the look-back chunk) with
    no wait for all vector loads in the instructions right behind them."""
    m = re.search(r"^(_ZN\S*gcp_scan_mainILi2ELb1ELb0ELb0ELb0EE\S*):.*?\n(.*?)^\.Lfunc_end", listing, re.M | re.S)
    assert m, "aligned backward kernel not found"
    ins = [ln.strip() for ln in m.group(2).split("\n") if ln.strip() and not ln.strip().startswith((";", "."))]
    bitmap = next(i for i, s in enumerate(ins) if s.startswith("ds_or_b32"))
    head = ins[:bitmap]
    vec = [i for i, s in enumerate(head) if s.startswith("global_load_dwordx4")]
    assert len(vec) >= 14, len(vec)
    lookups = [i for i, s in enumerate(head) if re.match(r"s_load_dword\s", s) and i > vec[0]]
    assert len(lookups) >= 2, "the scalar loads of inv are not behind the tile's first data load"
    assert lookups[0] > vec[11], "the scalar loads of inv are issued among the tile's data loads, not behind them"
    assert not any("vmcnt(0)" in s for s in head[vec[12]:vec[13] + 4]), head[vec[12]:vec[13] + 4]
