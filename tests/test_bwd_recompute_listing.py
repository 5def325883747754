"""The cumprod backward that rebuilds param_cumprod in the tile (scan MODE 4), read from the cross-compiled device code (no
GPU), in the manner of test_bwd_occupancy.py and test_bwd_registers.py.

It is pinned to four waves per SIMD like MODE 2 (at most 128 registers per lane on gfx950, and the pin only pays without
scratch), and its point is the stream it does not read: a full tile of the aligned kernel issues eight 16-byte loads
(`param`, `grad_out`), not twelve, ahead of the scalar lookups of `inv`.  A second segmented scan
that pushed the kernel into scratch, or an edit that brought the tile's param_cumprod loads back, would pass every
functional test."""
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from simplegaussiansplat_tk71_amd import _build

    src = [s for s in _build.SRCS if s.endswith("gcp_scan.hip")][0]
    out = tmp_path_factory.mktemp("scan_recompute") / "scan.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    res = subprocess.run([_build.find_hipcc(), *flags, "-I", _build.INCLUDE, "-S", "--cuda-device-only", "-o", str(out), src],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    return out.read_text()


def _recompute_kernels(listing):
    """{mangled name: (scratch bytes per lane, VGPRs + AGPRs, spilled VGPRs)} of gcp_scan_main<4, ...>"""
    kernels = {}
    for block in listing.split("amdhsa.kernels:")[1].split("\n  - ")[1:]:  # one metadata entry per kernel
        field = lambda key: re.search(r"^(?:    )?\.%s:\s+(\S+)" % key, block, re.M).group(1)  # (the entry's own keys, not its args')
        if re.search(r"^    \.name:\s+\S*gcp_scan_mainILi4E", block, re.M):
            kernels[field("name")] = (int(field("private_segment_fixed_size")), int(field("vgpr_count")) + int(field("agpr_count")),
                                      int(field("vgpr_spill_count")))
    return kernels


def test_two_kernels_at_four_waves_per_simd_without_scratch(listing):
    kernels = _recompute_kernels(listing)
    assert len(kernels) == 2, sorted(kernels)  # one per alignment
    for name, (scratch, regs, spills) in kernels.items():
        print(name, "scratch", scratch, "registers", regs, "spilled VGPRs", spills)
        assert scratch == 0, (name, scratch)
        assert spills == 0, (name, spills)
        assert regs <= 128, (name, regs)  # 512 registers per SIMD lane / 4 waves


def test_a_tile_issues_eight_16_byte_loads_before_the_group_lookups(listing):
    """The aligned kernel, in the order of the listing: exactly eight `global_load_dwordx4` (four of grad_out, four of
    param) ahead of the first single-dword scalar load that follows the tile's first data load (`inv` at an end of the
    wave's range)."""
    m = re.search(r"^(_ZN\S*gcp_scan_mainILi4ELb1ELb0ELb0ELb0EE\S*):.*?\n(.*?)^\.Lfunc_end", listing, re.M | re.S)
    assert m, "aligned recompute kernel not found"
    ins = [ln.strip() for ln in m.group(2).split("\n") if ln.strip() and not ln.strip().startswith((";", "."))]
    vec = [i for i, s in enumerate(ins) if s.startswith("global_load_dwordx4")]
    assert vec, "no 16-byte loads"
    lookup = next(i for i, s in enumerate(ins) if re.match(r"s_load_dword\s", s) and i > vec[0])
    ahead = [i for i in vec if i < lookup]
    assert len(ahead) == 8, (len(ahead), lookup)
