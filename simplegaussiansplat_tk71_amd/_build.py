"""Build recipe for libgrouped_cumprod_hip.so (gfx950 only, in-tree).

Replaces the reference's setup.py (reference: setup.py:1-47, a CUDAExtension of
cuda_kernel.cpp + three .cu files).  The product here is a C-ABI shared library
(no torch types, see include/grouped_cumprod_hip.h) compiled by one explicit
hipcc invocation; Python binds it with ctypes (_lib.py).
"""
import hashlib
import os
import shutil
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
SRCS = [os.path.join(PKG_DIR, "csrc", f) for f in ("gcp_scan.hip", "gcp_bin.hip", "gcp_blend.hip", "gcp_sort.hip", "gcp_walk.hip", "gcp_compact.hip",
                                                    "gcp_pairs.hip", "gcp_pixels.hip", "gcp_project.hip", "gcp_splat.hip", "gcp_loss.hip", "gcp_optim.hip",
                                                    "gcp_densify.hip", "gcp_mcmc.hip", "gcp_contrib.hip", "gcp_absgrad.hip", "gcp_distort.hip", "gcp_filter3d.hip",
                                                    "gcp_undistort.hip", "gcp_normal.hip", "gcp_tsdf.hip", "gcp_median.hip", "gcp_knn.hip",
                                                    "gcp_meshclean.hip")]
HDRS = [os.path.join(PKG_DIR, "csrc", f) for f in ("gcp_device.hpp", "gcp_tiles.hpp", "gcp_blend_shared.hpp", "gcp_project.hpp", "gcp_philox.hpp")]
INCLUDE = os.path.join(ROOT, "include")
LIB_DIR = os.path.join(PKG_DIR, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libgrouped_cumprod_hip.so")

HIPCC_FLAGS = [
    "--offload-arch=gfx950",
    "-O3",
    "-std=c++17",
    "-ffp-contract=off",  # products and sums stay separate: same arithmetic as the reference's C++
    # hipcc's SLP pass packs neighbouring f32 adds into v_pk_add_f32, which un-fuses the DPP
    # row reductions (v_add_f32_dpp -> v_mov_b32_dpp + v_pk_add + moves): blend backward 2.1 -> 1.7 ms
    "-fno-slp-vectorize",
    "-fPIC",
    "-shared",
]


def find_hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (looked at $HIPCC, /opt/rocm/bin/hipcc, PATH)")


def source_hash():
    """sha256 over the kernel sources, the headers and the compile flags: compiled into the library
    (gcp_source_hash()) so a binary older than the checkout is detected whatever the file times say — the .so is
    git-ignored and travels to the GPU box separately from the sources."""
    h = hashlib.sha256()
    for path in [*SRCS, *HDRS, os.path.join(INCLUDE, "grouped_cumprod_hip.h")]:
        with open(path, "rb") as f:
            h.update(os.path.basename(path).encode() + b"\0" + f.read() + b"\0")
    h.update(" ".join(HIPCC_FLAGS).encode())
    return h.hexdigest()[:32]


def built_hash():
    """Hash string compiled into the library on disk, or None (missing / older than this mechanism).  Read from the
    file's bytes, not through dlopen: a library loaded once stays mapped under its path even after a rebuild."""
    if not os.path.exists(LIB_PATH):
        return None
    import re

    with open(LIB_PATH, "rb") as f:
        m = re.search(rb"GCPSRCHASH:([0-9a-f]{32})", f.read())
    return m.group(1).decode() if m else None


def is_stale():
    return built_hash() != source_hash()


def build_hip_library(force=False, verbose=False):
    """Compile the HIP library in-tree; returns its path."""
    if not force and not is_stale():
        return LIB_PATH
    os.makedirs(LIB_DIR, exist_ok=True)
    cmd = [find_hipcc(), *HIPCC_FLAGS, f'-DGCP_SOURCE_HASH="{source_hash()}"', "-I", INCLUDE, "-o", LIB_PATH, *SRCS]
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + res.stdout + res.stderr)
    if verbose and res.stderr:
        print(res.stderr)
    return LIB_PATH
