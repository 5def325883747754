#!/usr/bin/env python3
"""Generate tests/golden/ref_host_golden.npz: the REFERENCE's own forward scans on the inputs of
tests/test_oracle.py::test_oracle_vs_live_reference_host_build, so that the test holds where oracle/_ref/ was not built.

Runs where oracle/_ref/ was built (oracle/Makefile, target ref_host):
    make -C oracle ref_host && python tests/golden/make_ref_host_golden.py

The outputs come from the reference's grouped_cumprod_forward.cu / grouped_cumsum_forward.cu compiled unmodified for the
host (oracle/_ref/grouped_cumprod_ref_host.so: thrust::inclusive_scan_by_key, sequential fp32).  Stored per case: the two
outputs and a sha256 of the inputs (key bytes, then x bytes) that tests/util.py draws from the case's seed.  Only data is
stored; no reference source is copied.
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))
import grouped_cumprod_ref_host as ref  # noqa: E402

from tests.util import make_keys, make_values  # noqa: E402

CASES = [(1, "all1"), (777, "poisson8"), (50000, "geo80"), (50000, "mixed"), (9000, "one_run")]  # as the test draws them


def inputs_digest(key, x):
    return hashlib.sha256(key.numpy().tobytes() + x.numpy().tobytes()).hexdigest()


def main():
    out = {}
    for n, dist in CASES:
        key, x = make_keys(n, dist, n), make_values(n, n)
        y = torch.zeros_like(x)
        ref.grouped_cumprod_forward(x, key, y)
        out[f"{n}_{dist}/cumprod"] = y.numpy().copy()
        ref.grouped_cumsum_forward(x, key, y)
        out[f"{n}_{dist}/cumsum"] = y.numpy().copy()
        out[f"{n}_{dist}/inputs_sha256"] = np.array(inputs_digest(key, x))
    path = os.path.join(HERE, "ref_host_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
