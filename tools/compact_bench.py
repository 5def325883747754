"""compact_finish alone at a BASELINE scene size, with and without dropped rows: A/B runs of library variants.

  GCP_LIBRARY=variants/<name>.so python tools/compact_bench.py [cfg3] [--iters 10]

variants/<name>.so: lib/libgrouped_cumprod_hip.so as built from another checkout.
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplegaussiansplat_tk71_amd import raster, synthetic  # noqa: E402
from tools.wrapper_bench import timeit  # noqa: E402

argv = sys.argv[1:]
iters = 10
if "--iters" in argv:
    i = argv.index("--iters")
    iters = int(argv[i + 1])
    del argv[i:i + 2]
dev = torch.device("cuda", 0)
for cfg in (argv or ["cfg3"]):
    sc, rects, anti, grad = synthetic.make_scene_pairs(cfg, seed=0, device=dev)
    bins = raster.bin_tiles(sc["start"], sc["end"], sc["width"], sc["height"])
    boff = raster.box_offsets(sc["start"], sc["end"], sc["width"], sc["height"])
    out = {"library": os.environ.get("GCP_LIBRARY", "in-tree"), "workload": cfg, "pairs": int(anti.numel())}
    for name, vals in (("nothing_dropped", anti), ("2pct_opaque", torch.where(torch.rand_like(anti) < 0.02, torch.zeros_like(anti), anti))):
        incl, dropped = raster.scan_boxes(bins, sc["start"], sc["end"], boff, vals, 0, count_dropped=True)
        v, k = raster.compact_finish(incl, vals, 0, dropped=dropped)
        out[name] = {"kept": int(v.numel()), "with_counts_ms": timeit(lambda: raster.compact_finish(incl, vals, 0, dropped=dropped), iters, 3),
                     "two_launch_ms": timeit(lambda: raster.compact_finish(incl, vals, 0), iters, 3),
                     "checksum": float(v.double().sum())}
    print(json.dumps(out), flush=True)
