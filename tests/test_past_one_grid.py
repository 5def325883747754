"""The conditions tests/test_past_one_grid_gpu.py puts on its inputs, checked where no GPU is needed: its sizes are the
first with a full block and a 3-row block in a second trip of the grid-stride loops as the sources cap them, its scenes put
every branch, enough split children, dead rows, draws and kept and culled Gaussians among the second-trip rows, the number
of weight levels is what the test says it is, and the argument check of gcp_mcmc_weights sits where the limit case needs it."""
import ctypes
import math
import re

import numpy as np
import torch

from simplegaussiansplat_tk71_amd import _build, density
from tests import density_torch as dt
from tests import mcmc_torch as mt
from tests.test_mcmc_gpu import noise_scene
from tests.test_past_one_grid_gpu import (BIG, GRID1, GRID2, MCMC_M, N1, N2, PROJECTION_CASES, SCAN_CHUNK, SCAN_SIZES, SEEDS, SPLITS, T_LIMIT_N,
                                          T_LIMIT_W, THREADS, WEIGHT_LEVELS, WEIGHT_SIZES, densify_plan, densify_scene)
from tests.test_projection_rows_gpu import SHAPES, position_config, run_formulation, sub_world, world


def _source(name):
    path = [p for p in (*_build.SRCS, *_build.HDRS) if p.endswith(name)][0]
    with open(path) as f:
        return f.read()


def test_sizes_are_the_first_with_a_full_and_a_three_row_block_in_a_second_trip():
    assert (N1, N2) == (4_194_563, 16_777_475)
    assert N1 - GRID1 == N2 - GRID2 == THREADS + 3 == BIG  # the second trip's rows are one copy of the 259-Gaussian world
    # the caps as the sources have them: another cap moves the first second trip, and these sizes with it
    for name in ("gcp_densify.hip", "gcp_mcmc.hip"):
        src = _source(name)
        assert re.search(r"constexpr int kThreads = 256;", src) and re.search(r"b > 16384 \? 16384 : b", src), name
    src = _source("gcp_project.hpp")
    assert re.search(r"constexpr int kThreads = 256;", src) and re.search(r"/ kThreads < 65536 \? \(n \+ kThreads - 1\) / kThreads : 65536", src)
    assert GRID1 == 16384 * 256 and GRID2 == 65536 * 256
    # the prefix sum: 2048 elements per block, 256 chunk totals per trip of the loop in front of a block
    src = _source("gcp_bin.hip")
    assert re.search(r"constexpr int kScanChunk = 2048;", src) and re.search(r"j < \(i64\)blockIdx\.x; j \+= 256\)", src)
    chunks = [-(-n // SCAN_CHUNK) for n in SCAN_SIZES]
    assert chunks == [257, 258, 2049]
    assert chunks[0] - 1 == 256 and chunks[1] - 1 == 257  # the last block of the first has 256 totals in front: one full trip; of the second, a second trip
    assert (chunks[2] - 1) // 256 == 8
    assert all(500 * n < 2 ** 31 for n in SCAN_SIZES)  # counts in [0, 500): the total fits


def test_every_branch_of_the_plan_sits_among_the_second_trip_gaussians():
    sc = densify_scene()
    late = sc["branch"][GRID1:]
    assert late.numel() == 259
    for b, name in enumerate(dt.BRANCHES):
        assert int((late == b).sum()) >= 1, name
    for n_split in (2, 3):
        want = densify_plan(n_split)
        assert want["M"] > GRID1 + THREADS  # fill, split and the row gather reach past 16384 blocks of output rows
        assert -(-want["M"] // THREADS) > 16384


def test_split_children_of_second_trip_parents_and_in_second_trip_rows():
    for n_split, _ in SPLITS:
        want = densify_plan(n_split)
        rows = torch.nonzero(want["kind"] == dt.CHILD).reshape(-1)
        parent = want["src_row"].long()[rows]
        assert int((parent >= GRID1).sum()) >= 8 * n_split, n_split
        assert int((rows >= GRID1).sum()) > 0, n_split
        print(n_split, "children", rows.numel(), "of second-trip parents", int((parent >= GRID1).sum()), "in second-trip rows", int((rows >= GRID1).sum()))


def test_weight_levels():
    for n, w in ((1, 1 << 16), (T_LIMIT_N, 1 << 16), (T_LIMIT_N + 1, 1 << 15), (10 ** 6, 2048), (N1, 256), (2 ** 31 - 1, 1)):
        assert density.mcmc_weight_levels(n) == mt.weight_levels(n) == w, n
        assert n * w <= 2 ** 31 - 1 and (w == 1 << 16 or n * 2 * w > 2 ** 31 - 1)
    assert all(mt.weight_levels(n) == 1 << 16 for n in WEIGHT_SIZES)  # the levels below 2^16 are the test's, not the model's, at these sizes
    assert all(w & (w - 1) == 0 and 1 <= w < 1 << 16 for w in WEIGHT_LEVELS)
    assert 256 in WEIGHT_LEVELS and 2048 in WEIGHT_LEVELS  # what the model passes at N1 and at 10^6 Gaussians


def test_total_limit_is_where_the_argument_check_puts_it():
    """n W <= 2^31 - 1 at n = 32 767, W = 2^16 and not at 32 768; gcp_mcmc_weights refuses the latter (status 1) before any
    HIP call, and passes the former on to its next check, the workspace size (status 2 with none)."""
    from simplegaussiansplat_tk71_amd import _lib

    lib = _lib.load()
    assert T_LIMIT_N * T_LIMIT_W == 2_147_418_112 <= 2 ** 31 - 1 < (T_LIMIT_N + 1) * T_LIMIT_W
    buf = ctypes.create_string_buffer(4096)  # host memory standing in for device arrays: no call below may read it
    p = [((ctypes.addressof(buf) + 63) & ~63) + 256 * k for k in range(4)]
    assert lib.gcp_mcmc_weights(p[0], T_LIMIT_N + 1, mt.MIN_OPACITY, T_LIMIT_W, p[1], p[2], p[3], 1 << 20, None) == 1
    assert lib.gcp_mcmc_weights(p[0], T_LIMIT_N, mt.MIN_OPACITY, T_LIMIT_W, p[1], p[2], p[3], 0, None) == 2
    assert lib.gcp_mcmc_weights(p[0], N1, mt.MIN_OPACITY, 512, p[1], p[2], p[3], 1 << 20, None) == 1  # N1 needs W <= 256
    assert lib.gcp_mcmc_weights(p[0], N1, mt.MIN_OPACITY, 256, p[1], p[2], p[3], 0, None) == 2
    # sigmoid(20) is exactly 1.0f, so every weight of the limit case is W
    one = 1.0 / (1.0 + torch.exp(-torch.tensor(20.0)))
    assert float(one) == 1.0 and int(mt.weights(torch.full((4, 1), 20.0), w_max=T_LIMIT_W)[0].min()) == T_LIMIT_W


def test_mcmc_scene_has_dead_rows_and_drawn_sources_in_the_second_trip():
    """With the formulation's own weights (the device's differ by at most 1 per row): dead rows among the last 259, draws
    whose source is one of them, sources drawn more than once, and every grown row a slot."""
    sc = mt.scene(N1, n_coeff=1)
    weight, dead = mt.weights(sc["opacity"])
    assert int(weight.max()) <= 256 and int(weight[~dead].min()) >= 1
    assert 8 <= int(dead[GRID1:].sum()) <= 259 - 8
    cum = np.concatenate([[0], np.cumsum(weight.numpy())])
    assert cum[-1] <= 2 ** 31 - 1
    want = mt.draw(cum, MCMC_M, SEEDS[1])
    slot, src = want["slot"], want["src_row"].long()
    assert MCMC_M - N1 == N1 // 20 and bool(slot[N1:].all()) and int(slot.sum()) == int(dead.sum()) + MCMC_M - N1
    assert int((src[slot] >= GRID1).sum()) >= 8
    assert int(want["times"].max()) >= 2
    print("slots", int(slot.sum()), "draws of a second-trip source", int((src[slot] >= GRID1).sum()), "times up to", int(want["times"].max()))


def test_relocated_sums_per_number_of_copies_as_it_did_per_row():
    """mt.relocated adds the terms of D for all rows of one n at once; a plain per-row evaluation of the same double sum
    agrees to float64 round-off, at n = 2, 3, 10 and the cap 51."""
    op = torch.logit(torch.tensor([0.02, 0.3, 0.7, 0.99, 0.5, 0.9]))[:, None]
    copies = torch.tensor([1, 2, 9, 50, 79, 1])
    scale = torch.zeros(6, 3)
    got_op, got_scale = mt.relocated(op, scale, copies)
    for j in range(6):
        o = 1 / (1 + math.exp(-float(op[j].double())))
        n = min(int(copies[j]) + 1, mt.MAX_COPIES)
        o_new = 1 - (1 - o) ** (1.0 / n)
        d = sum(math.comb(i - 1, k) * (-1) ** k * o_new ** (k + 1) / math.sqrt(k + 1) for i in range(1, n + 1) for k in range(i))
        assert abs(float(got_scale[j, 0]) - math.log(o / d)) <= 1e-9, j
        assert abs(float(got_op[j]) - math.log(max(o_new, mt.MIN_OPACITY) / (1 - max(o_new, mt.MIN_OPACITY)))) <= 1e-9, j


def test_noise_scene_has_movers_among_the_last_rows():
    sc = noise_scene(N1)
    o = torch.sigmoid(sc["opacity"]).reshape(-1)[GRID1:]
    assert o.numel() == 259
    assert int((o < 0.5).sum()) >= 64 and int((o < 0.021).sum()) >= 32 and int((o >= 0.8).sum()) >= 8
    assert not bool(((o >= 0.5) & (o < 0.8)).any())  # an opaque row is far enough above 0.5 to stay where it is (gate <= e^-79.5)


def test_tiled_world_keeps_and_culls_among_its_second_trip_rows():
    """Rows 65536 * 256 .. N2 - 1 of the tiled world are one copy of each of the 259 Gaussians; by the float32 formulation's own
    lists both families keep some of them and cull some, with one and with four colour rows."""
    residues = torch.arange(GRID2, N2) % BIG
    assert sorted(residues.tolist()) == list(range(BIG))
    assert set(PROJECTION_CASES) == {("project", 1), ("splat", 1), ("splat", 4)}
    for family, n_basis in PROJECTION_CASES:
        with torch.no_grad():
            _, cams = run_formulation(sub_world(world(SHAPES[0], 16), 0, BIG, n_basis), position_config(family, n_basis), torch.float32)
        kept = torch.zeros(BIG, dtype=torch.bool)
        kept[cams[0]["index"]] = True
        late = kept[residues]
        assert 8 <= int(late.sum()) <= BIG - 8, (family, n_basis)
        assert bool(late[:THREADS].any()) and not bool(late[:THREADS].all())  # the full block of the second trip has both
        print(family, n_basis, "kept", int(late.sum()), "of", BIG, "| the 3-row block:", late[THREADS:].tolist())
