"""No kernel writes outside its outputs or its workspace, skips an output element, depends on what a buffer held before, or
modifies an input ("Write guards").  One table of scenarios; every scenario is a thunk `run(A, mp)` that builds
its inputs with the suite's own builders, places them with `A.put`, takes caller-owned outputs from `A` and calls public
wrappers.  It runs twice: plainly, then with its inputs in guarded blocks and the listed package modules allocating from
the arena (tests/guarded_alloc.py).  Then, exactly:

  (a) every guard byte of every block allocated during the call still holds the paint;
  (b) every result has the bits of the plain run;
  (c) no result holds a word of paint;
  (d) every input has the bits it was given, the documented in-place operands (`A.put(..., inplace=True)`) apart.

A thunk returns {name: tensor}: what the wrapper returns as a result.  Buffers a wrapper documents as capacity-sized or
opaque are returned only up to their documented extent (or not at all), with the docstring sentence that allows it next to
the slice: EXEMPT below lists them.  Every test prints one line "GUARD family name blocks=N".

Entry points of the C ABI (`_lib.SIGNATURES`) that no scenario reaches, because no public wrapper that writes device memory
calls them: the earlier forms kept for C callers — gcp_project_forward, gcp_project_backward, gcp_project_backward_depth,
gcp_splat_forward, gcp_splat_backward (the wrappers call the _sh / _flags forms) — and gcp_workspace_init (`Workspace` zeroes
its block with torch); gcp_last_fallback_tiles and gcp_last_lookback_tiles, which read the module's own workspace back; and
the host-only calls gcp_abi_version, gcp_source_hash, gcp_status_string, gcp_last_hip_error, gcp_set_lookback_wait_us,
gcp_set_validate_operands.
"""
import math

import numpy as np
import pytest
import torch

from simplegaussiansplat_tk71_amd import _lib, density, filter3d, lens, loss, mesh, normals, optim, projection, raster
from simplegaussiansplat_tk71_amd import grouped_cumprod as gc
from tests.guarded_alloc import Arena, guarded, same_bits
from tests.util import make_keys, make_scene, make_values

pytestmark = pytest.mark.gpu

# what (c) does not ask for, and the sentence that allows it
EXEMPT = {
    "tile_list past the listed entries (bin_tiles, capacity=)":
        "raster.bin_tiles: \"`bins.n_tile_pairs` is then the capacity, the true count stays on the device (`bins.info`)\"",
    "t_ckpt (blend_forward / blend_forward_depth, with_checkpoints=True)":
        "raster.blend_forward: \"t_ckpt being the per-pixel transmittance checkpoints `blend_backward` restarts from\" — opaque, sized "
        "by gcp_blend_checkpoint_floats for the capacity; what the backward computes from it is checked",
    "rect-cut row arrays (rects_to_boxes)":
        "raster._cut_rects_once: \"slot_rows / min_rect: the room made — row records per 4096-pair tile, pairs per rectangle\": "
        "start / end / box_off / tile_off are allocated for `cap` rectangles and returned cut to the n_rects found",
    "pixels_min rows past the count":
        "raster.pixels_min: \"The read that sizes the result (the number of distinct pixels, as torch.unique has it) remains in every "
        "case\": out_xy / out_val are allocated for min(table, n) rows and returned cut to the count",
    "partial block sums (loss, normals)":
        "internal to the wrappers and reduced there: never returned, so (c) has nothing to ask; their guards are checked",
    "finish_boxes values of dropped pairs":
        "raster.finish_boxes: \"Where `keep` is 0 the pair is dropped and its `final` is unspecified: a wave whose 64 pixels have all "
        "reached the product 0 clears the bytes of the rest of its list and stores no values there\"",
    "compact_finish values past the kept count":
        "raster.compact_finish: \"the kept count sizes the returned tensor, as the reference's boolean-mask indexing does\"",
}


class Alloc:
    """What a thunk places its inputs and takes its caller-owned outputs with: torch's allocator (arena None) or the arena."""

    def __init__(self, arena, device):
        self.arena, self.device, self.inputs = arena, device, []

    def put(self, t, inplace=False, offset_bytes=0):
        t = t.to(self.device)
        if self.arena is None:
            out = self.empty(*t.shape, dtype=t.dtype, offset_bytes=offset_bytes).copy_(t) if t.numel() else t.clone()
        else:
            out = self.arena.copy(t, offset_bytes=offset_bytes)
        if not inplace:
            self.inputs.append((out, t.clone()))
        return out

    def empty(self, *shape, dtype=torch.float32, offset_bytes=0):
        if self.arena is not None:
            return self.arena.empty(*shape, dtype=dtype, device=self.device, offset_bytes=offset_bytes)
        nbytes = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()
        raw = torch.empty(nbytes + 16, dtype=torch.uint8, device=self.device)
        return raw[offset_bytes:offset_bytes + nbytes].view(dtype).view(shape)

    def zeros(self, *shape, dtype=torch.float32, offset_bytes=0):
        t = self.empty(*shape, dtype=dtype, offset_bytes=offset_bytes)
        return t.zero_() if t.numel() else t


SCENARIOS = []


def scenario(family, name, *modules):
    def add(run):
        SCENARIOS.append(pytest.param(family, modules, run, id=f"{family}-{name}"))
        return run
    return add


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- scans ---------------------------------------------------------------------------------------------------------------
SCAN_SIZES = {"1": lambda T: 1, "5": lambda T: 5, "T-1": lambda T: T - 1, "T+1": lambda T: T + 1, "3T+1": lambda T: 3 * T + 1}
SCAN_DISTS = ("poisson8", "one_run", "runs9000")
FORWARD = {"cumprod_forward": gc.grouped_cumprod_forward, "cumsum_forward": gc.grouped_cumsum_forward, "cumsum_reverse": gc.grouped_cumsum_reverse}
INDEXED = {"cumprod_forward_indexed": gc.grouped_cumprod_forward_indexed, "cumsum_forward_indexed": gc.grouped_cumsum_forward_indexed,
           "cumsum_reverse_indexed": gc.grouped_cumsum_reverse_indexed}
CARRY = {"cumprod_forward_carry": gc.grouped_cumprod_forward_carry, "cumsum_forward_carry": gc.grouped_cumsum_forward_carry,
         "cumsum_reverse_carry": gc.grouped_cumsum_reverse_carry}


def _scan_workspace(A, mp, n, seed_cache):
    """A zeroed block of exactly gcp_workspace_bytes(n) in a `Workspace`; seed_cache: also the module's own for this stream."""
    ws = gc.Workspace(A.device, n)
    ws.tensor = A.zeros(_lib.load().gcp_workspace_bytes(n), dtype=torch.uint8)
    if seed_cache:
        mp.setitem(gc._workspaces, (A.device.index, torch.cuda.current_stream(A.device).cuda_stream), ws)
    return ws


def _scan_scenario(entry, size, dist, offset):
    @scenario("scans", f"{entry}-{size}-{dist}-off{offset}")
    def run(A, mp):
        from oracle import c_oracle as co

        n = SCAN_SIZES[size](gc.tile_elems())
        key = make_keys(n, dist, seed=n)
        inv, inv_len = co.groups_from_key(key)
        x = make_values(n, seed=n, kind="alpha" if dist == "poisson8" else "near1")
        outs = [A.empty(n, offset_bytes=offset) for _ in range(2)]  # a fresh workspace, then the same one again
        if entry in FORWARD:
            ws = _scan_workspace(A, mp, n, False)
            args = (A.put(x), A.put(key))
            for out in outs:
                FORWARD[entry](*args, out, workspace=ws)
        elif entry in INDEXED:
            _scan_workspace(A, mp, n, True)
            args = (A.put(x), A.put(key), A.put(torch.randperm(n, generator=_gen(n)).to(torch.int32)))
            for out in outs:
                INDEXED[entry](*args, out)
        elif entry in CARRY:
            _scan_workspace(A, mp, n, True)
            args = (A.put(x), A.put(inv), A.put(0.25 + 0.75 * torch.rand(inv_len.numel(), generator=_gen(n))))
            for out in outs:
                CARRY[entry](*args, out)
        else:
            ws = _scan_workspace(A, mp, n, False)
            args = (A.put(x), A.put(co.cumprod_forward(x, key)), A.put(make_values(n, seed=n + 3, kind="normal")), A.put(inv))
            ends = A.put(inv_len)
            for out in outs:
                gc.grouped_cumprod_backward(*args, out, ends, workspace=ws)
        return {"first": outs[0], "second": outs[1]}


def _operand_checks_scenario(size):
    @scenario("scans", f"operand_checks-{size}")
    def run(A, mp):
        from oracle import c_oracle as co

        n = SCAN_SIZES[size](gc.tile_elems())
        inv, inv_len = co.groups_from_key(make_keys(n, "poisson8", seed=n))
        index = torch.randperm(n, generator=_gen(n)).to(torch.int32)
        index[n // 2] = index[0]  # one repeat
        inv_d, ends, index = A.put(inv), A.put(inv_len), A.put(index)
        counts = [gc.check_groups(inv_d, ends), gc.check_permutation(index), gc.check_group_ids(inv_d, inv_len.numel())]
        assert counts == [0, int(n > 1), 0]
        return {"counts": A.put(torch.tensor(counts))}  # they report to the host: the guards of their operands are the check


for _size in ("5", "T+1"):
    _operand_checks_scenario(_size)

for _entry in (*FORWARD, *INDEXED, *CARRY, "cumprod_backward"):
    for _size in SCAN_SIZES:
        for _dist in SCAN_DISTS:
            for _offset in (0, 4):
                _scan_scenario(_entry, _size, _dist, _offset)


# ---- sorts and index plumbing --------------------------------------------------------------------------------------------
SORT_SIZES = (1, 63, 4095, 4097, 100003)
W_MAX, H_MAX = 1919, 1079


def _sort_scenarios(n):
    @scenario("sorts", f"stable_sort_keys-{n}", raster)
    def keys(A, mp):
        k = A.put(torch.randint(0, 1 << 20, (n,), generator=_gen(n), dtype=torch.int32))
        a, b = raster.stable_sort_keys(k, key_bits=20)
        c, d = raster.stable_sort_keys(k)  # read back
        return {"keys_bits": a, "index_bits": b, "keys_read": c, "index_read": d}

    @scenario("sorts", f"sort_rects-{n}", raster)
    def rects(A, mp):
        g = _gen(n + 1)
        r = A.put(torch.stack([torch.randint(0, W_MAX + 1, (n,), generator=g), torch.randint(0, H_MAX + 1, (n,), generator=g)], 1).to(torch.int32))
        out = {}
        for name, kw in (("bits", {"key_bits": (H_MAX * 10000 + W_MAX).bit_length()}), ("image", {"image_size": (W_MAX, H_MAX)}), ("read", {})):
            out["key_" + name], out["index_" + name] = raster.sort_rects(r, **kw)
        return out

    @scenario("sorts", f"gather_unsort-{n}", raster)
    def plumbing(A, mp):
        g = _gen(n + 2)
        index = A.put(torch.randperm(n, generator=g).to(torch.int32))
        src = A.put(torch.randn(n, generator=g))
        inc = torch.rand(n, generator=g)
        inc[::5] = 0.0
        inc, sx = A.put(inc), A.put(0.1 + torch.rand(n, generator=g))
        out = {"gathered": raster.gather_f32(src, index)}
        for mode in (0, 1):
            out[f"full{mode}"], out[f"keep{mode}"] = raster.unsort_finish(inc, sx, index, mode)
        return out


for _n in SORT_SIZES:
    _sort_scenarios(_n)


def _compact_scenario(n, zero_every, whole, mode):
    begin, end = (0, n) if whole else (1, n - 2)

    @scenario("sorts", f"compact_finish-{n}-zero{zero_every}-{begin}to{end}-mode{mode}", raster)
    def run(A, mp):
        g = _gen(n + zero_every)
        inc = 0.05 + torch.rand(n, generator=g)
        if zero_every:
            inc[::zero_every] = 0.0
        # values past the kept count: EXEMPT["compact_finish values past the kept count"] — the wrapper returns values[:kept]
        values, keep = raster.compact_finish(A.put(inc), A.put(0.5 + torch.rand(n, generator=g)), mode, begin, end)
        return {"values": values, "keep": keep}


for _n in (1, 3, 4096, 4097):
    for _z in (0, 1, 7):
        for _whole in (True, False):
            if _whole or _n - 2 >= 1:
                for _mode in (0, 1):
                    _compact_scenario(_n, _z, _whole, _mode)


def _scan_i32_scenario(n):
    @scenario("sorts", f"exclusive_scan_i32-{n}", raster)
    def run(A, mp):
        return {"out": raster.exclusive_scan_i32(A.put(torch.randint(0, 10, (n,), generator=_gen(n), dtype=torch.int32)))}


for _n in (1, 1023, 1025, 4099, 65537):
    _scan_i32_scenario(_n)


# ---- binning, blend, rect cut and walk -----------------------------------------------------------------------------------
def _scenes():
    from tests.test_render_depth_gpu import stack_scene

    return {"1g_8x8": lambda: make_scene(1, 8, 8, 2, 1), "40g_33x17": lambda: make_scene(40, 33, 17, 4, 2),
            "400g_100x70": lambda: make_scene(400, 100, 70, 9, 3),
            "stack257": lambda: stack_scene(257, 0.02, 0.3, 5)}  # one past the forward's stage of 256


SCENE_NAMES = ("1g_8x8", "40g_33x17", "400g_100x70", "stack257")


def _placed_scene(A, name):
    """The scene's per-Gaussian arguments in A's blocks (the centre as float32: the blend then reads the block itself) plus
    depths in list order, a background and upstream gradients -> (dict, width, height)."""
    sc = _scenes()[name]()
    n, w, h = sc["start"].shape[0], sc["width"], sc["height"]
    g = _gen(n + w)
    s = {k: A.put(sc[k]) for k in ("start", "end", "vinv", "opacity", "l_d")}
    s["mean"] = A.put(sc["mean"].float())
    s["z"] = A.put(torch.sort(1.0 + 5.0 * torch.rand(n, generator=g)).values)
    s["bg"] = A.put(torch.rand(3, generator=g))
    s["g_image"] = A.put(torch.randn(h + 1, w + 1, 3, generator=g))
    for k in ("g_depth", "g_alpha", "g_dist"):
        s[k] = A.put(torch.randn(h + 1, w + 1, generator=g))
    s["args"] = (s["start"], s["end"], s["mean"], s["vinv"], s["opacity"])
    return s, w, h


def _bins_results(prefix, bins, listed=None):
    out = {prefix + "tile_off": bins.tile_off, prefix + "tile_start": bins.tile_start}
    # EXEMPT["tile_list past the listed entries (bin_tiles, capacity=)"]
    out[prefix + "tile_list"] = bins.tile_list if listed is None else bins.tile_list[:listed]
    if bins.info is not None:
        out[prefix + "info"] = bins.info
    return out


def _raster_scenarios(name):
    @scenario("binning", f"bin_tiles-{name}", raster)
    def bin_tiles(A, mp):
        s, w, h = _placed_scene(A, name)
        exact = raster.bin_tiles(s["start"], s["end"], w, h)
        K = exact.n_tile_pairs
        out = _bins_results("exact_", exact)
        roomy = raster.bin_tiles(s["start"], s["end"], w, h, capacity=K)
        assert not roomy.overflowed() and int(roomy.info[0]) == K
        out.update(_bins_results("capacity_", roomy, K))
        if K >= 2:
            tight = raster.bin_tiles(s["start"], s["end"], w, h, capacity=K - 1)
            assert tight.overflowed()  # reported; and nothing past the capacity: the guard behind tile_list
            out.update(_bins_results("tight_", tight, min(int(tight.info[0]), K - 1)))
        return out

    @scenario("binning", f"lists-{name}", raster)
    def lists(A, mp):
        s, w, h = _placed_scene(A, name)
        bins = raster.bin_tiles(s["start"], s["end"], w, h)
        pl = raster.pixel_lists(bins, s["start"], s["end"])
        out = {"pixel_off": pl.pixel_off, "pair_gauss": pl.pair_gauss, "pair_index": pl.pair_index, "pair_key": pl.pair_key, "box_off": pl.box_off}
        out["rects"] = raster.expand_rects(s["start"], s["end"], w, h)
        out["rects_owner"], out["owner"] = raster.expand_rects(s["start"], s["end"], w, h, with_gaussian=True)
        out["box_offsets"] = raster.box_offsets(s["start"], s["end"], w, h)
        return out

    @scenario("blend", f"colour-{name}", raster)
    def colour(A, mp):
        s, w, h = _placed_scene(A, name)
        n = s["start"].shape[0]
        bins = raster.bin_tiles(s["start"], s["end"], w, h)
        out = {"image_plain": raster.blend_forward(bins, *s["args"], s["l_d"])}
        # EXEMPT["t_ckpt (blend_forward / blend_forward_depth, with_checkpoints=True)"]: not a result; what is made from it is
        out["image"], ckpt = raster.blend_forward(bins, *s["args"], s["l_d"], with_checkpoints=True)
        grads = raster.blend_backward(bins, *s["args"], s["l_d"], ckpt, s["g_image"])
        out.update({f"grad{i}": t for i, t in enumerate(grads)})
        out["w_max"], out["w_sum"] = raster.blend_contribution(bins, *s["args"])
        out["absgrad"] = raster.blend_absgrad(bins, *s["args"], s["l_d"], ckpt, s["g_image"])
        mine = A.empty(n, 2)
        assert raster.blend_absgrad(bins, *s["args"], s["l_d"], ckpt, s["g_image"], out=mine) is mine
        out["absgrad_out"] = mine
        return out

    for with_bg in (False, True):
        @scenario("blend", f"depth-{name}-{'bg' if with_bg else 'black'}", raster)
        def depth(A, mp, with_bg=with_bg):
            s, w, h = _placed_scene(A, name)
            n = s["start"].shape[0]
            bg = s["bg"] if with_bg else None
            bins = raster.bin_tiles(s["start"], s["end"], w, h)
            out = dict(zip(("image_plain", "depth_plain", "alpha_plain"), raster.blend_forward_depth(bins, *s["args"], s["l_d"], s["z"], bg)))
            out["image"], out["depth"], out["alpha"], ckpt = raster.blend_forward_depth(bins, *s["args"], s["l_d"], s["z"], bg, with_checkpoints=True)
            grads = raster.blend_backward_depth(bins, *s["args"], s["l_d"], s["z"], ckpt, s["g_image"], s["g_depth"], s["g_alpha"],
                                                background=bg, background_grad=True)
            out.update({f"grad{i}": t for i, t in enumerate(grads)})
            mine = A.empty(n, 2)
            raster.blend_absgrad_depth(bins, *s["args"], s["l_d"], s["z"], ckpt, s["g_image"], s["g_depth"], s["g_alpha"], background=bg, out=mine)
            out["absgrad_out"] = mine
            out["absgrad"] = raster.blend_absgrad_depth(bins, *s["args"], s["l_d"], s["z"], ckpt, None, s["g_depth"], None, background=bg)
            return out

    @scenario("blend", f"distort-{name}", raster)
    def distort(A, mp):
        s, w, h = _placed_scene(A, name)
        bins = raster.bin_tiles(s["start"], s["end"], w, h)
        ckpt = raster.blend_forward_depth(bins, *s["args"], s["l_d"], s["z"], with_checkpoints=True)[3]
        dist, a_n, b_n = raster.blend_distort_forward(bins, *s["args"], s["z"])
        grads = raster.blend_distort_backward(bins, *s["args"], s["z"], ckpt, a_n, b_n, s["g_dist"])
        return {"dist": dist, "a_n": a_n, "b_n": b_n, **{f"grad{i}": t for i, t in enumerate(grads)}}

    def boxes_results(prefix, rb):
        # EXEMPT["rect-cut row arrays (rects_to_boxes)"]: the wrapper returns them cut to the rectangles found
        out = {prefix + "start": rb.start, prefix + "end": rb.end, prefix + "box_off": rb.box_off}
        if rb.tile_off is not None:
            out[prefix + "tile_off"] = rb.tile_off
        return out

    @scenario("rect_cut", f"rects_to_boxes-{name}", raster)
    def cut(A, mp):
        mp.setattr(raster, "_cut_sizing", {})  # what the last list cut on the device needed: the same start for both runs
        s, w, h = _placed_scene(A, name)
        rects = raster.expand_rects(s["start"], s["end"], w, h)
        out = {}
        for one_call in (True, False):
            rb = raster.rects_to_boxes(rects, one_call=one_call)
            assert rb is not None and (rb.width, rb.height) == (int(rects[:, 0].max()), int(rects[:, 1].max()))
            out.update(boxes_results(f"one_call{int(one_call)}_", rb))
        r64 = A.put(rects.long(), offset_bytes=8)  # the reference's own int64 list, 8-byte aligned only
        for one_call in (True, False):
            rb = raster.rects_to_boxes(r64, one_call=one_call)
            assert rb is not None
            out.update(boxes_results(f"i64_one_call{int(one_call)}_", rb))
        # a second chunk's list: the sorted unique pixels of the first half in front (tests/test_wrappers_gpu.py,
        # test_chunked_calls_with_carry_rows_take_the_walk)
        half = rects.size(0) // 2
        unique = torch.unique(rects[:half], dim=0)
        lst = A.put(torch.cat([unique, rects[half:]]))
        rb = raster.rects_to_boxes(lst, carry_rows=unique.size(0))
        if rb is not None:
            out.update(boxes_results("carry_", rb))
        return out

    @scenario("rect_cut", f"walk-{name}", raster)
    def walk(A, mp):
        mp.setattr(raster, "_cut_sizing", {})
        s, w, h = _placed_scene(A, name)
        rects, owner = raster.expand_rects(s["start"], s["end"], w, h, with_gaussian=True)
        m = rects.size(0)
        anti = 1.0 - s["opacity"].reshape(-1)[owner.long()].cpu() * torch.rand(m, generator=_gen(m))
        anti[::17] = 0.0
        anti = A.put(anti)
        rb = raster.rects_to_boxes(rects)
        assert rb is not None
        bins = rb.bin()
        out = _bins_results("bins_", bins)
        for mode in (0, 1, 2):
            out[f"scan{mode}"], out[f"dropped{mode}"] = raster.scan_boxes(bins, rb.start, rb.end, rb.box_off, anti, mode, count_dropped=True)
        out["scan_plain"] = raster.scan_boxes(bins, rb.start, rb.end, rb.box_off, anti, 0)
        # EXEMPT["finish_boxes values of dropped pairs"]: `final` is a result where `keep` is set
        final, keep, dropped = raster.finish_boxes(bins, rb.start, rb.end, rb.box_off, anti, 0)
        out.update(final=torch.where(keep.view(torch.bool), final, torch.zeros_like(final)), keep=keep, dropped=dropped)
        f1, k1, d1 = raster.finish_boxes(bins, rb.start, rb.end, rb.box_off, anti, 1, buffers=raster.finish_buffers(anti))
        out.update(final_prepared=torch.where(k1.view(torch.bool), f1, torch.zeros_like(f1)), keep_prepared=k1, dropped_prepared=d1)
        out["kept_values"], out["kept_mask"] = raster.compact_kept(final, keep, dropped)
        out["kept_values_counted"], out["kept_mask_counted"] = raster.compact_kept(final, keep)
        if m > 3:
            out["kept_values_slice"], out["kept_mask_slice"] = raster.compact_kept(final, keep, dropped, 1, m - 2)
        out["finish_dropped"], out["finish_keep"] = raster.compact_finish(out["scan0"], anti, 0, dropped=out["dropped0"])
        return out

    @scenario("rect_cut", f"pixels_min-{name}", raster)
    def pixels(A, mp):
        mp.setattr(raster, "_extent_seen", {})
        s, w, h = _placed_scene(A, name)
        rects = raster.expand_rects(s["start"], s["end"], w, h)
        values = A.put(torch.rand(rects.size(0), generator=_gen(7)))
        out = {}
        # EXEMPT["pixels_min rows past the count"]: the wrapper returns both arrays cut to the count
        for tag, r in (("i32", rects), ("i64", A.put(rects.long()))):
            out[tag + "_xy_sized"], out[tag + "_min_sized"] = raster.pixels_min(r, values, image_size=(w, h))
            out[tag + "_xy_measured"], out[tag + "_min_measured"] = raster.pixels_min(r, values)
            out[tag + "_xy_first"], out[tag + "_first"] = raster.pixels_min(r, None, image_size=(w, h))
            out[tag + "_xy_first_seen"], out[tag + "_first_seen"] = raster.pixels_min(r)  # from the remembered extent
        return out


for _name in SCENE_NAMES:
    _raster_scenarios(_name)


# ---- projection ----------------------------------------------------------------------------------------------------------
def _projection_scenario(family, with_depth, degree, capture_safe, n):
    options = {} if family == "project" else {"centres": "subpixel", "cov_dilation": 0.3, "clamp_colour": True}

    @scenario("projection", f"{family}-{'depth' if with_depth else 'nodepth'}-deg{degree}-{'capture' if capture_safe else 'read'}-{n}", projection, raster)
    def run(A, mp):
        from tests.test_sh3_gpu import NAMES, TILE_LOGIT, random_world

        w = random_world(n, 2, 40, 30, 7 + n, "cpu", sigma=0.05, n_basis=16)
        leaves = [A.put(w[k]).requires_grad_(True) for k in NAMES]
        cams, grad_iter, _ = projection.camera_inputs(*leaves, A.put(w["P"]), A.put(w["K"]), w["wh"].tolist(), TILE_LOGIT, L_max=degree,
                                                      capture_safe=capture_safe, with_depth=with_depth, **options)
        out = {"grad_iter": grad_iter}
        paths = ("variance_inverse", "opacity", "l_d") + (("depth",) if with_depth else ()) + (("mean",) if options else ())
        total = None
        for c, cam in enumerate(cams):
            if cam is None:
                continue
            out.update({f"cam{c}_{k}": v for k, v in cam.items()})
            for k in paths:
                term = (cam[k] * torch.linspace(0.5, 1.5, cam[k].numel(), device=A.device).reshape(cam[k].shape)).sum()
                total = term if total is None else total + term
        if total is not None:
            grads = torch.autograd.grad(total, leaves, allow_unused=True)
            out.update({"grad_" + k: g for k, g in zip(NAMES, grads) if g is not None})
        return out


for _family in ("project", "splat"):
    for _with_depth in (False, True):
        for _degree in (0, 3):
            for _capture in (False, True):
                for _n in (1, 65, 1000):
                    _projection_scenario(_family, _with_depth, _degree, _capture, _n)


# ---- loss ----------------------------------------------------------------------------------------------------------------
LOSS_SHAPES = ((1, 3, 6, 6), (1, 3, 17, 33), (2, 3, 39, 71))


def _loss_scenarios(shape):
    tag = "x".join(map(str, shape))

    def case(A):
        from tests.test_exposure_gpu import _case

        x, b, E, _ = _case(shape, 0, 11 + shape[2])
        return A.put(x), A.put(b), A.put(E)

    for want in ("plain", "exposure_e", "exposure_x", "exposure_both"):
        @scenario("loss", f"splat_loss-{want}-{tag}", loss)
        def splat(A, mp, want=want):
            x, b, E = case(A)
            x.requires_grad_(want in ("plain", "exposure_x", "exposure_both"))
            E.requires_grad_(want in ("exposure_e", "exposure_both"))
            value = loss.splat_loss(x, b, 0.2, exposure=None if want == "plain" else E)
            value.backward()
            out = {"loss": value.detach()}
            if x.grad is not None:
                out["grad_x"] = x.grad
            if E.grad is not None:
                out["grad_e"] = E.grad
            assert (x.grad is not None) == x.requires_grad and (E.grad is not None) == E.requires_grad
            return out

    for clamp in (True, False):
        for with_e in (False, True):
            @scenario("loss", f"image_metrics-{'clamp' if clamp else 'raw'}-{'exposure' if with_e else 'plain'}-{tag}", loss)
            def metrics(A, mp, clamp=clamp, with_e=with_e):
                x, b, E = case(A)
                return loss.image_metrics(1.5 * x - 0.2, b, clamp=clamp, exposure=E if with_e else None)._asdict()


for _shape in LOSS_SHAPES:
    _loss_scenarios(_shape)


# ---- normals -------------------------------------------------------------------------------------------------------------
def _normals_scenario(n, full):
    @scenario("normals", f"gaussian_normals-{n}-{'full' if full else 'subset'}", normals)
    def run(A, mp):
        from tests.normal_cases import normals_case

        q, scale, mean, P_c, index, G = normals_case(n, full)
        q = A.put(q).requires_grad_(True)
        normal = normals.gaussian_normals(q, A.put(scale), A.put(mean), A.put(P_c), A.put(index))
        out = {"normal": normal.detach()}
        if index.numel():
            normal.backward(A.put(G))
            out["grad_q"] = q.grad
        return out


def _consistency_scenario(batch, height, width):
    @scenario("normals", f"consistency-{batch}x{height}x{width}", normals)
    def run(A, mp):
        from tests.normal_cases import consistency_case

        depth, alpha, normal, K = (A.put(t) for t in consistency_case(batch, height, width))
        leaves = [t.requires_grad_(True) for t in (depth, alpha, normal)]
        value = normals.normal_consistency(*leaves, K)
        value.backward()
        out = {"loss": value.detach(), "grad_depth": depth.grad, "grad_alpha": alpha.grad, "grad_normal": normal.grad}
        out["e_map"], out["defined"] = normals.normal_consistency_map(depth.detach(), alpha.detach(), normal.detach(), K)
        out["depth_normals"] = normals.depth_normals(depth.detach(), alpha.detach(), K)
        return out


for _n in (1, 65, 1000):
    for _full in (False, True):
        _normals_scenario(_n, _full)
for _batch in (1, 3):
    for _h, _w in ((3, 3), (17, 33), (33, 65)):
        _consistency_scenario(_batch, _h, _w)


# ---- filter, lens, optimiser, density, mesh -------------------------------------------------------------------------------
def _filter_scenarios():
    for n_cam in (1, 3):
        @scenario("filter3d", f"sampling_rate-{n_cam}cam", filter3d)
        def rate(A, mp, n_cam=n_cam):
            from tests.test_sh3_gpu import random_world

            w = random_world(257, n_cam, 40, 30, 3, "cpu", sigma=0.05, n_basis=9)
            r = filter3d.sampling_rate(A.put(w["mean"]), A.put(w["P"]), A.put(w["K"]), w["wh"])
            return {"rate": r, "filter": filter3d.filter_from_rate(r)}

    from tests.filter3d_torch import APPLY_SIZES

    for n in sorted(APPLY_SIZES)[:3]:
        @scenario("filter3d", f"apply_filter-{n}", filter3d)
        def apply(A, mp, n=n):
            g = _gen(n)
            v = A.put(torch.log(0.05 * (0.4 + 1.2 * torch.rand(n, 3, generator=g)))).requires_grad_(True)
            x = A.put(torch.logit(0.02 + 0.96 * torch.rand(n, 1, generator=g))).requires_grad_(True)
            phi = torch.rand(n, generator=g) * 0.1
            phi[::4] = 0.0
            v2, x2 = filter3d.apply_filter(v, x, A.put(phi))
            g_v, g_x = torch.autograd.grad([v2, x2], [v, x], [A.put(torch.randn(n, 3, generator=g)), A.put(torch.randn(n, 1, generator=g))])
            return {"variance_scale": v2.detach(), "opacity": x2.detach(), "grad_v": g_v, "grad_x": g_x}


_filter_scenarios()


def _lens_scenarios():
    from tests import undistort_torch as ut

    for width, height, f in ut.SIZES[:2]:
        for kind in ("u8", "f32"):
            @scenario("lens", f"undistort-{kind}-{width}x{height}", lens)
            def run(A, mp, width=width, height=height, f=f, kind=kind):
                dicts = [ut.make_lens(name, width, height, f * (1 + 0.03 * i)) for i, name in enumerate(("OpenCV", "fisheye", "identity"))]
                lenses = [lens.Lens(**d) for d in dicts]
                K = torch.stack([lens.fit_pinhole(one)[0] for one in lenses])
                photo = ut.random_bytes(3, width, height, 5)
                if kind == "f32":
                    photo = (photo.permute(0, 3, 1, 2).float() / 255).contiguous()
                return {"out": lens.undistort(A.put(photo), lenses, K)}


_lens_scenarios()


def _adam_scenario(n, masked):
    @scenario("optim", f"adam_per_tensor-{n}", optim) if masked is None else scenario("optim", f"fused_adam-{n}-{'masked' if masked else 'dense'}", optim)
    def run(A, mp):
        g = _gen(n)
        shapes = ((n, 3), (n, 4), (n, 1), (n, 9, 3))
        params = [A.put(torch.randn(s, generator=g), inplace=True) for s in shapes]  # in place: the parameters
        for p in params:
            p.grad = A.put(torch.randn(p.shape, generator=g))
        opt = optim.HipAdam([{"params": [p], "lr": 1e-3 * (i + 1)} for i, p in enumerate(params)], fused=masked is not None)
        visible = A.put(torch.rand(n, generator=g) < 0.6) if masked else None
        for _ in range(2):  # the first step allocates Adam's state (in place from then on) and, fused, the rate vectors
            opt.step(*(() if masked is None else (visible,)))
        out = {}
        for i, p in enumerate(params):
            out[f"param{i}"] = p
            out.update({f"{k}{i}": opt.state[p][k] for k in ("exp_avg", "exp_avg_sq") + (() if masked is None else ("step",))})
        return out


for _n in (1, 1001, 3 * 4096 + 2):
    for _masked in (False, True, None):  # None: one gcp_adam_step per tensor (fused=False)
        _adam_scenario(_n, _masked)


def _density_scenario(n):
    def cloud(A, g):
        from tests.density_torch import NAMES

        shapes = {"mean": (n, 3), "variance_q": (n, 4), "variance_scale": (n, 3), "opacity": (n, 1), "color": (n, 9, 3)}
        raw = {k: torch.randn(shapes[k], generator=g) for k in NAMES}
        raw["variance_scale"] = torch.log(0.02 + 0.3 * torch.rand(n, 3, generator=g))
        raw["opacity"] = torch.logit(0.001 + 0.9 * torch.rand(n, 1, generator=g))
        moments = {k: (torch.randn(shapes[k], generator=g), torch.rand(shapes[k], generator=g)) for k in NAMES}
        return raw, moments

    def flat(prefix, new, new_moments):
        out = {f"{prefix}{k}": t for k, t in new.items()}
        for k, pair in new_moments.items():
            out[f"{prefix}{k}_exp_avg"], out[f"{prefix}{k}_exp_avg_sq"] = pair
        return out

    @scenario("density", f"rows-{n}", density)
    def rows(A, mp):
        g = _gen(n)
        raw, mom = cloud(A, g)
        params = {k: A.put(t) for k, t in raw.items()}
        moments = {k: (A.put(a), A.put(b)) for k, (a, b) in mom.items()}
        norm, views = A.put(2.0 * torch.rand(n, generator=g)), A.put(torch.randint(0, 4, (n,), generator=g, dtype=torch.int32))
        new, new_moments, m = density.densify_rows(params, moments, norm, views, 0.5, 0.1, 1.0, 0.005, 2, 1234567890123)
        out = flat("densify_", new, new_moments)
        new, new_moments, extra = density.mcmc_rows(params, moments, n + n // 4 + 1, 0.005, 987654321)
        out.update(flat("mcmc_", new, new_moments))
        out.update({"mcmc_" + k: t for k, t in extra.items()})
        keep = torch.rand(n, generator=g) < 0.7
        keep[0] = True
        new, new_moments, _ = density.keep_rows(params, moments, A.put(keep))
        out.update(flat("keep_", new, new_moments))
        return out

    @scenario("density", f"in_place-{n}", density)
    def in_place(A, mp):
        g = _gen(n + 1)
        raw, _ = cloud(A, g)
        m = (2 * n) // 3 + 1 if n > 1 else 1
        index = A.put(torch.randperm(n, generator=g)[:m])
        norm_acc = A.put(torch.rand(n, generator=g), inplace=True)                                   # in place: the statistic
        view_count = A.put(torch.randint(0, 5, (n,), generator=g, dtype=torch.int32), inplace=True)  # in place
        for validate in (False, True):
            density.accumulate_screen_grads(A.put(torch.randn(m, 2, generator=g)), index, (20.0, 15.0), norm_acc, view_count, validate=validate)
        mean = A.put(raw["mean"], inplace=True)                                                      # in place: mcmc_noise's `mean`
        density.mcmc_noise(mean, A.put(raw["variance_q"]), A.put(raw["variance_scale"]), A.put(raw["opacity"]), 0.05, 424242)
        return {"norm_acc": norm_acc, "view_count": view_count, "mean": mean}


for _n in (1, 257, 1000):
    _density_scenario(_n)


def _mesh_scenarios():
    from tests import mesh_cases as mc
    from tests import mesh_ref as mr

    for colour in (True, False):
        @scenario("mesh", f"tsdf_integrate-13x7x5-{'colour' if colour else 'plain'}", mesh)
        def integrate(A, mp, colour=colour):
            case = next(c for c in mc.TSDF_CASES if c["id"] == "13x7x5")
            inp = mc.tsdf_inputs(case)
            # the volume is the in-place operand: allocated by the wrapper, so guarded with the module patched
            vol = mesh.TSDFVolume(case["origin"], case["voxel"], case["dims"], case["trunc"], A.device, colour=colour)
            vol.integrate(A.put(inp["depth"]), A.put(inp["alpha"]), A.put(inp["P"]), A.put(inp["K"]), image=A.put(inp["image"]),
                          alpha_min=mc.ALPHA_MIN, depth_max=case["depth_max"])
            out = {"tsdf": vol.tsdf, "weight": vol.weight}
            if colour:
                out["rgb"] = vol.rgb
            out["vertices"], out["faces"], colours = vol.extract()
            if colours is not None:
                out["colours"] = colours
            return out

    corner = np.full((2, 2, 2), 0.75, dtype=np.float32)
    corner[0, 0, 0] = -0.25
    fields = {"one_corner_2x2x2": lambda: (corner, None, None),
              "sphere_6x5x4": lambda: (mr.sphere_field((6, 5, 4), (2.63, 2.17, 1.41), 1.7), None, None),
              "slab_rgb": lambda: (mr.sphere_field(**mr.SPHERE), mc.slab_weight(mr.sphere_field(**mr.SPHERE).shape), True)}
    for name, make in fields.items():
        @scenario("mesh", f"extract_surface-{name}", mesh)
        def extract(A, mp, make=make):
            f, weight, rgb = make()
            f = torch.from_numpy(f)
            if rgb:
                rgb = A.put(torch.rand((3, *f.shape), generator=_gen(2)))
            v, faces, colours = mesh.extract_surface(A.put(f), None if weight is None else A.put(torch.from_numpy(weight)), rgb,
                                                     origin=(0.1, -0.2, 0.3), voxel=0.25)
            assert v.shape[0] > 0 and faces.shape[0] > 0
            out = {"vertices": v, "faces": faces}
            if colours is not None:
                out["colours"] = colours
            return out


_mesh_scenarios()


# ---- the test ------------------------------------------------------------------------------------------------------------
def _run(run, arena, modules, device, monkeypatch):
    A = Alloc(arena, device)
    with monkeypatch.context() as mp:
        if arena is not None:
            guarded(mp, arena, *modules)
        results = run(A, mp)
        torch.cuda.synchronize(device)
    return A, results


@pytest.mark.parametrize("family,modules,run", SCENARIOS)
def test_kernels_write_their_outputs_and_nothing_else(device, monkeypatch, family, modules, run, request):
    _, plain = _run(run, None, modules, device, monkeypatch)
    arena = Arena()
    A, got = _run(run, arena, modules, device, monkeypatch)
    print(f"GUARD {family} {request.node.callspec.id} blocks={len(arena.blocks)} results={len(got)}")
    assert len(arena.blocks) > 0 and len(got) > 0 and sorted(got) == sorted(plain)
    assert arena.check() == [], "(a) a guard byte was written"
    different = [k for k in got if not same_bits(got[k], plain[k])]
    assert different == [], "(b) results that differ from the plain run's bits"
    unwritten = {k: arena.unwritten(t) for k, t in got.items() if arena.unwritten(t)}
    assert unwritten == {}, "(c) results that still hold paint"
    changed = [i for i, (t, before) in enumerate(A.inputs) if not same_bits(t, before)]
    assert changed == [], "(d) inputs that were modified (in placement order)"


def test_a_stray_write_on_the_device_is_reported(device):
    """One element past the output, inside the thunk's own arena block: nothing leaves the allocation."""
    arena = Arena()
    arena.empty(7, dtype=torch.int32, device=device).fill_(1)
    out = arena.empty(1001, dtype=torch.float32, device=device)
    out.fill_(1.0)
    torch.as_strided(out, (1,), (1,), out.storage_offset() + 1001).fill_(7.0)
    torch.cuda.synchronize(device)
    assert arena.check() == [{"order": 1, "dtype": torch.float32, "shape": (1001,), "side": "after", "first": 4004, "last": 4007}]


def test_a_skipped_half_on_the_device_is_counted(device):
    arena = Arena()
    out = arena.empty(1000, dtype=torch.float32, device=device)
    out[:500] = 1.0
    keep = arena.empty(1000, dtype=torch.uint8, device=device)
    keep[::2] = 1
    torch.cuda.synchronize(device)
    assert arena.unwritten(out) == 500 and arena.unwritten(keep) == 500 and arena.check() == []
