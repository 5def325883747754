"""Density control on the device, the part that needs no GPU: the numpy Philox4x32-10 of tests/density_torch.py against the
published known answers, the fixture scene reaching every branch of the plan (asserted on the torch formulation, so that
tests/test_densify_gpu.py cannot pass vacuously), and the Python layer's refusals."""
import numpy as np
import pytest
import torch

from tests import density_torch as dt


@pytest.mark.parametrize("counter, key, want", [
    ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
], ids=["zeros", "ones", "pi"])
def test_numpy_philox_reproduces_the_known_answers(counter, key, want):
    assert dt.philox4x32_10(counter, key).tolist() == want
    # vectorised: the same answer in every row
    got = dt.philox4x32_10(np.array([counter] * 3, dtype=np.uint64), np.array([key] * 3, dtype=np.uint64))
    assert got.tolist() == [want] * 3


def test_split_normals_depend_on_seed_parent_and_child_only():
    a = dt.split_normals(7, [3, 3, 4], [0, 1, 0])
    assert np.array_equal(a[0], dt.split_normals(7, [3], [0])[0])
    assert len({tuple(r) for r in a}) == 3
    assert not np.array_equal(a, dt.split_normals(8, [3, 3, 4], [0, 1, 0]))
    assert not np.array_equal(a, dt.split_normals(7 + 2 ** 32, [3, 3, 4], [0, 1, 0]))  # the high word of the seed is the second key word
    z = dt.split_normals(1, np.arange(40000), np.zeros(40000, dtype=np.int64))
    assert np.all(np.abs(z.mean(axis=0)) <= 4 / np.sqrt(40000)) and np.all(np.abs(z.var(axis=0) - 1) <= 4 * np.sqrt(2 / 40000))


def test_fixture_scene_reaches_every_branch_of_the_plan():
    sc = dt.scene(4097)
    pl = dt.plan(sc["norm"], sc["views"], sc["variance_scale"], sc["opacity"], **dt.HYPER)
    s = torch.exp(sc["variance_scale"]).max(dim=1).values
    alpha = torch.sigmoid(sc["opacity"].reshape(-1))
    want = {  # branch -> (action, rows, a property of the Gaussians in it)
        "keep": (dt.KEEP, 1, ~pl["hot"]),
        "clone": (dt.CLONE, 2, pl["hot"] & (s <= 0.1)),
        "split": (dt.SPLIT, 2, pl["hot"] & (s > 0.1) & (s <= 1.0)),
        "split_children_pruned_by_scale": (dt.SPLIT, 0, pl["hot"] & (s / 1.6 > 1.0)),
        "prune_by_opacity": (dt.KEEP, 0, (alpha < 0.005) & (s <= 1.0)),
        "prune_by_scale": (dt.KEEP, 0, (alpha >= 0.005) & (s > 1.0)),
        "hot_without_views": (dt.KEEP, 1, (sc["views"] == 0) & (sc["norm"] >= 0.5)),
        "exactly_at_threshold": (dt.CLONE, 2, pl["g"] == 0.5),
        "clone_pruned_by_opacity": (dt.CLONE, 0, pl["hot"] & (alpha < 0.005)),
        "split_parent_over_prune_extent_children_under": (dt.SPLIT, 2, pl["hot"] & (s > 1.0) & (s / 1.6 <= 1.0)),
    }
    assert set(want) == set(dt.BRANCHES)
    for k, name in enumerate(dt.BRANCHES):
        sel = sc["branch"] == k
        action, rows, prop = want[name]
        assert int(sel.sum()) >= 8, name
        assert bool((pl["action"][sel] == action).all()) and bool((pl["count"][sel] == rows).all()) and bool(prop[sel].all()), name
    # the row list: contiguous, in Gaussian order, survivors first
    assert pl["M"] == int(pl["count"].sum()) == pl["src_row"].numel()
    assert bool((pl["src_row"][1:] >= pl["src_row"][:-1]).all())
    clones = pl["action"][pl["src_row"].long()] == dt.CLONE
    assert pl["kind"][clones].tolist() == [dt.SURVIVOR, dt.FRESH] * (int(clones.sum()) // 2)
    assert bool((pl["kind"][pl["action"][pl["src_row"].long()] == dt.SPLIT] == dt.CHILD).all())
    moments = dt.gather(pl, torch.ones(4097, 3), moments=True)
    assert bool((moments[pl["kind"] == dt.SURVIVOR] == 1).all()) and bool((moments[pl["kind"] != dt.SURVIVOR] == 0).all())


def _cpu_model(**kw):
    from simplegaussiansplat_tk71_amd import gs_model as gm

    sc = dt.scene(16)
    return gm.GS_model_with_param(sc["mean"], sc["variance_q"], sc["variance_scale"], sc["opacity"], **kw)


def test_screen_statistic_needs_float_centres():
    with pytest.raises(ValueError, match="subpixel"):
        _cpu_model(densify_on="screen")
    with pytest.raises(ValueError, match="subpixel"):
        _cpu_model(densify_on="screen", centres="pixel", cov_dilation=0.3)
    with pytest.raises(ValueError, match="densify_on"):
        _cpu_model(densify_on="centre")
    model = _cpu_model(densify_on="screen", centres="subpixel")
    assert model.densify_on == "screen" and _cpu_model().densify_on == "position"
    assert model.screen_grads_norm.dtype == torch.float32 and model.screen_grads_views.dtype == torch.int32
    assert model.screen_grads_norm.shape == model.screen_grads_views.shape == (16,)


def test_device_methods_raise_on_cpu_tensors():
    from simplegaussiansplat_tk71_amd import gs_model as gm

    model = _cpu_model()
    with pytest.raises(RuntimeError, match="no CPU path"):
        model.densify_and_prune_device(10.0, seed=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gm.accumulate_screen_grads(torch.zeros(4, 2), torch.arange(4), (1.0, 1.0), torch.zeros(8), torch.zeros(8, dtype=torch.int32))


def test_reset_opacity_keeping_the_optimiser_on_the_cpu_model():
    """The in-place form is plain torch: on a CPU model (torch.optim.Adam) it keeps every tensor's state but the opacity's moments."""
    model = _cpu_model()
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    model.train_step()
    opt, opacity = model._optimizer, model.opacity
    before = {k: opt.state[p]["exp_avg"].clone() for k, p in model.named_parameters()}
    model.reset_opacity(0.01, keep_optimizer=True)
    assert model._optimizer is opt and model.opacity is opacity
    assert float(torch.sigmoid(model.opacity.detach()).max()) <= 0.01 + 1e-6
    for k, p in model.named_parameters():
        st = opt.state[p]
        assert int(st["step"]) == 1
        if k == "opacity":
            assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
        else:
            assert torch.equal(st["exp_avg"], before[k]) and st["exp_avg_sq"].any()
    model.reset_opacity(0.005)  # the default still rebuilds the optimiser
    assert model._optimizer is not opt and not model._optimizer.state


def test_train_refuses_an_unknown_densify_mode():
    from examples.train_cameras import train

    with pytest.raises(ValueError, match="densify"):
        train(torch.zeros(4, 3), None, None, None, None, densify="gpu")
