"""The fused Adam step (gcp_adam_step_multi, csrc/gcp_optim.hip; HipAdam(fused=True), optim.py) against the float64
formulation of tests/adam_torch.py: all tensors of the model in one call from arbitrary states, a tensor past one grid beside
small ones, the row mask bit for bit, rows that must not move, the optimiser's interface, a captured step against an eager
one, and the model's `adam=` modes."""
import pytest
import torch

from simplegaussiansplat_tk71_amd import gs_model as gm
from tests import adam_torch as at

pytestmark = pytest.mark.gpu

GRID = 16384 * 256 * 4  # floats one pass of a tensor's blocks covers: at most 16384 blocks of 256 threads, one float4 each
STEPS_AND_RATES = [(s, l) for s in (1, 2, 7, 1000, 30000) for l in (1.6e-4, 1e-2, 1.0)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _fused_step(tensors, steps, lrs, device, visible=None, step_as_tensor=False):
    """One HipAdam(fused=True) step of every (p, g, m, v) from step - 1 -> [(p, m, v) on the CPU], the step counts after it."""
    params = [p.to(device).requires_grad_(True) for p, _, _, _ in tensors]
    opt = gm.HipAdam([{"params": q, "lr": lr} for q, lr in zip(params, lrs)], fused=True)
    for q, (_, g, m, v), step in zip(params, tensors, steps):
        q.grad = g.to(device)
        opt.state[q] = {"step": torch.tensor([step - 1], dtype=torch.int32, device=device) if step_as_tensor else step - 1,
                        "exp_avg": m.to(device), "exp_avg_sq": v.to(device)}
    opt.step(visible=None if visible is None else visible.to(device))
    counts = [opt.state[q]["step"] for q in params]
    assert all(torch.is_tensor(c) and c.dtype == torch.int32 and c.is_cuda and c.numel() == 1 for c in counts)
    return [(q.detach().cpu(), opt.state[q]["exp_avg"].cpu(), opt.state[q]["exp_avg_sq"].cpu()) for q in params], [int(c) for c in counts]


@pytest.mark.parametrize("colour", [27, 48])
@pytest.mark.parametrize("rows", [1, 2, 5, 67, 1025])
def test_all_model_tensors_in_one_call_against_float64(rows, colour, device):
    """Widths 3, 4, 3, 1 and the colour's: tails of 0-3 elements, tensors smaller than one block beside larger ones, float4s
    that straddle rows; steps at which the bias corrections are far from and at 1, given as int and as device tensor."""
    widths = (3, 4, 3, 1, colour)
    worst_hip, worst_torch = [0.0] * 3, [0.0] * 3
    for i, (step, lr) in enumerate(STEPS_AND_RATES):
        gen = torch.Generator().manual_seed(1000 * rows + 10 * i + colour)
        tensors = [at.state(rows, w, gen) for w in widths]
        steps, lrs = [step] * 5, [lr] * 5
        wanted = at.masked_adam(tensors, steps, lrs)
        # the guard: float32 torch.optim.Adam is inside the bounds, so a failure below is the kernel's
        for t, (want, bounds, _) in zip(tensors, wanted):
            worst_torch = list(map(max, worst_torch, at.worst(at.torch_step(*t, step, lr), want, bounds, what=("float32 torch", step, lr))))
        for as_tensor in (False, True):
            got, counts = _fused_step(tensors, steps, lrs, device, step_as_tensor=as_tensor)
            assert counts == steps
            for k, (out, (want, bounds, _)) in enumerate(zip(got, wanted)):
                worst_hip = list(map(max, worst_hip, at.worst(out, want, bounds, what=("kernel", step, lr, "tensor", k, as_tensor))))
    print(f"F1 rows {rows} colour {colour}: worst error / bound (p, m, v) kernel {worst_hip[0]:.3f} {worst_hip[1]:.3f} {worst_hip[2]:.3f}, "
          f"float32 torch {worst_torch[0]:.3f} {worst_torch[1]:.3f} {worst_torch[2]:.3f}")


def test_rates_and_steps_are_per_tensor(device):
    """Every tensor of one call at its own step count and rate."""
    gen = torch.Generator().manual_seed(77)
    tensors = [at.state(67, w, gen) for w in at.WIDTHS]
    steps, lrs = [1, 2, 7, 1000, 30000], [1.6e-4, 1e-2, 1.0, 2.5e-3, 5e-3]
    got, counts = _fused_step(tensors, steps, lrs, device)
    assert counts == steps
    for out, (want, bounds, _) in zip(got, at.masked_adam(tensors, steps, lrs)):
        at.worst(out, want, bounds)


def test_two_steps_past_one_grid_beside_small_tensors(device):
    """One tensor of more floats than one pass of its 16384 blocks covers (768 float4 of a second pass and a scalar tail of 3)
    in one call with four small ones.  Every element against float64 Adam after one step from zero moments and after a
    second from the resulting state: an element updated twice or never is off by orders of magnitude."""
    gen = torch.Generator(device=device).manual_seed(5)
    shapes = [(67, 3), (GRID + 3072 + 3,), (67, 4), (67, 3), (67, 1)]
    params = [torch.randn(s, device=device, generator=gen).requires_grad_(True) for s in shapes]
    opt = gm.HipAdam([{"params": p, "lr": 1e-2} for p in params], fused=True)
    moments = [(torch.zeros(s, device=device), torch.zeros(s, device=device)) for s in shapes]
    for step in (1, 2):
        for p in params:
            p.grad = torch.randn(p.shape, device=device, generator=gen) * 0.1
        wanted = [at.reference(p.detach(), p.grad, m, v, step, 1e-2) for p, (m, v) in zip(params, moments)]
        opt.step()
        for k, (p, (want, bounds)) in enumerate(zip(params, wanted)):
            st = opt.state[p]
            worst = at.worst((p.detach(), st["exp_avg"], st["exp_avg_sq"]), want, bounds, what=("step", step, "tensor", k))
            if k == 1:
                print(f"F2 step {step}: worst error / bound (p, m, v) {worst[0]:.3f} {worst[1]:.3f} {worst[2]:.3f}")
        del wanted
        moments = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params]
    assert all(int(opt.state[p]["step"]) == 2 for p in params)


MASK_WIDTHS = (3, 4, 3, 1, 27, 48)


@pytest.mark.parametrize("rows", [67, 1025])
def test_masked_rows_keep_their_bits_and_the_others_step(rows, device):
    """Every mask of adam_torch.masks with bytes 1 and 255: an invisible row keeps param and both moments as bit patterns — a
    -0.0 and NaNs planted in it and in its gradient included —, a visible row lies inside the bounds, the step advances."""
    worst = [0.0] * 3
    for value in (1, 255):
        for i, (name, mask) in enumerate(at.masks(rows, value).items()):
            gen = torch.Generator().manual_seed(rows + 10 * i + value)
            tensors = [at.state(rows, w, gen) for w in MASK_WIDTHS]
            hidden = (mask == 0).nonzero().reshape(-1)
            for p, g, m, v in tensors:  # at both ends of invisible rows, where a float4 may straddle into a visible one
                for r in hidden[:3].tolist() + hidden[-3:].tolist():
                    p[r, 0], m[r, 0], v[r, 0], g[r, 0] = -0.0, float("nan"), float("nan"), float("nan")
                    p[r, -1], g[r, -1] = float("nan"), float("inf")
            steps, lrs = [7] * 6, [1e-2] * 6
            got, counts = _fused_step(tensors, steps, lrs, device, visible=mask)
            assert counts == steps, name
            moved = False
            for k, (out, (p, g, m, v), (want, bounds, on)) in enumerate(zip(got, tensors, at.masked_adam(tensors, steps, lrs, mask))):
                for new, old, what in zip(out, (p, m, v), "pmv"):
                    assert torch.equal(_bits(new[~on]), _bits(old[~on])), (name, value, "tensor", k, what, "an invisible row changed")
                keep = on.reshape(-1, 1).expand_as(p)
                worst = list(map(max, worst, at.worst(out, want, bounds, keep=keep, what=(name, value, "tensor", k))))
                moved |= bool((out[0][on] != p[on]).any())
            assert moved == bool(mask.any()), (name, value, "no visible row of any tensor moved")
    print(f"F3 rows {rows}: worst error / bound (p, m, v) on visible rows {worst[0]:.3f} {worst[1]:.3f} {worst[2]:.3f}")


def test_elements_without_gradient_or_moments_do_not_move(device):
    """g = m = v = 0 leaves p bit-identical and the moments exactly zero, also in a visible row: `oneup_sh_degree` keeps the
    SH rows that are not active yet in the optimiser."""
    rows = 67
    for mask in (None, at.masks(rows)["ones"], at.masks(rows)["alternating"]):
        gen = torch.Generator().manual_seed(9)
        tensors = [at.state(rows, w, gen) for w in MASK_WIDTHS]
        for p, g, m, v in tensors:
            p[4, 0] = -0.0
            for t in (g, m, v):
                t[:, p.shape[1] // 2:] = 0.0  # the upper columns of every row, as the inactive SH coefficients
                t[4, 0] = 0.0
        got, _ = _fused_step(tensors, [3] * 6, [1e-2] * 6, device, visible=mask)
        for out, (p, g, m, v), (want, bounds, on) in zip(got, tensors, at.masked_adam(tensors, [3] * 6, [1e-2] * 6, mask)):
            still = g == 0
            assert bool(still.any()) and torch.equal(_bits(out[0][still]), _bits(p[still]))
            assert not _bits(out[1][still]).any() and not _bits(out[2][still]).any()
            at.worst(out, want, bounds, keep=on.reshape(-1, 1).expand_as(p))  # and the others moved as they should


def test_optimiser_interface(device):
    gen = torch.Generator().manual_seed(11)
    a0, b0, ga, gb = (torch.randn(37, 3, generator=gen) for _ in range(4))
    a, b = a0.to(device).requires_grad_(True), b0.to(device).requires_grad_(True)
    c = torch.ones(5, device=device, requires_grad=True)
    d0 = torch.randn(37, 3, generator=gen)
    d = d0.to(device).requires_grad_(True)
    opt = gm.HipAdam([{"params": a, "lr": 1e-2}, {"params": [c, b], "lr": 1.6e-4}, {"params": d, "lr": 1.0}], fused=True)
    a.grad, b.grad, d.grad = ga.to(device), gb.to(device), ga.to(device)
    opt.state[d] = {"step": 6, "exp_avg": torch.zeros_like(d), "exp_avg_sq": torch.zeros_like(d)}  # a Python int, installed by a caller
    opt.step()
    zero = torch.zeros(37, 3)
    for q, q0, gq, lr, step in ((a, a0, ga, 1e-2, 1), (b, b0, gb, 1.6e-4, 1), (d, d0, ga, 1.0, 7)):  # each group at its own rate
        want, bounds = at.reference(q0, gq, zero, zero, step, lr)
        at.worst((q.detach().cpu(), opt.state[q]["exp_avg"].cpu(), opt.state[q]["exp_avg_sq"].cpu()), want, bounds, what=lr)
        assert int(opt.state[q]["step"]) == step and opt.state[q]["step"].dtype == torch.int32 and opt.state[q]["step"].is_cuda
    assert c not in opt.state and torch.equal(c.detach().cpu(), torch.ones(5))  # no gradient: untouched, no state
    # a parameter without gradient keeps its step while the others advance; a changed rate holds from the next step on
    opt.zero_grad()
    assert a.grad is None and b.grad is None
    b_after_one = b.detach().clone()
    opt.param_groups[0]["lr"] = 0.5
    for k in range(2, 5):
        before = [t.clone().cpu() for t in (a.detach(), opt.state[a]["exp_avg"], opt.state[a]["exp_avg_sq"])]
        a.grad = ga.to(device)
        opt.step()
        assert int(opt.state[a]["step"]) == k and int(opt.state[b]["step"]) == 1 and int(opt.state[d]["step"]) == 7
        want, bounds = at.reference(before[0], ga, before[1], before[2], k, 0.5)
        at.worst((a.detach().cpu(), opt.state[a]["exp_avg"].cpu(), opt.state[a]["exp_avg_sq"].cpu()), want, bounds, what=("lr 0.5", k))
    assert torch.equal(b.detach(), b_after_one) and torch.equal(c.detach().cpu(), torch.ones(5))
    kept = a.grad
    opt.zero_grad(set_to_none=False)
    assert a.grad is kept and float(a.grad.abs().max()) == 0.0 and c.grad is None
    # more than eight tensors: chunked, every one stepped once
    many0 = [torch.randn(5 + k, 3, generator=gen) for k in range(11)]
    many = [t.to(device).requires_grad_(True) for t in many0]
    grads = [torch.randn(t.shape, generator=gen) for t in many0]
    big = gm.HipAdam([{"params": many[:6], "lr": 1e-2}, {"params": many[6:], "lr": 1e-3}], fused=True)
    for q, g in zip(many, grads):
        q.grad = g.to(device)
    big.init_state()
    big.step()
    for k, (q, q0, g) in enumerate(zip(many, many0, grads)):
        want, bounds = at.reference(q0, g, torch.zeros_like(q0), torch.zeros_like(q0), 1, 1e-2 if k < 6 else 1e-3)
        at.worst((q.detach().cpu(), big.state[q]["exp_avg"].cpu(), big.state[q]["exp_avg_sq"].cpu()), want, bounds, what=k)
        assert int(big.state[q]["step"]) == 1
    # fused=False keeps the step a Python int (and takes no mask)
    e = a0.to(device).requires_grad_(True)
    e.grad = ga.to(device)
    plain = gm.HipAdam([{"params": e, "lr": 1e-2}])
    plain.step()
    assert type(plain.state[e]["step"]) is int and plain.state[e]["step"] == 1
    with pytest.raises(RuntimeError):
        plain.step(visible=torch.ones(37, dtype=torch.bool, device=device))
    torch.cuda.synchronize(device)
    assert plain.state[e]["step"] == 1


def test_refused_parameters_stay_unchanged(device):
    base = torch.randn(4, 8, device=device)
    good = torch.randn(4, 8, device=device, requires_grad=True)
    good0 = good.detach().clone()
    for make in (lambda: base.clone().t(),             # not contiguous
                 lambda: base.clone().double(),        # not float32
                 lambda: base.clone().reshape(-1)[1:]):  # contiguous, 4 bytes into its storage: not float4-aligned
        p = make().detach().requires_grad_(True)
        before = p.detach().clone()
        p.grad, good.grad = torch.ones_like(p), torch.ones_like(good)
        opt = gm.HipAdam([{"params": good, "lr": 0.1}, {"params": p, "lr": 0.1}], fused=True)
        with pytest.raises(RuntimeError):
            opt.step()
        torch.cuda.synchronize(device)
        assert torch.equal(p.detach(), before) and torch.equal(good.detach(), good0)  # nothing was launched: the good one stays too
    # a mask with parameters of differing leading dimension, or of another length than the rows
    other = torch.randn(5, 8, device=device, requires_grad=True)
    other0 = other.detach().clone()
    good.grad, other.grad = torch.ones_like(good), torch.ones_like(other)
    opt = gm.HipAdam([{"params": [good, other], "lr": 0.1}], fused=True)
    for mask in (torch.ones(4, dtype=torch.bool, device=device), torch.ones(5, dtype=torch.uint8, device=device)):
        with pytest.raises(RuntimeError):
            opt.step(visible=mask)
    one = gm.HipAdam([{"params": good, "lr": 0.1}], fused=True)
    for mask in (torch.ones(5, dtype=torch.bool, device=device), torch.ones(4, dtype=torch.int32, device=device), torch.ones(4, dtype=torch.bool)):
        with pytest.raises(RuntimeError):
            one.step(visible=mask)
    torch.cuda.synchronize(device)
    assert torch.equal(good.detach(), good0) and torch.equal(other.detach(), other0)
    assert all(int(st["step"]) == 0 for o in (opt, one) for st in o.state.values())


def _graph_nodes_and_edges(graph):
    """The captured graph's node count and (from, to) edges, read through the HIP runtime the process has loaded."""
    import ctypes

    path = sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line})[0]
    hip = ctypes.CDLL(path)
    handle = ctypes.c_void_p(graph.raw_cuda_graph())
    n_nodes, n_edges = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(handle, None, ctypes.byref(n_nodes)) == 0
    assert hip.hipGraphGetEdges(handle, None, None, ctypes.byref(n_edges)) == 0
    src, dst = (ctypes.c_void_p * max(1, n_edges.value))(), (ctypes.c_void_p * max(1, n_edges.value))()
    if n_edges.value:
        assert hip.hipGraphGetEdges(handle, src, dst, ctypes.byref(n_edges)) == 0
    return n_nodes.value, [(src[k], dst[k]) for k in range(n_edges.value)]


def test_a_captured_step_replays_the_device_step_and_rates(device):
    """`init_state()`, one `step()` captured on a side stream, three replays with fresh gradients in the static buffers and
    one rate changed through `sync_lr()` between them — against a second optimiser that takes the same three steps eagerly.
    Both run the same kernels on the same device scalars: parameters, moments and steps are bit-equal."""
    gen = torch.Generator().manual_seed(21)
    start = [torch.randn(67, w, generator=gen) for w in at.WIDTHS]
    grads = [[0.1 * torch.randn(67, w, generator=gen) for w in at.WIDTHS] for _ in range(3)]
    rates = [1e-2, 5e-3, 1.6e-4]  # of the first group, one per step

    def make():
        params = [t.to(device).requires_grad_(True) for t in start]
        opt = gm.HipAdam([{"params": p, "lr": 1e-3} for p in params], fused=True)
        for p in params:
            p.grad = torch.zeros_like(p)
        return params, opt

    eager_p, eager = make()
    for k in range(3):
        for p, g in zip(eager_p, grads[k]):
            p.grad.copy_(g)
        eager.param_groups[0]["lr"] = rates[k]
        eager.step()

    params, opt = make()
    opt.init_state()
    buffers = [p.grad for p in params]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph(keep_graph=True)  # the captured graph stays readable (hipGraphGetEdges below)
    with torch.cuda.graph(graph, stream=side):
        allocations = torch.cuda.memory_stats(device)["allocation.all.allocated"]
        opt.step()
        allocations = torch.cuda.memory_stats(device)["allocation.all.allocated"] - allocations
    assert allocations == 0  # the captured step allocated nothing
    assert all(int(opt.state[p]["step"]) == 0 for p in params) and all(torch.equal(p.detach().cpu(), t) for p, t in zip(params, start))
    for k in range(3):
        for buf, g in zip(buffers, grads[k]):
            buf.copy_(g)
        opt.param_groups[0]["lr"] = rates[k]
        opt.sync_lr()
        graph.replay()
        opt.zero_grad(set_to_none=False)
        assert all(p.grad is buf for p, buf in zip(params, buffers))
    torch.cuda.synchronize(device)
    for p, q in zip(params, eager_p):
        assert torch.equal(_bits(p.detach()), _bits(q.detach()))
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(_bits(opt.state[p][name]), _bits(eager.state[q][name])), name
        assert int(opt.state[p]["step"]) == int(eager.state[q]["step"]) == 3
    # the graph is a chain of the two kernels: no node has two successors or two predecessors
    nodes, edges = _graph_nodes_and_edges(graph)
    assert nodes == 2 and len(edges) == 1, (nodes, edges)
    assert len({a for a, _ in edges}) == len(edges) == len({b for _, b in edges}), edges


# ---- through the model --------------------------------------------------------------------------------------------------
N_SEEN, N_UNSEEN = 300, 20


def _model(device, **kw):
    """synthetic.py's blob, drawn in to half its extent, in front of one 64 x 48 camera of its ring, plus 20 Gaussians behind
    that camera, which it does not see."""
    from simplegaussiansplat_tk71_amd import synthetic

    P, K, wh = (t[:1].contiguous() for t in synthetic.ring_cameras(8, 64, 48, device=device))
    mean, q, scale, op = synthetic.make_world(N_SEEN + N_UNSEEN, 64, sigma_px=1.5, seed=0, device=device)
    eye = -(P[0, :, :3].T @ P[0, :, 3])
    behind = 10.0 * eye / eye.norm() + 0.3 * torch.randn(N_UNSEEN, 3, generator=torch.Generator().manual_seed(1)).to(device)
    mean = torch.cat((0.5 * mean[:N_SEEN], behind))
    model = gm.GS_model_with_param(mean, q, scale, op, **kw)
    with torch.no_grad():
        model.color[:, 0, :] = 0.5 + 2.0 * torch.rand(model.color.shape[0], 3, generator=torch.Generator().manual_seed(5)).to(device)
    return model, P, K, wh


def _one_step(model, P, K, wh, target):
    """forward / backward / train_step(visible=grad_iter) with the MCMC regularisers, which give every row a gradient."""
    images, _, grad_iter = model(P, K, wh, [0])
    loss = gm.splat_loss(images, target, 0.2) + 0.01 * torch.sigmoid(model.opacity).mean() + 0.01 * torch.exp(model.variance_scale).mean()
    loss.backward()
    model.train_step(visible=grad_iter)
    return grad_iter


def test_sparse_model_step_moves_only_the_rows_the_camera_saw(device):
    target = torch.rand(1, 3, 48, 64, generator=torch.Generator().manual_seed(2)).to(device)
    sparse, P, K, wh = _model(device, adam="sparse")
    fused, _, _, _ = _model(device, adam="fused")
    start = {k: p.detach().clone() for k, p in sparse.named_parameters()}
    seen = _one_step(sparse, P, K, wh, target)
    assert torch.equal(seen, _one_step(fused, P, K, wh, target))
    assert seen.dtype == torch.bool and not seen[N_SEEN:].any() and int(seen.sum()) >= N_SEEN // 2
    moved = False
    for (k, p), (_, q) in zip(sparse.named_parameters(), fused.named_parameters()):
        s, f = sparse._optimizer.state[p], fused._optimizer.state[q]
        assert torch.equal(_bits(p.detach()[~seen]), _bits(start[k][~seen])), k
        assert not _bits(s["exp_avg"][~seen]).any() and not _bits(s["exp_avg_sq"][~seen]).any(), k
        for got, want in ((p.detach(), q.detach()), (s["exp_avg"], f["exp_avg"]), (s["exp_avg_sq"], f["exp_avg_sq"])):
            assert torch.equal(_bits(got[seen]), _bits(want[seen])), k
        assert int(s["step"]) == int(f["step"]) == 1
        moved |= not torch.equal(q.detach()[~seen], start[k][~seen])
    assert moved  # the regularisers do move unseen rows under the dense step: the mask is what held them
    with pytest.raises(RuntimeError):
        sparse.train_step()
    with pytest.raises(ValueError):
        _model(device, adam="other")


def test_fused_model_keeps_its_device_steps_through_the_density_passes(device):
    model, P, K, wh = _model(device, adam="fused")
    gen = torch.Generator().manual_seed(3)

    def step():
        for p in model.parameters():
            p.grad = (0.01 * torch.randn(p.shape, generator=gen)).to(device)
        model.train_step(visible=torch.zeros(model.mean.shape[0], dtype=torch.bool, device=device))  # ignored by "fused"

    step()
    assert all(int(model._optimizer.state[p]["step"]) == 1 for p in model.parameters())
    _, n = model.densify_and_prune_device(3.0, seed=1)
    _, n = model.relocate_and_grow_device(seed=2, cap_max=n + 16)
    keep = torch.ones(n, dtype=torch.bool, device=device)
    keep[::7] = False
    _, n = model.prune_rows(keep)
    assert model.mean.shape[0] == n and isinstance(model._optimizer, gm.HipAdam) and model._optimizer.fused
    assert all(torch.is_tensor(model._optimizer.state[p]["step"]) and int(model._optimizer.state[p]["step"]) == 1 for p in model.parameters())
    step()
    for p in model.parameters():
        st = model._optimizer.state[p]
        assert st["step"].dtype == torch.int32 and st["step"].is_cuda and int(st["step"]) == 2
        assert st["exp_avg"].shape == p.shape and bool(torch.isfinite(p.detach()).all())
