"""The Adam kernel (csrc/gcp_optim.hip, optim.py) against float64 Adam, per element: one step from arbitrary states over
the whole dynamic range, tensors past one grid of the grid-stride loop, rows that must not move, non-finite gradients,
and the optimiser's interface."""
import math

import pytest
import torch

from simplegaussiansplat_tk71_amd import _lib
from simplegaussiansplat_tk71_amd import gs_model as gm

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8
GRID = 16384 * 256 * 4  # floats one pass of k_adam covers: 16384 blocks of 256 threads, one float4 each


def _reference(p, g, m, v, step, lr):
    """Float64 Adam from the fp32 inputs (any device) and the per-element bounds of the three outputs.  With
    S = |b1 m| + |(1 - b1) g|: the first moment is two rounded products and a rounded sum; the second moment the same of
    positive terms (a denormal result may be flushed); the parameter one rounding of itself and the rounded update."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    m2, v2 = B1 * m + (1 - B1) * g, B2 * v + (1 - B2) * g * g
    bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
    denom = v2.sqrt() / math.sqrt(bc2) + ADAM_EPS
    p2 = p - (lr / bc1) * m2 / denom
    s = (B1 * m).abs() + ((1 - B1) * g).abs()
    return (p2, m2, v2), (EPS * p2.abs() + 8 * EPS * (lr / bc1) * s / denom, 4 * EPS * s, 4 * EPS * v2 + 2.0 ** -125)


def _worst(got, want, bounds, keep=None, what=""):
    """Asserts |got - want| <= bound per element (where `keep`); returns the worst error / bound of (p, m, v)."""
    worst = []
    for name, a, w, b in zip("pmv", got, want, bounds):
        err = (a.double() - w).abs()
        ok = err <= b  # False for NaN
        if keep is not None:
            ok = ok | ~keep
            err = torch.where(keep, err, torch.zeros_like(err))
        bad = (~ok).nonzero()
        assert bad.numel() == 0, (what, name, "first index outside the bound", bad[0].item(), "of", bad.shape[0],
                                  a.reshape(-1)[bad[0]].item(), w.reshape(-1)[bad[0]].item(), b.reshape(-1)[bad[0]].item())
        worst.append((err / b.clamp_min(1e-300)).max().item())
    return worst


def _log_uniform(n, lo, hi, gen, signed=True):
    x = 10.0 ** (lo + (hi - lo) * torch.rand(n, generator=gen))
    return x * (1 - 2 * torch.randint(0, 2, (n,), generator=gen)) if signed else x


def _state(n, gen):
    """Parameters 1e-4 .. 1e2, gradients and first moments 1e-20 .. 1e4 (signed), second moments 1e-24 .. 1e8."""
    return (_log_uniform(n, -4, 2, gen), _log_uniform(n, -20, 4, gen), _log_uniform(n, -20, 4, gen),
            _log_uniform(n, -24, 8, gen, signed=False))


def _hip_step(p, g, m, v, step, lr, device):
    """One HipAdam step from the given state; returns the new (p, m, v) on the CPU."""
    q = p.to(device).requires_grad_(True)
    q.grad = g.to(device)
    opt = gm.HipAdam([{"params": q, "lr": lr}])
    opt.state[q] = {"step": step - 1, "exp_avg": m.to(device), "exp_avg_sq": v.to(device)}
    opt.step()
    assert opt.state[q]["step"] == step
    return q.detach().cpu(), opt.state[q]["exp_avg"].cpu(), opt.state[q]["exp_avg_sq"].cpu()


def _torch_step(p, g, m, v, step, lr):
    """The same step by torch.optim.Adam in float32 on the CPU."""
    q = p.clone().requires_grad_(True)
    q.grad = g.clone()
    opt = torch.optim.Adam([q], lr=lr, betas=(B1, B2), eps=ADAM_EPS, foreach=False)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1027, 262_147])
def test_one_step_from_an_arbitrary_state_against_float64(n, device):
    """Every float4 lane, the scalar tail of one to three elements, one block and many; steps at which the bias
    corrections are far from and at 1; learning rates of the model and 1."""
    worst_hip, worst_torch = [0.0] * 3, [0.0] * 3
    for i, (step, lr) in enumerate((s, l) for s in (1, 2, 7, 1000, 30000) for l in (1e-2, 1.6e-4, 1.0)):
        p, g, m, v = _state(n, torch.Generator().manual_seed(100 * n + i))
        want, bounds = _reference(p, g, m, v, step, lr)
        # the guard: float32 torch.optim.Adam is inside the bounds, so a failure below is the kernel's
        worst_torch = list(map(max, worst_torch, _worst(_torch_step(p, g, m, v, step, lr), want, bounds, what=("float32 torch", step, lr))))
        worst_hip = list(map(max, worst_hip, _worst(_hip_step(p, g, m, v, step, lr, device), want, bounds, what=("kernel", step, lr))))
    print(f"B1 n {n}: worst error / bound (p, m, v) kernel {worst_hip[0]:.3f} {worst_hip[1]:.3f} {worst_hip[2]:.3f}, "
          f"float32 torch {worst_torch[0]:.3f} {worst_torch[1]:.3f} {worst_torch[2]:.3f}")


@pytest.mark.parametrize("n", [GRID, GRID + 4, GRID + 3072 + 3])
def test_two_steps_past_one_grid(n, device):
    """More than 16 777 216 floats: some threads take a second pass of the grid-stride loop (all 4, 1 and 768 float4 of a
    second pass; scalar tails of 0, 0 and 3).  Every element against float64 Adam after one step from zero moments and
    after a second from the resulting state: an element updated twice or never is off by orders of magnitude."""
    gen = torch.Generator(device=device).manual_seed(n % 9973)
    p = torch.randn(n, device=device, generator=gen).requires_grad_(True)
    opt = gm.HipAdam([{"params": p, "lr": 1e-2}])
    m, v = torch.zeros(n, device=device), torch.zeros(n, device=device)
    for step in (1, 2):
        g = torch.randn(n, device=device, generator=gen) * 0.1
        want, bounds = _reference(p.detach(), g, m, v, step, 1e-2)
        p.grad = g
        opt.step()
        m, v = opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
        worst = _worst((p.detach(), m, v), want, bounds, what=("step", step))
        print(f"B2 n {n} step {step}: worst error / bound (p, m, v) {worst[0]:.3f} {worst[1]:.3f} {worst[2]:.3f}")
        del want, bounds
        m, v = m.clone(), v.clone()
    assert opt.state[p]["step"] == 2


# positions in every float4 lane, the last full float4 and the three-element tail of 1027
N_EDGE = 1027
EDGE_INDICES = [0, 5, 10, 15, 512, 1020, 1021, 1022, 1023, 1024, 1025, 1026]


def test_rows_without_gradient_or_moments_do_not_move(device):
    """g = m = v = 0 leaves p bit-identical and the moments exactly zero: the model keeps rows that are not active yet
    in the optimiser."""
    for idx in (EDGE_INDICES, list(range(N_EDGE))):
        p, g, m, v = _state(N_EDGE, torch.Generator().manual_seed(len(idx)))
        p[7] = -0.0
        idx = torch.tensor(idx + [7])
        g[idx], m[idx], v[idx] = 0.0, 0.0, 0.0
        got_p, got_m, got_v = _hip_step(p, g, m, v, 3, 1e-2, device)
        assert torch.equal(got_p[idx].view(torch.int32), p[idx].view(torch.int32))
        assert torch.equal(got_m[idx].view(torch.int32), torch.zeros(len(idx), dtype=torch.int32))
        assert torch.equal(got_v[idx].view(torch.int32), torch.zeros(len(idx), dtype=torch.int32))
        want, bounds = _reference(p, g, m, v, 3, 1e-2)
        _worst((got_p, got_m, got_v), want, bounds)  # and the rows between them moved as they should


def test_non_finite_gradients_stay_local(device):
    p, g, m, v = _state(N_EDGE, torch.Generator().manual_seed(4))
    idx = torch.tensor(EDGE_INDICES)
    bad = torch.zeros(N_EDGE, dtype=torch.bool)
    bad[idx] = True
    g_bad = g.clone()
    g_bad[idx] = torch.tensor([float("inf"), float("nan"), -float("inf")]).repeat(len(idx) // 3 + 1)[:len(idx)]
    got = _hip_step(p, g_bad, m, v, 5, 1e-2, device)
    for t in got:
        assert torch.equal(~torch.isfinite(t), bad)
    want, bounds = _reference(p, g, m, v, 5, 1e-2)
    _worst(got, want, bounds, keep=~bad)


def test_optimiser_interface(device):
    gen = torch.Generator().manual_seed(11)
    a0, b0, ga, gb = (torch.randn(37, generator=gen) for _ in range(4))
    a, b, c = a0.to(device).requires_grad_(True), b0.to(device).requires_grad_(True), torch.ones(5, device=device, requires_grad=True)
    opt = gm.HipAdam([{"params": a, "lr": 1e-2}, {"params": [b, c], "lr": 1.6e-4}])
    a.grad, b.grad = ga.to(device), gb.to(device)
    opt.step()
    zero = torch.zeros(37)
    for q, q0, gq, lr in ((a, a0, ga, 1e-2), (b, b0, gb, 1.6e-4)):  # each group at its own learning rate
        want, bounds = _reference(q0, gq, zero, zero, 1, lr)
        _worst((q.detach().cpu(), opt.state[q]["exp_avg"].cpu(), opt.state[q]["exp_avg_sq"].cpu()), want, bounds, what=lr)
        assert (q.detach().cpu() - q0).abs().min().item() > 0.5 * lr
    assert c not in opt.state and torch.equal(c.detach().cpu(), torch.ones(5))  # no gradient: untouched, no state
    kept = a.grad
    opt.zero_grad(set_to_none=False)
    assert a.grad is kept and float(a.grad.abs().max()) == 0.0 and c.grad is None
    opt.zero_grad()
    assert a.grad is None and b.grad is None
    for k in range(2, 5):
        a.grad = ga.to(device)
        opt.step()
        assert opt.state[a]["step"] == k and opt.state[b]["step"] == 1

    # a gradient that is one expanded scalar (stride 0)
    for make_grad in (lambda q: q.sum().backward(), lambda q: setattr(q, "grad", torch.ones((), device=device).expand(37))):
        q = a0.to(device).requires_grad_(True)
        make_grad(q)
        one = gm.HipAdam([{"params": q, "lr": 1e-2}])
        one.step()
        want, bounds = _reference(a0, torch.ones(37), zero, zero, 1, 1e-2)
        _worst((q.detach().cpu(), one.state[q]["exp_avg"].cpu(), one.state[q]["exp_avg_sq"].cpu()), want, bounds)


def test_refused_parameters_stay_unchanged(device):
    base = torch.randn(4, 8, device=device)
    for make in (lambda: base.clone().t(),             # not contiguous
                 lambda: base.clone().double(),        # not float32
                 lambda: base.clone().reshape(-1)[1:]):  # contiguous, 4 bytes into its storage: not float4-aligned
        p = make().detach().requires_grad_(True)
        before = p.detach().clone()
        p.grad = torch.ones_like(p)
        with pytest.raises(RuntimeError):
            gm.HipAdam([{"params": p, "lr": 0.1}]).step()
        torch.cuda.synchronize(device)
        assert torch.equal(p.detach(), before)
    # the last of them is refused by the C entry point, and that refusal is what reaches Python
    p = base.clone().reshape(-1)[1:].detach().requires_grad_(True)
    assert p.is_contiguous() and p.dtype == torch.float32 and p.data_ptr() % 16 == 4
    p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="gcp_adam_step: invalid argument"):
        gm.HipAdam([{"params": p, "lr": 0.1}]).step()
    lib = _lib.load()
    whole = [torch.zeros(32, device=device) for _ in range(4)]
    for k in range(4):  # any one of param, grad, exp_avg, exp_avg_sq
        ptrs = [t[1:].data_ptr() if i == k else t.data_ptr() for i, t in enumerate(whole)]
        with torch.cuda.device(device):
            assert lib.gcp_adam_step(*ptrs, 31, 0.1, B1, B2, ADAM_EPS, 1, torch.cuda.current_stream(device).cuda_stream) == 1, k
    torch.cuda.synchronize(device)
    assert all(float(t.abs().max()) == 0.0 for t in whole)
