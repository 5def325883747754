"""The float64 formulation of the fused, row-masked Adam step (include/grouped_cumprod_hip.h, gcp_adam_step_multi), which the
kernels of csrc/gcp_optim.hip are tested against: masked Adam over a list of [rows, width] tensors, the per-element bounds
of its three outputs, and the states and masks the tests draw.  CPU tensors throughout."""
import math

import torch

EPS = 2.0 ** -23
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8
WIDTHS = (3, 4, 3, 1, 27)  # mean, variance_q, variance_scale, opacity, colour of degree 2 (degree 3: 48)


def reference(p, g, m, v, step, lr):
    """Float64 Adam from the fp32 inputs and the per-element bounds of the three outputs (tests/test_adam_gpu.py::_reference).
    With S = |b1 m| + |(1 - b1) g|: the first moment is two rounded products and a rounded sum; the second moment the same of
    positive terms (a denormal result may be flushed); the parameter one rounding of itself and the rounded update, whose
    scalar lr / bc1 is rounded once."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    m2, v2 = B1 * m + (1 - B1) * g, B2 * v + (1 - B2) * g * g
    bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
    denom = v2.sqrt() / math.sqrt(bc2) + ADAM_EPS
    p2 = p - (lr / bc1) * m2 / denom
    s = (B1 * m).abs() + ((1 - B1) * g).abs()
    return (p2, m2, v2), (EPS * p2.abs() + 8 * EPS * (lr / bc1) * s / denom, 4 * EPS * s, 4 * EPS * v2 + 2.0 ** -125)


def masked_adam(tensors, steps, lrs, visible=None):
    """One step over a list of (p, g, m, v), each [rows, width] float32; steps[t] = the step being taken, lrs[t] its rate;
    visible: None or a [rows] mask, non-zero = visible.  -> per tensor ((p2, m2, v2), (bounds), rows_on): float64 results
    and bounds as `reference`; on a row outside the mask the result is the input and the bound 0 (the test compares bits)."""
    out = []
    for (p, g, m, v), step, lr in zip(tensors, steps, lrs):
        want, bounds = reference(p, g, m, v, step, lr)
        on = torch.ones(p.shape[0], dtype=torch.bool) if visible is None else visible != 0
        sel = on.reshape(-1, *([1] * (p.dim() - 1))).expand_as(p)
        want = tuple(torch.where(sel, w, old.double()) for w, old in zip(want, (p, m, v)))
        bounds = tuple(torch.where(sel, b, torch.zeros_like(b)) for b in bounds)
        out.append((want, bounds, on))
    return out


def worst(got, want, bounds, keep=None, what=""):
    """Asserts |got - want| <= bound per element (where `keep`); returns the worst error / bound of (p, m, v)."""
    ratios = []
    for name, a, w, b in zip("pmv", got, want, bounds):
        err = (a.double() - w).abs()
        ok = err <= b  # False for NaN
        if keep is not None:
            ok = ok | ~keep
            err = torch.where(keep, err, torch.zeros_like(err))
        bad = (~ok).reshape(-1).nonzero()
        assert bad.numel() == 0, (what, name, "first index outside the bound", bad[0].item(), "of", bad.shape[0],
                                  a.reshape(-1)[bad[0]].item(), w.reshape(-1)[bad[0]].item(), b.reshape(-1)[bad[0]].item())
        ratios.append((err / b.clamp_min(1e-300)).max().item() if err.numel() else 0.0)
    return ratios


def log_uniform(n, lo, hi, gen, signed=True):
    x = 10.0 ** (lo + (hi - lo) * torch.rand(n, generator=gen))
    return x * (1 - 2 * torch.randint(0, 2, (n,), generator=gen)) if signed else x


def state(rows, width, gen):
    """(p, g, m, v) [rows, width] in the ranges of tests/test_adam_gpu.py::_state: parameters 1e-4 .. 1e2, gradients and first
    moments 1e-20 .. 1e4 (signed), second moments 1e-24 .. 1e8."""
    n = rows * width
    return tuple(t.reshape(rows, width) for t in (log_uniform(n, -4, 2, gen), log_uniform(n, -20, 4, gen), log_uniform(n, -20, 4, gen),
                                                  log_uniform(n, -24, 8, gen, signed=False)))


def torch_step(p, g, m, v, step, lr):
    """The same step by torch.optim.Adam in float32 on the CPU."""
    q = p.clone().requires_grad_(True)
    q.grad = g.clone()
    opt = torch.optim.Adam([q], lr=lr, betas=(B1, B2), eps=ADAM_EPS, foreach=False)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]


def masks(rows, value=1):
    """name -> uint8 [rows] with `value` where visible: all, none, alternating, only the first, only the last row, runs of 64
    and of 300 rows (visible, invisible, visible, ...: whole waves skip, and float4s straddle both ends of a run)."""
    idx = torch.arange(rows)
    named = {"ones": idx >= 0, "zeros": idx < 0, "alternating": idx % 2 == 0, "first": idx == 0, "last": idx == rows - 1,
             "runs64": (idx // 64) % 2 == 0, "runs300": (idx // 300) % 2 == 1}
    return {k: (m.to(torch.uint8) * value) for k, m in named.items()}
