"""The optimiser step on the HIP library (csrc/gcp_optim.hip)."""
import torch

from . import _lib


class HipAdam:
    """torch.optim.Adam's update (default betas / eps, no weight decay, no amsgrad — what the reference constructs at
    gs_model.py:43-47) on the HIP library: one streaming kernel per parameter tensor (csrc/gcp_optim.hip, gcp_adam_step)
    instead of torch's multi-tensor launches (0.38 -> 0.2 ms per step at 10^6 Gaussians).  Same interface as far as the
    model uses it: `param_groups` with one tensor and an `lr` each, `step()`, `zero_grad()`."""

    def __init__(self, param_groups, betas=(0.9, 0.999), eps=1e-8):
        self.param_groups = [dict(g, params=list(g["params"]) if isinstance(g["params"], (list, tuple)) else [g["params"]])
                             for g in param_groups]
        self.betas, self.eps = betas, eps
        self.state = {}

    @torch.no_grad()
    def step(self):
        lib = _lib.load()
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("HipAdam updates contiguous float32 GPU tensors")
                st = self.state.setdefault(p, {"step": 0, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)})
                st["step"] += 1
                grad = p.grad.contiguous()
                with torch.cuda.device(p.device):
                    _lib.check(lib.gcp_adam_step(p.data_ptr(), grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                                 p.numel(), float(group["lr"]), self.betas[0], self.betas[1], self.eps, st["step"],
                                                 torch.cuda.current_stream(p.device).cuda_stream), "gcp_adam_step")

    def zero_grad(self, set_to_none=True):
        for group in self.param_groups:
            for p in group["params"]:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()
