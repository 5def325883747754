"""The optimiser step on the HIP library (csrc/gcp_optim.hip)."""
import ctypes

import torch

from . import _lib

MAX_TENSORS = 8  # GCP_ADAM_MAX_TENSORS of the header


class HipAdam:
    """torch.optim.Adam's update (default betas / eps, no weight decay, no amsgrad — what the reference constructs at
    gs_model.py:43-47) on the HIP library: one streaming kernel per parameter tensor (csrc/gcp_optim.hip, gcp_adam_step)
    instead of torch's multi-tensor launches (0.38 -> 0.2 ms per step at 10^6 Gaussians).  Same interface as far as the
    model uses it: `param_groups` with one tensor and an `lr` each, `step()`, `zero_grad()`.

    fused=True: every parameter that has a gradient goes through ONE gcp_adam_step_multi call (two launches: a prologue
    that advances the step counts and forms the bias-corrected scalars on the device, and one kernel over all tensors; more
    than 8 tensors, or a parameter without gradient between others, split the call).  `state[p]["step"]` is then a 1-element
    int32 device tensor (a Python int found there is converted on first use) and the learning rates live in a device vector
    that is refreshed from `param_groups[i]["lr"]` with one small non-blocking copy when one of them has changed.
    `step(visible)` takes a row mask (bool or uint8 [rows] on the device, non-zero = visible): rows outside it keep their
    parameters and both moments bit for bit, while every step count advances — the sparse Adam of other 3DGS trainers.  All
    parameters of a masked step must share their leading dimension.

    Capture: after `init_state()` a fused `step()` inside `torch.cuda.graph` launches only the two kernels and allocates
    nothing (take one eager fused step somewhere before the capture, so that the kernels are loaded).  The graph holds the
    addresses of the gradients: keep the gradient buffers alive across replays with `zero_grad(set_to_none=False)` and copy
    or accumulate fresh gradients into them.  Learning rates are not refreshed while a stream captures; call `sync_lr()`
    between replays after changing one."""

    def __init__(self, param_groups, betas=(0.9, 0.999), eps=1e-8, fused=False):
        self.param_groups = [dict(g, params=list(g["params"]) if isinstance(g["params"], (list, tuple)) else [g["params"]])
                             for g in param_groups]
        self.betas, self.eps = betas, eps
        self.fused = bool(fused)
        self.state = {}
        self._lr = self._scal = self._lr_host = None  # fused: device float[n], device float[2 n], the rates last uploaded

    @torch.no_grad()
    def step(self, visible=None):
        if self.fused:
            return self._step_fused(visible)
        if visible is not None:
            raise RuntimeError("HipAdam: a row mask needs fused=True")
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

    # ---- fused=True ------------------------------------------------------------------------------------------------
    def _params(self):
        return [p for group in self.param_groups for p in group["params"]]

    def _state_of(self, p):
        """The state of `p` with a device step count; allocates what is missing (nothing after `init_state`)."""
        st = self.state.setdefault(p, {})
        step = st.get("step", 0)
        if not (torch.is_tensor(step) and step.device == p.device and step.dtype == torch.int32 and step.numel() == 1):
            st["step"] = torch.tensor([int(step)], dtype=torch.int32, device=p.device)
        for name in ("exp_avg", "exp_avg_sq"):
            if name not in st:
                st[name] = torch.zeros_like(p)
        return st

    def _rates(self, device, refresh):
        """The device vectors lr[n] and scal[2 n], one slot per parameter in `param_groups` order.  `refresh`: upload the
        rates if one differs from what the device holds."""
        rates = [float(group["lr"]) for group in self.param_groups for _ in group["params"]]
        if self._lr is None or self._lr.numel() != len(rates) or self._lr.device != device:
            self._lr = torch.empty(max(1, len(rates)), dtype=torch.float32, device=device)
            self._scal = torch.empty(2 * max(1, len(rates)), dtype=torch.float32, device=device)
            self._lr_host = None
        if refresh and rates and rates != self._lr_host:
            host = torch.empty(len(rates), dtype=torch.float32, pin_memory=True)  # from torch's pinned pool: reused once the copy is done
            host.copy_(torch.tensor(rates, dtype=torch.float32))
            self._lr[:len(rates)].copy_(host, non_blocking=True)
            self._lr_host = rates
        return self._lr, self._scal

    def init_state(self):
        """fused=True: allocate the moments and step counts of every parameter and the device rate vectors, and upload the
        rates, so that a captured `step()` allocates nothing."""
        if not self.fused:
            raise RuntimeError("HipAdam.init_state belongs to fused=True")
        params = self._params()
        for p in params:
            self._check(p)
            self._state_of(p)
        if params:
            self._rates(params[0].device, refresh=True)

    def sync_lr(self):
        """fused=True: upload `param_groups[i]["lr"]` to the device if one has changed (one non-blocking copy on the current
        stream); for use between replays of a captured step."""
        if not self.fused:
            raise RuntimeError("HipAdam.sync_lr belongs to fused=True")
        params = self._params()
        if params:
            with torch.cuda.device(params[0].device):
                self._rates(params[0].device, refresh=True)

    @staticmethod
    def _check(p):
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise RuntimeError("HipAdam updates contiguous float32 GPU tensors")
        if p.data_ptr() % 16:
            raise RuntimeError("gcp_adam_step_multi: invalid argument (a parameter is not 16-byte aligned)")

    def _step_fused(self, visible):
        params = self._params()
        active = [(i, p) for i, p in enumerate(params) if p.grad is not None]
        if not active:
            return
        device = active[0][1].device
        # every refusal before anything is launched
        for _, p in active:
            self._check(p)
            if p.device != device:
                raise RuntimeError("HipAdam(fused=True): all parameters must live on one device")
        grads = {p: p.grad.contiguous() for _, p in active}
        for p, g in grads.items():
            if g.dtype != torch.float32 or g.shape != p.shape or g.device != device or g.data_ptr() % 16:
                raise RuntimeError("HipAdam updates contiguous float32 GPU tensors (the gradient: same shape, 16-byte aligned)")
        if visible is not None:
            rows = {p.shape[0] if p.dim() else 1 for _, p in active}
            if len(rows) != 1:
                raise RuntimeError(f"HipAdam: a row mask needs parameters of one leading dimension, got {sorted(rows)}")
            if visible.dtype == torch.bool:
                visible = visible.view(torch.uint8)
            if (visible.dtype != torch.uint8 or visible.device != device or visible.shape != (rows.pop(),) or not visible.is_contiguous()):
                raise RuntimeError("HipAdam: the row mask is a contiguous bool or uint8 tensor with one entry per row, on the parameters' device")
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and (self._lr_host is None or any(not torch.is_tensor(self.state.get(p, {}).get("step")) for _, p in active)):
            raise RuntimeError("HipAdam: call init_state() before capturing a step (rates and step counts must be on the device)")
        lib = _lib.load()
        with torch.cuda.device(device):
            lr, scal = self._rates(device, refresh=not capturing)
            states = {p: self._state_of(p) for _, p in active}
            stream = torch.cuda.current_stream(device).cuda_stream
            # runs of consecutive parameters (the rate vector has one slot per parameter), at most MAX_TENSORS each
            start = 0
            while start < len(active):
                end = start + 1
                while end < len(active) and end - start < MAX_TENSORS and active[end][0] == active[end - 1][0] + 1:
                    end += 1
                run = [p for _, p in active[start:end]]
                first, k = active[start][0], len(run)
                ptrs = lambda ts: (ctypes.c_void_p * k)(*[t.data_ptr() for t in ts])  # noqa: E731
                if visible is None:
                    shape = [(p.numel(), 1) for p in run]
                else:
                    shape = [(p.shape[0], p.numel() // p.shape[0] if p.shape[0] else 1) if p.dim() else (1, 1) for p in run]
                _lib.check(lib.gcp_adam_step_multi(
                    k, ptrs(run), ptrs([grads[p] for p in run]), ptrs([states[p]["exp_avg"] for p in run]),
                    ptrs([states[p]["exp_avg_sq"] for p in run]), (ctypes.c_int64 * k)(*[s[0] for s in shape]),
                    (ctypes.c_int32 * k)(*[s[1] for s in shape]), ptrs([states[p]["step"] for p in run]), lr.data_ptr() + 4 * first,
                    scal.data_ptr() + 8 * first, None if visible is None else visible.data_ptr(), self.betas[0], self.betas[1], self.eps,
                    stream), "gcp_adam_step_multi")
                start = end

    def zero_grad(self, set_to_none=True):
        for group in self.param_groups:
            for p in group["params"]:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()
