"""Per-camera exposure compensation: one learned 3 x 4 colour affine per training image, applied to the render inside the
loss kernels (`loss.splat_loss(exposure=)`, csrc/gcp_loss.hip) and trained with its own Adam group — the remedy upstream
3DGS added in 2024 for photographs of one scene that differ in exposure and white balance.

The matrices are NOT parameters of `GS_model_with_param`: its optimiser and every densify, prune or relocate pass walk
`named_parameters(recurse=False)` and expect one row per Gaussian.  `CameraExposure` is a module of its own with one row per
camera.

Gauge freedom: scene brightness times exposure gain is not pinned — a scene twice as bright under half the gain has the same
loss — as upstream does not pin it either.  No regulariser is added."""
import json

import torch

from .optim import HipAdam


class CameraExposure(torch.nn.Module):
    """`matrix` (n_cameras, 3, 4), initialised to [I | 0]: the compensated render of camera i is
    y_c = matrix[i, c, 0] x_0 + matrix[i, c, 1] x_1 + matrix[i, c, 2] x_2 + matrix[i, c, 3].
    `names`: the image name of every camera (default: the zero-padded index), the keys of `save_json` / `load_json`.
    `lr_init`, `lr_final`, `max_steps`: the log-linear decay of the learning rate (`gs_model.get_expon_lr_func`) from 0.01 to
    0.001 over 30 000 steps — the published values of upstream 3DGS, not tuned here."""

    def __init__(self, n_cameras, names=None, device="cpu", lr_init=0.01, lr_final=0.001, max_steps=30_000):
        super().__init__()
        from .gs_model import get_expon_lr_func

        n_cameras = int(n_cameras)
        if n_cameras < 0:
            raise ValueError(f"n_cameras: >= 0, got {n_cameras}")
        self.names = [f"{i:06d}" for i in range(n_cameras)] if names is None else [str(n) for n in names]
        if len(self.names) != n_cameras or len(set(self.names)) != n_cameras:
            raise ValueError(f"names: {n_cameras} distinct entries expected, got {len(self.names)} ({len(set(self.names))} distinct)")
        start = torch.zeros(n_cameras, 3, 4, dtype=torch.float32, device=device)
        start[:, 0, 0] = start[:, 1, 1] = start[:, 2, 2] = 1.0
        self.matrix = torch.nn.Parameter(start)
        self.lr_func = get_expon_lr_func(lr_init, lr_final, max_steps=max_steps)
        self.lr = self.lr_func(0)
        self.optimizer = HipAdam([{"params": [self.matrix], "lr": self.lr, "name": "exposure"}], fused=True)

    def __len__(self):
        return self.matrix.shape[0]

    def _index(self, cameras):
        """`cameras` (a list or tensor of camera numbers) as an int64 tensor on the matrices' device; a camera twice raises."""
        idx = torch.as_tensor(cameras, dtype=torch.int64).reshape(-1)
        listed = idx.tolist()
        if len(set(listed)) != len(listed):
            raise ValueError(f"a camera twice in one call: {listed}")
        if listed and (min(listed) < 0 or max(listed) >= len(self)):
            raise IndexError(f"cameras {listed}: expected numbers in 0..{len(self) - 1}")
        return idx.to(self.matrix.device)

    def rows(self, cameras):
        """The (B, 3, 4) matrices of `cameras`, in order, by `index_select` (differentiable: its backward scatters into
        `matrix.grad`).  A camera twice in one call raises, so that scatter adds nothing to anything and stays
        deterministic."""
        return self.matrix.index_select(0, self._index(cameras))

    def mask(self, cameras):
        """A device bool over all cameras, true at `cameras`; a bool tensor of that shape is passed through."""
        if torch.is_tensor(cameras) and cameras.dtype == torch.bool:
            if cameras.shape != (len(self),):
                raise ValueError(f"a camera mask has one entry per camera ({len(self)}), got {tuple(cameras.shape)}")
            return cameras.to(self.matrix.device)
        m = torch.zeros(len(self), dtype=torch.bool, device=self.matrix.device)
        m[self._index(cameras)] = True
        return m

    def set_lr(self, iteration):
        """The learning rate of the step after `iteration` steps, as `GS_model_with_param.set_mean_lr`."""
        self.lr = self.lr_func(iteration)
        for group in self.optimizer.param_groups:
            group["lr"] = self.lr
        return self.lr

    def step(self, cameras):
        """One Adam step (`HipAdam(fused=True)`, csrc/gcp_optim.hip) on the rows of `cameras` (camera numbers, or the bool mask
        `allreduce_grads` returns), then `zero_grad`.  The cameras outside keep their matrix and both moments bit for bit —
        the row mask of the sparse Adam.  The step count is shared by all rows and advances with every call: the bias
        correction is global, not per camera, so a camera first drawn late starts with a correction close to 1.  GPU only."""
        if self.matrix.grad is not None:
            self.optimizer.step(visible=self.mask(cameras))
        self.optimizer.zero_grad()

    def allreduce_grads(self, cameras, group=None):
        """Sums `matrix.grad` over the ranks and ORs the mask of `cameras` (this rank's share of the batch) -> the bool mask
        of the cameras any rank drew, for `step`.  Each camera is drawn by one rank per step, so the sum adds zeros to that
        rank's rows and keeps their bits.  Under backend "gloo" through the host, as `GS_model_with_param.allreduce_grads`."""
        import torch.distributed as dist

        grad = self.matrix.grad if self.matrix.grad is not None else torch.zeros_like(self.matrix)
        seen = self.mask(cameras).to(torch.uint8)
        out = []
        for t, op in ((grad.contiguous(), dist.ReduceOp.SUM), (seen, dist.ReduceOp.MAX)):
            if t.is_cuda and dist.get_backend(group) == "gloo":
                host = t.cpu()
                dist.all_reduce(host, op=op, group=group)
                t = host.to(t.device)
            else:
                dist.all_reduce(t, op=op, group=group)
            out.append(t)
        self.matrix.grad = out[0]
        return out[1].bool()

    def save_json(self, path):
        """One object, image name -> 3 x 4 nested list: the `exposure.json` layout other trainers write.  The float32 values
        are written as the doubles they equal, so `load_json` restores their bits."""
        values = self.matrix.detach().cpu().double().tolist()
        with open(path, "w") as f:
            json.dump(dict(zip(self.names, values)), f, indent=1)

    def load_json(self, path):
        """Reads what `save_json` wrote into `matrix`.  The file must hold exactly this module's names: an unknown or a
        missing name raises, as does an entry that is not 3 x 4."""
        with open(path) as f:
            data = json.load(f)
        if not isinstance(data, dict):
            raise ValueError(f"{path}: expected one object, image name -> 3 x 4 list")
        unknown, missing = sorted(set(data) - set(self.names)), [n for n in self.names if n not in data]
        if unknown or missing:
            raise KeyError(f"{path}: unknown names {unknown}, missing names {missing}")
        if not self.names:
            return
        values = torch.tensor([data[n] for n in self.names], dtype=torch.float64)
        if tuple(values.shape) != (len(self), 3, 4):
            raise ValueError(f"{path}: every entry must be a 3 x 4 list")
        with torch.no_grad():
            self.matrix.copy_(values.to(torch.float32))
