"""The yardstick of the exposure tests: the compensation as one einsum, followed by the PyTorch formulation of the loss
(oracle/loss_torch.py, imported and unchanged), in the dtype of its arguments.  Not a test module."""
import torch

from oracle import loss_torch


def compensate(x, E):
    """y = E[:, :, :3] x + E[:, :, 3] of (B, 3, H, W) `x` and (B, 3, 4) `E`."""
    return torch.einsum("bck,bkhw->bchw", E[..., :3], x) + E[..., 3, None, None]


def splat_loss(x, b, lamda, E):
    return loss_torch.splat_loss(compensate(x, E), b, lamda)


def ssim(x, b, E):
    return loss_torch.ssim(compensate(x, E), b, max_val=1.0, window_size=11)
