"""GaussianMSE (named and called as the reference's loss/gaussian_mse.py): mean squared error against a target that is
max-pooled to the prediction's size and then smoothed with a given kernel.  A torch composition on every device; the
training objective does not use it."""
import torch
import torch.nn.functional as F
from torch import nn


@torch.no_grad()
def smoothed_target(target, kernel, size):
    """target [B, 1, h, w] max-pooled to `size`, then correlated with the [1, 1, k, k] fp32 taps at the same size (odd k).
    A constant of the loss: nothing here is differentiated."""
    taps = torch.as_tensor(kernel, dtype=torch.float32, device=target.device)
    reach = (taps.shape[-1] - 1) // 2
    return F.conv2d(F.adaptive_max_pool2d(target, tuple(size)), taps, padding=reach)


class GaussianMSE(nn.Module):
    def forward(self, x, target, kernel):
        return (x - smoothed_target(target, kernel, x.shape[-2:])).square().mean()
