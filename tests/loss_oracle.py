"""Restatement of the two detection losses and their input gradients in numpy, at a chosen precision (fp64 by default):
the formulas of the issue text, written out with the analytic derivative instead of autograd.  tests/test_loss.py pins it
to the goldens the reference's own modules produced; the GPU tests compare the kernels against it at full size, and run it
in fp32 to get the reference formula's own rounding error for the bars."""
import numpy as np
import torch

P_MIN = 1e-4
CLAMP_LOGIT = float(np.log((1 - P_MIN) / P_MIN))            # 9.21024: |logit| at which the sigmoid meets a clamp bound


def focal(x, target, mask=None, dtype=np.float64):
    """(loss, grad) of the focal loss on logits x [B, C, H, W]."""
    dt = np.dtype(dtype).type
    x, t0 = np.asarray(x).astype(dt), np.asarray(target)
    t = t0.astype(dt)
    m = np.ones_like(x) if mask is None else np.asarray(mask).astype(dt)
    with np.errstate(over="ignore"):
        s = dt(1) / (dt(1) + np.exp(-x))
    lo, hi = dt(P_MIN), dt(1 - P_MIN)
    p = np.clip(s, lo, hi)
    passes = ((s >= lo) & (s <= hi)).astype(dt)               # the clamp's derivative
    q = dt(1) - p
    pos, neg = (t == 1).astype(dt), (t < 1).astype(dt)
    # the weight is formed in the target's own precision (fp32 maps) by torch's pow, as the formula's torch.pow(1 - t, 4) is
    nw = ((1 - torch.from_numpy(np.ascontiguousarray(t0))) ** 4).numpy().astype(dt) * m
    pos_sum = (np.log(p) * q * q * pos).sum(dtype=dt)
    neg_sum = (np.log(q) * p * p * nw * neg).sum(dtype=dt)
    num_pos = pos.sum(dtype=dt)
    norm = num_pos if num_pos > 0 else dt(1)
    loss = -(pos_sum + neg_sum) / norm
    d_pos = (q * q / p - dt(2) * q * np.log(p)) * pos
    d_neg = (-p * p / q + dt(2) * p * np.log(q)) * nw * neg
    grad = -(d_pos + d_neg) * (p * q * passes) / norm
    return dt(loss), grad.astype(dt)


def reg_l1(x, mask, ind, target, dtype=np.float64):
    """(loss, grad) of the masked L1 at gathered positions; x [B, C, H, W], mask / ind [B, K], target [B, K, C].  The mask
    sum of the denominator is an fp32 sum at every precision, as `mask.float().sum() + 1e-4` makes it."""
    dt = np.dtype(dtype).type
    x, t = np.asarray(x).astype(dt), np.asarray(target).astype(dt)
    mask, ind = np.asarray(mask).astype(bool), np.asarray(ind)
    B, C, H, W = x.shape
    K = ind.shape[1]
    den = dt(np.float32(C * int(mask.sum())) + np.float32(1e-4))
    total = dt(0)
    grad = np.zeros_like(x)
    for b in range(B):
        for k in range(K):
            if not mask[b, k]:
                continue
            y, xx = divmod(int(ind[b, k]), W)
            for c in range(C):
                d = x[b, c, y, xx] - t[b, k, c]
                total += abs(d)
                grad[b, c, y, xx] += np.sign(d) / den
    return dt(total / den), grad


def clamp_band(x, half_width=2e-3):
    """Elements whose logit lies within half_width of +-logit(1e-4): the gradient is discontinuous there, so gradient
    comparisons between precisions leave them out."""
    return np.abs(np.abs(np.asarray(x, dtype=np.float64)) - CLAMP_LOGIT) <= half_width
