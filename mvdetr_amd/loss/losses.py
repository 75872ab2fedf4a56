"""MVDeTr's detection losses (the reference's loss/losses.py:17-79 by name and call signature).

FocalLoss and RegL1Loss take two routes.  CUDA fp32 / fp64 tensors run csrc/detection_loss.hip: one launch forward and one
backward per call, no host synchronise, the loss a 0-dim device tensor; focal_loss_segments() / reg_l1_loss_segments() put
several maps (different shapes, targets, weights) into the SAME launch, which is how train.MVDeTrCriterion gets the whole
objective in two launches each way.  Everything else -- CPU tensors, other dtypes, ``MVDETR_LOSS_FUSION=0`` in the
environment or set_loss_fusion(False) -- runs the torch compositions below.  RegCELoss is a torch composition everywhere."""
from __future__ import annotations

import ctypes
import os

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from .. import _lib

_enabled = os.environ.get("MVDETR_LOSS_FUSION", "1") != "0"
P_MIN = 1e-4


def set_loss_fusion(on: bool) -> bool:
    """Switch the HIP losses on or off for this process (default on; ``MVDETR_LOSS_FUSION=0`` starts with them off).
    Returns the previous setting.  Off: every loss is the torch composition."""
    global _enabled
    prev, _enabled = _enabled, bool(on)
    return prev


def loss_fusion_enabled() -> bool:
    return _enabled


def last_kernel() -> str:
    """Name of the kernel the last fused loss call of this process launched ("none" before the first)."""
    return _lib.lib().mvdetr_loss_last_kernel().decode()


def launch_count() -> int:
    """Number of fused loss launches of this process so far."""
    return int(_lib.lib().mvdetr_loss_launch_count())


def fused_loss_available(x) -> bool:
    """True when a loss over this head output runs the HIP kernels: the switch is on and x is a 4-d CUDA fp32 / fp64 tensor."""
    return (_enabled and isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.numel() > 0
            and x.dtype in (torch.float32, torch.float64))


# ---- torch compositions ---------------------------------------------------------------------------------------------------

def focal_loss_composed(output, target, mask=None):
    p = output.sigmoid().clamp(P_MIN, 1 - P_MIN)
    target = target.to(output.device)
    positive, negative = target == 1, target < 1
    pos_term = torch.where(positive, p.log() * (1 - p) ** 2, p.new_zeros(()))
    neg_term = torch.where(negative, (1 - p).log() * p ** 2 * (1 - target) ** 4, p.new_zeros(()))
    if mask is not None:
        neg_term = neg_term * mask.to(output.device)
    num_pos = positive.sum()
    # no branch on the host: with no positive the positive term is zero and the divisor becomes 1
    return -(pos_term.sum() + neg_term.sum()) / num_pos.clamp(min=1).to(p.dtype)


def gather_positions(output, ind):
    """pred[b, k, c] = output[b, c, ind[b, k]] (ind = y * W + x)."""
    B, C = output.shape[:2]
    return output.flatten(2).gather(2, ind.to(output.device)[:, None, :].expand(B, C, ind.shape[1])).transpose(1, 2)


def reg_l1_loss_composed(output, mask, ind, target):
    pred = gather_positions(output, ind)
    m = mask.to(output.device)[:, :, None].expand_as(pred).float()
    target = target.to(output.device)
    return (pred * m - target * m).abs().sum() / (m.sum() + 1e-4)


# ---- the HIP route ---------------------------------------------------------------------------------------------------------

_counters = {}


def _ticket_counters(device, stream_ptr):
    # zero when handed to a launch and zero again when it ends, so one buffer per stream serves every call
    key = (device.index, stream_ptr)
    buf = _counters.get(key)
    if buf is None:
        buf = _counters[key] = torch.zeros(_lib.LOSS_MAX_SEGMENTS + 1, dtype=torch.int32, device=device)
    return buf


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _check_segments(first, xs, what):
    if not 1 <= len(xs) <= _lib.LOSS_MAX_SEGMENTS:
        raise ValueError(f"{what}: 1 to {_lib.LOSS_MAX_SEGMENTS} segments per call, got {len(xs)}")
    for x in xs:
        if not fused_loss_available(x):
            raise RuntimeError(f"{what}: these arguments do not take the HIP kernels (see fused_loss_available)")
        if x.dtype != first.dtype or x.device != first.device:
            raise RuntimeError(f"{what}: every segment must share one dtype and device")


class _FocalSegments(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, *tensors):
        n = len(weights)
        xs, ts, ms = tensors[:n], tensors[n:2 * n], tensors[2 * n:]
        dev, dtype = xs[0].device, xs[0].dtype
        segs = (_lib.FocalSegment * n)()
        for s, (x, t, m) in enumerate(zip(xs, ts, ms)):
            B, C, H, W = x.shape
            segs[s].logits, segs[s].target, segs[s].mask, segs[s].grad = x.data_ptr(), t.data_ptr(), _ptr(m), 0
            segs[s].stride = segs[s].grad_stride = (ctypes.c_int64 * 4)(*x.stride())
            segs[s].batch, segs[s].channels, segs[s].height, segs[s].width = B, C, H, W
            segs[s].weight = float(weights[s])
        lib = _lib.lib()
        nbytes = lib.mvdetr_focal_loss_workspace_bytes(segs, n, xs[0].element_size())
        if nbytes < 0:
            raise RuntimeError("focal_loss: bad segment description")
        work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        out = torch.empty(n + 1, dtype=dtype, device=dev)
        stats = torch.empty(n, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            stream = _lib.current_stream_ptr(dev)
            code = getattr(lib, "mvdetr_focal_loss_forward_" + _lib.suffix(dtype))(
                stream, segs, n, work.data_ptr(), _ticket_counters(dev, stream).data_ptr(), out.data_ptr(), stats.data_ptr())
        _lib.check(code, "focal_loss forward")
        ctx.save_for_backward(stats, *tensors)
        ctx.weights, ctx.segs = weights, segs
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        stats, *tensors = ctx.saved_tensors
        n, segs = len(ctx.weights), ctx.segs
        xs = tensors[:n]
        grad_out = grad_out.contiguous()
        grads = []
        for s, x in enumerate(xs):
            g = torch.empty_like(x) if ctx.needs_input_grad[1 + s] else None           # the input's own layout
            grads.append(g)
            segs[s].grad = _ptr(g)
            if g is not None:
                segs[s].grad_stride = (ctypes.c_int64 * 4)(*g.stride())
        dev = xs[0].device
        with torch.cuda.device(dev):
            code = getattr(_lib.lib(), "mvdetr_focal_loss_backward_" + _lib.suffix(xs[0].dtype))(
                _lib.current_stream_ptr(dev), segs, n, grad_out.data_ptr(), stats.data_ptr())
        _lib.check(code, "focal_loss backward")
        return (None, *grads) + (None,) * (2 * n)


class _L1Segments(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, *tensors):
        n = len(weights)
        xs, ms, inds, ts = (tensors[i * n:(i + 1) * n] for i in range(4))
        dev, dtype = xs[0].device, xs[0].dtype
        segs = (_lib.L1Segment * n)()
        for s, (x, m, ind, t) in enumerate(zip(xs, ms, inds, ts)):
            B, C, H, W = x.shape
            segs[s].output, segs[s].mask, segs[s].ind, segs[s].target, segs[s].grad = (
                x.data_ptr(), m.data_ptr(), ind.data_ptr(), t.data_ptr(), 0)
            segs[s].stride = segs[s].grad_stride = (ctypes.c_int64 * 4)(*x.stride())
            segs[s].batch, segs[s].channels, segs[s].height, segs[s].width, segs[s].k = B, C, H, W, ind.shape[1]
            segs[s].weight = float(weights[s])
        out = torch.empty(n + 1, dtype=dtype, device=dev)
        stats = torch.empty(n, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            code = getattr(_lib.lib(), "mvdetr_reg_l1_loss_forward_" + _lib.suffix(dtype))(
                _lib.current_stream_ptr(dev), segs, n, out.data_ptr(), stats.data_ptr())
        _lib.check(code, "reg_l1_loss forward")
        ctx.save_for_backward(stats, *tensors)
        ctx.weights, ctx.segs = weights, segs
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        stats, *tensors = ctx.saved_tensors
        n, segs = len(ctx.weights), ctx.segs
        xs = tensors[:n]
        grad_out = grad_out.contiguous()
        grads = []
        for s, x in enumerate(xs):
            g = torch.empty_like(x) if ctx.needs_input_grad[1 + s] else None
            grads.append(g)
            segs[s].grad = _ptr(g)
            if g is not None:
                segs[s].grad_stride = (ctypes.c_int64 * 4)(*g.stride())
        dev = xs[0].device
        with torch.cuda.device(dev):
            code = getattr(_lib.lib(), "mvdetr_reg_l1_loss_backward_" + _lib.suffix(xs[0].dtype))(
                _lib.current_stream_ptr(dev), segs, n, grad_out.data_ptr(), stats.data_ptr())
        _lib.check(code, "reg_l1_loss backward")
        return (None, *grads) + (None,) * (3 * n)


def _side(t, x, dtype, shape, what):
    """A target-side tensor on x's device (asynchronous copy when it is not there yet), dense, of the given dtype."""
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.to(device=x.device, dtype=dtype, non_blocking=True).contiguous()


def focal_loss_segments(outputs, targets, masks=None, weights=None):
    """Focal loss of several heat maps in ONE launch.  Returns a [n + 1] tensor: the n losses, then sum_s weights[s] * loss_s
    (weights default to 1).  Every output must pass fused_loss_available()."""
    n = len(outputs)
    _check_segments(outputs[0] if n else None, outputs, "focal_loss_segments")
    masks = [None] * n if masks is None else list(masks)
    weights = (1.0,) * n if weights is None else tuple(float(w) for w in weights)
    ts = [_side(t, x, x.dtype, x.shape, "focal target") for x, t in zip(outputs, targets)]
    ms = [None if m is None else _side(m, x, x.dtype, x.shape, "focal mask") for x, m in zip(outputs, masks)]
    return _FocalSegments.apply(weights, *outputs, *ts, *ms)


def reg_l1_loss_segments(outputs, masks, inds, targets, weights=None):
    """Masked L1 of several regression maps in ONE launch; returns [n + 1] as focal_loss_segments() does."""
    n = len(outputs)
    _check_segments(outputs[0] if n else None, outputs, "reg_l1_loss_segments")
    weights = (1.0,) * n if weights is None else tuple(float(w) for w in weights)
    ms, ids, ts = [], [], []
    for x, m, ind, t in zip(outputs, masks, inds, targets):
        B, C, K = x.shape[0], x.shape[1], ind.shape[-1]
        if K > 1024:
            raise ValueError("reg_l1_loss: at most 1024 slots per map")
        ms.append(_side(m, x, torch.bool, (B, K), "L1 mask").view(torch.uint8))
        ids.append(_side(ind, x, torch.int64, (B, K), "L1 ind"))
        ts.append(_side(t, x, x.dtype, (B, K, C), "L1 target"))
    return _L1Segments.apply(weights, *outputs, *ms, *ids, *ts)


class FocalLoss(nn.Module):
    """CornerNet focal loss on logits: p = clamp(sigmoid(output), 1e-4, 1 - 1e-4); positives are target == 1, negatives
    target < 1 weighted by (1 - target)^4; the optional mask multiplies the negative term only; the sum is divided by the
    number of positives of the whole call (not divided when there is none).

    On the HIP route target and mask must have exactly the logits' shape (ValueError otherwise: the kernel addresses them
    element for element); the torch composition broadcasts them as torch's operators do."""

    def forward(self, output, target, mask=None):
        if fused_loss_available(output):
            return focal_loss_segments([output], [target], [mask])[0]
        return focal_loss_composed(output, target, mask)


class RegL1Loss(nn.Module):
    """sum |pred m - target m| / (C sum m + 1e-4) with pred[b, k, c] = output[b, c, ind[b, k]]."""

    def forward(self, output, mask, ind, target):
        if fused_loss_available(output):
            return reg_l1_loss_segments([output], [mask], [ind], [target])[0]
        return reg_l1_loss_composed(output, mask, ind, target)


class RegCELoss(nn.Module):
    """Cross entropy of the gathered class scores over the masked slots, summed, over (sum m + 1e-4); 0 for an empty
    selection.  A torch composition on every device (the training objective does not use it)."""

    def forward(self, output, mask, ind, target):
        mask, target = mask.to(output.device), target.to(output.device)
        pred = gather_positions(output, ind)
        if int(mask.sum()) == 0:
            return 0
        return F.cross_entropy(pred[mask], target[mask], reduction="sum") / (mask.sum() + 1e-4)

