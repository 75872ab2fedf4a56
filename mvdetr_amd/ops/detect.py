"""Detection extraction where the maps live: world heat-map logits (+ offsets) -> ground-plane detections in one fused
decode + threshold + distance NMS (csrc/detect.hip; csrc/host_path.cpp for CPU tensors).

Replaces, for tensors that stay on the device, the tail of the reference's test loop (multiview_detector/trainer.py:121-135:
``mvdet_decode(sigmoid(heatmap.cpu()), offset.cpu())``, the ``cls_thres`` test and ``nms``): nothing here waits for the GPU and
nothing is read back -- the result is a fixed-capacity tensor per frame plus the number of valid rows, all on the device.

Tie rule (this library's; the reference's order among equal scores is that of an unstable ``torch.sort``): equal scores are
visited higher row-major cell index first.  On tie-free input the result is the reference's.
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import torch

from .. import _lib


class Detections(NamedTuple):
    """``bev_detect``'s result; everything lives on the inputs' device.  Rows of a frame are in kept order (descending
    score); rows at and after ``min(count, max_det)`` are zero."""
    xy: torch.Tensor        # [B, max_det, 2] ground-plane positions
    score: torch.Tensor     # [B, max_det]
    cell: torch.Tensor      # [B, max_det] int32 row-major index of the heat-map cell
    count: torch.Tensor     # [B] int32: the true number kept, also when it exceeds max_det


def _top_k(top_k) -> int:
    return 0 if top_k is None or math.isinf(top_k) or top_k <= 0 else min(int(top_k), 2 ** 31 - 1)


def _strides(t: torch.Tensor):
    return (ctypes.c_int64 * 4)(*t.stride())


def last_kernel() -> str:
    return _lib.lib().mvdetr_detect_last_kernel().decode()


def launch_count() -> int:
    return int(_lib.lib().mvdetr_detect_launch_count())


def bev_detect(world_heatmap, world_offset=None, *, world_reduce=4, cls_thres=0.4, dist_thres=20, top_k=float("inf"),
               indexing="xy", max_det=None) -> Detections:
    """world_heatmap [B,1,H,W] raw logits, world_offset [B,2,H,W] or None (cell centres), any strides (channels_last maps are
    read in place).  ``max_det=None`` means H*W, which cannot overflow.  Not differentiable."""
    hm = world_heatmap.detach()
    off = None if world_offset is None else world_offset.detach()
    if hm.dim() != 4 or hm.shape[1] != 1:
        raise RuntimeError(f"world_heatmap must be [B, 1, H, W], got {tuple(hm.shape)}")
    B, _, H, W = hm.shape
    if off is not None:
        if off.shape != (B, 2, H, W):
            raise RuntimeError(f"world_offset must be [{B}, 2, {H}, {W}], got {tuple(off.shape)}")
        if off.device != hm.device or off.dtype != hm.dtype:
            raise RuntimeError("world_heatmap and world_offset must share device and dtype")
    sfx = _lib.suffix(hm.dtype)
    cap = H * W if max_det is None else int(max_det)
    if cap < 1 or B < 1 or H * W < 1:
        raise RuntimeError("bev_detect needs a non-empty map and max_det >= 1")
    det = torch.empty(B, cap, 3, dtype=hm.dtype, device=hm.device)
    cell = torch.empty(B, cap, dtype=torch.int32, device=hm.device)
    count = torch.empty(B, dtype=torch.int32, device=hm.device)
    lib = _lib.lib()
    args = (hm.data_ptr(), _strides(hm), 0 if off is None else off.data_ptr(), _strides(hm if off is None else off), B, H, W,
            float(world_reduce), float(cls_thres), float(dist_thres), _top_k(top_k), 0 if indexing == "xy" else 1, cap)
    outs = (det.data_ptr(), cell.data_ptr(), count.data_ptr())
    if hm.is_cuda:
        nbytes = lib.mvdetr_detect_workspace_bytes(B, H, W, hm.element_size())
        if nbytes < 0:
            raise RuntimeError(f"bev_detect: unsupported map size {B} x {H} x {W}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=hm.device)
        with torch.cuda.device(hm.device):
            rc = getattr(lib, f"mvdetr_detect_forward_{sfx}")(_lib.current_stream_ptr(hm.device), *args, ws.data_ptr(), *outs)
    else:
        rc = getattr(lib, f"mvdetr_detect_forward_host_{sfx}")(*args, *outs)
    _lib.check(rc, "bev_detect")
    return Detections(det[..., :2], det[..., 2], cell, count)


def distance_nms(points, scores, dist_thres=50 / 2.5, top_k=50):
    """The NMS stage alone, the contract of ``utils.nms`` (utils/nms.py:7-44) with the library's tie rule: points [n,2],
    scores [n] -> ``(keep, count)``: keep int64 [n] whose first ``count`` entries are the kept indices (then zeros), count an
    int32 tensor [1] on the same device (not read back)."""
    points, scores = points.detach(), scores.detach()
    if points.shape[0] != scores.shape[0]:
        raise RuntimeError("make sure same points and scores have the same size")
    if points.device != scores.device or points.dtype != scores.dtype:
        raise RuntimeError("points and scores must share device and dtype")
    n = scores.shape[0]
    keep = torch.zeros(n, dtype=torch.long, device=scores.device)
    count = torch.zeros(1, dtype=torch.int32, device=scores.device)
    if points.numel() == 0:
        return keep, count
    if points.dim() != 2 or points.shape[1] != 2 or scores.dim() != 1:
        raise RuntimeError(f"points must be [n, 2] and scores [n], got {tuple(points.shape)} and {tuple(scores.shape)}")
    sfx = _lib.suffix(scores.dtype)
    points, scores = points.contiguous(), scores.contiguous()
    lib = _lib.lib()
    args = (points.data_ptr(), scores.data_ptr(), n, float(dist_thres), _top_k(top_k))
    if scores.is_cuda:
        nbytes = lib.mvdetr_detect_workspace_bytes(1, 1, n, scores.element_size())
        if nbytes < 0:
            raise RuntimeError(f"distance_nms: unsupported size {n}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=scores.device)
        with torch.cuda.device(scores.device):
            rc = getattr(lib, f"mvdetr_distance_nms_{sfx}")(_lib.current_stream_ptr(scores.device), *args, ws.data_ptr(),
                                                            keep.data_ptr(), count.data_ptr())
    else:
        rc = getattr(lib, f"mvdetr_distance_nms_host_{sfx}")(*args, keep.data_ptr(), count.data_ptr())
    _lib.check(rc, "distance_nms")
    return keep, count
