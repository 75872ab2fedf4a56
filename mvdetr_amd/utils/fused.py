"""The same post-processing as ``decode.py`` / ``nms.py`` on the library's fused kernel (ops/detect.py): the maps stay where
the model left them, one call extracts every frame's detections, and the only read-back is the frames' counts at the end.

Same signatures, same rows -- except among candidates of exactly equal score, where ``nms`` follows whatever permutation an
unstable ``torch.sort`` produced and the fused path visits the higher index first (ops/detect.py)."""
from __future__ import annotations

import torch

from ..ops.detect import bev_detect, distance_nms
from ..ops.peak_detect import peak_detect


def detection_rows(det, frames):
    """``bev_detect``'s result + the frames' numbers -> ([B * max_det, 3] (frame, x, y) rows, [B * max_det] validity mask), on
    the device and without a read-back; ``rows[mask]`` are the reference's result rows."""
    B, cap = det.score.shape
    frames = torch.as_tensor(frames, dtype=det.xy.dtype).reshape(B).to(det.xy.device, non_blocking=True)
    rows = torch.cat([frames.view(B, 1, 1).expand(B, cap, 1), det.xy], dim=2).reshape(B * cap, 3)
    mask = torch.arange(cap, device=det.count.device).view(1, cap) < det.count.view(B, 1)
    return rows, mask.reshape(B * cap)


def detections_from_heatmap_fused(world_heatmap, world_offset, frames, world_reduce=4, cls_thres=0.4, indexing="xy",
                                  dist_thres=20, top_k=float("inf"), max_det=None):
    """``detections_from_heatmap`` on the fused kernel: [n, 3] (frame, x, y) rows, frames in batch order, a frame's detections
    in descending score order.  One read-back (the counts).  Raises if a frame kept more than ``max_det``."""
    det = bev_detect(world_heatmap, world_offset, world_reduce=world_reduce, cls_thres=cls_thres, dist_thres=dist_thres,
                     top_k=top_k, indexing=indexing, max_det=max_det)
    rows, mask = detection_rows(det, frames)
    counts = det.count.cpu()
    cap = det.score.shape[1]
    if int(counts.max()) > cap:
        raise RuntimeError(f"a frame kept {int(counts.max())} detections, more than max_det = {cap}")
    return rows[mask]


def nms_fused(points, scores, dist_thres=50 / 2.5, top_k=50):
    """``nms``'s signature and return types (keep LongTensor, count int) on the library's kernel."""
    keep, count = distance_nms(points, scores, dist_thres, top_k)
    return keep, int(count)


def ctdet_decode_fused(heatmap, offset=None, wh=None, top_K=100):
    """``ctdet_decode``'s tensor ([B, top_K, 3] or [B, top_K, 5]) from the fused kernel (ops/peak_detect.py), single-channel
    heat maps only, no read-back.  Differs from ``ctdet_decode`` in two places: rows past the map's candidate count are zero
    (the reference fills them with zero-score cells in ``torch.topk``'s order), and equal scores come higher cell first."""
    det = peak_detect(heatmap, offset, wh, top_k=top_K)
    parts = [det.xy] + ([] if wh is None else [det.wh]) + [det.score.unsqueeze(2)]
    return torch.cat(parts, dim=2)
