"""BEV heat-map -> ground-plane detections, and the peak decoder of the image-plane heads.

Mirrors ``mvdet_decode`` (multiview_detector/utils/decode.py:80-93) and the per-frame post-processing of
the reference's test loop (multiview_detector/trainer.py:133-149): every cell of the world heat-map is a
candidate at (cell + predicted offset) * world_reduce, candidates above ``cls_thres`` go through the
distance NMS, survivors are written as ``frame x y`` rows.  Device-agnostic torch; runs where its inputs live.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .nms import nms


def mvdet_decode(scoremap, offset=None, reduce=4):
    """scoremap [B,1,H,W] (already a probability), offset [B,2,H,W] or None -> [B, H*W, 3] rows
    (x, y, score) in row-major cell order, x = (column + dx) * reduce, y = (row + dy) * reduce; without an
    offset map the cell centre (+0.5) is used (decode.py:80-93)."""
    B, C, H, W = scoremap.shape
    ys, xs = torch.meshgrid(torch.arange(H, device=scoremap.device), torch.arange(W, device=scoremap.device),
                            indexing="ij")
    xy = torch.stack([xs, ys], -1).reshape(1, H * W, 2).float().expand(B, -1, -1)
    if offset is not None:
        xy = xy + offset.permute(0, 2, 3, 1).reshape(B, H * W, 2)
    else:
        xy = xy + 0.5
    xy = xy * reduce
    scores = scoremap.permute(0, 2, 3, 1).reshape(B, H * W, C)[..., :1]
    return torch.cat([xy, scores], dim=2)


def _peaks(scoremap):
    """Zero every cell that is not the maximum of its 3x3 neighbourhood (decode.py:7-11; max_pool2d pads with -inf)."""
    hmax = F.max_pool2d(scoremap, (3, 3), stride=1, padding=1)
    return scoremap * (hmax == scoremap).float()


def _gather_map(feat, inds):
    """feat [B,C,H,W], inds [B,K] row-major cells -> [B,K,C] (tensor_utils.py's _transpose_and_gather_feat)."""
    B, C = feat.shape[:2]
    feat = feat.permute(0, 2, 3, 1).reshape(B, -1, C)
    return feat.gather(1, inds.unsqueeze(2).expand(B, inds.shape[1], C))


def ctdet_decode(heatmap, offset=None, wh=None, id=None, top_K=100):
    """The reference's peak decoder (decode.py:47-77), used on the image heads (trainer.py:173) and as the world maps' peak-based
    alternative (mvdetr.py:237): heatmap [B,C,H,W] raw logits, offset and wh [B,2,H,W] or None -> [B, top_K, 3] rows
    (x, y, score), or [B, top_K, 5] rows (x, y, w, h, score) with ``wh``, in descending score order.  Positions are in map
    cells: x = column + dx (one add), + 0.5 without an offset map.  A score survives where it equals the maximum of its 3x3
    neighbourhood and is zeroed elsewhere, so with fewer than top_K peaks the remaining rows are zero-score cells in
    ``torch.topk``'s order.  Several channels go through the reference's two-stage top-K (per class, then over the classes'
    winners); the class column is dropped, as the reference drops it.  ``id`` is not implemented: the reference's branch views a
    [B, K, 1] argmax as [B, K, 2] and cannot run."""
    if id is not None:
        raise NotImplementedError("ctdet_decode: the id branch of the reference cannot run (decode.py:72-76); pass id=None")
    B, C, H, W = heatmap.shape
    scoremap = _peaks(torch.sigmoid(heatmap))
    class_scores, class_inds = torch.topk(scoremap.view(B, C, -1), top_K)
    class_inds = class_inds % (H * W)
    scores, pick = torch.topk(class_scores.view(B, -1), top_K)
    inds = class_inds.view(B, -1).gather(1, pick)
    ys, xs = (inds / W).int().float(), (inds % W).int().float()
    xy = torch.stack([xs, ys], dim=2)
    xy = xy + (0.5 if offset is None else _gather_map(offset, inds))
    parts = [xy] + ([] if wh is None else [_gather_map(wh, inds)]) + [scores.view(B, top_K, 1)]
    return torch.cat(parts, dim=2)


def detections_from_heatmap(world_heatmap, world_offset, frames, world_reduce=4, cls_thres=0.4, indexing="xy",
                            dist_thres=20, top_k=float("inf")):
    """The reference test loop's result rows for one batch (trainer.py:133-149): raw heat-map logits
    [B,1,H,W] + offsets [B,2,H,W] -> float tensor [n, 3] of (frame, x, y) rows, frames in batch order,
    detections of a frame in descending score order.  ``indexing='ij'`` swaps the coordinates like
    trainer.py:139-142."""
    xys = mvdet_decode(torch.sigmoid(world_heatmap.detach()), None if world_offset is None else world_offset.detach(),
                       reduce=world_reduce)
    positions, scores = xys[:, :, :2], xys[:, :, 2]
    if indexing != "xy":
        positions = positions[:, :, [1, 0]]
    rows = []
    for b in range(xys.shape[0]):
        sel = scores[b] > cls_thres
        pos, s = positions[b, sel], scores[b, sel]
        keep, count = nms(pos, s, dist_thres, top_k)
        kept = pos[keep[:count]]
        rows.append(torch.cat([torch.full((count, 1), float(frames[b]), device=kept.device), kept], dim=1))
    return torch.cat(rows, dim=0) if rows else torch.empty(0, 3)
