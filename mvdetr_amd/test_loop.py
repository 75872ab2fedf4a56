"""The reference's test loop (multiview_detector/trainer.py:99-169) with the detections extracted on the device.

Per batch: one ``model.detect`` (forward + fused decode / threshold / NMS), whose result rows are kept on the device behind a
validity mask; nothing is read back until the epoch is over.  Then, as the reference: ``np.savetxt(res_fpath, rows, '%d')``
and the CLEAR-MOD evaluation against the ground-truth file."""
from __future__ import annotations

import os

import numpy as np
import torch

from .evaluation import evaluate
from .ops.detect import bev_detect
from .utils.fused import detection_rows


def test_epoch(model, batches, res_fpath=None, gt_fpath=None, dataset_name="Wildtrack", criterion=None, cls_thres=0.4,
               dist_thres=20, top_k=float("inf"), indexing=None, max_det=None, device=None):
    """``batches``: any iterable of the reference dataloader's tuples ``(imgs, world_gt, imgs_gt, M, frame)``.
    ``criterion(outputs, world_gt, imgs_gt)`` (e.g. train.MVDeTrCriterion) -> loss or ``(loss, terms)``; None: no loss.
    ``indexing`` defaults to the model geometry's (trainer.py:125-128 reads the dataset's).  Returns ``(mean loss or None,
    moda)``; moda is 0 without ``res_fpath``, as in the reference.  Raises if a frame kept more than ``max_det``."""
    model.eval()
    if device is None:
        device = next(model.parameters()).device
    if indexing is None:
        geom = getattr(model, "geom", None)
        indexing = geom.indexing if geom is not None else "xy"
    kw = dict(cls_thres=cls_thres, dist_thres=dist_thres, top_k=top_k, indexing=indexing, max_det=max_det)
    losses, rows, masks, over = [], [], [], []
    for imgs, world_gt, imgs_gt, M, frame in batches:
        imgs = imgs.to(device, non_blocking=True)
        if criterion is None:
            det = model.detect(imgs, M, **kw)
        else:
            # the loss needs the raw outputs: one forward serves both
            with torch.no_grad():
                outputs = model(imgs, M)
                loss = criterion(outputs, world_gt, imgs_gt)
                losses.append((loss[0] if isinstance(loss, tuple) else loss).detach().reshape(()))
            reduce = getattr(getattr(model, "geom", None), "world_reduce", 4)
            det = bev_detect(outputs[0][0], outputs[0][1], world_reduce=reduce, **kw)
        if res_fpath is not None:
            r, m = detection_rows(det, frame)
            rows.append(r)
            masks.append(m)
            over.append((det.count > det.score.shape[1]).any().reshape(1))
    mean_loss = float(torch.stack(losses).mean()) if losses else None
    moda = 0
    if res_fpath is not None:
        if rows:
            if bool(torch.cat(over).any()):
                raise RuntimeError("a frame kept more detections than max_det")
            res = torch.cat(rows)[torch.cat(masks)].cpu().numpy()          # the epoch's one read-back of detections
        else:
            res = np.empty([0, 3])
        np.savetxt(res_fpath, res, "%d")
        if gt_fpath is not None:
            _, _, moda, _ = evaluate(os.path.abspath(res_fpath), os.path.abspath(gt_fpath), dataset_name)
    return mean_loss, moda


test_epoch.__test__ = False        # not a pytest test, whatever a collector thinks of the name
