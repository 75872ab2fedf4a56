"""The training objective and one training step (the reference's trainer.py:44-73 without its loop, logging and
schedules).  On CUDA fp32 / fp64 head outputs the whole objective is two launches of csrc/detection_loss.hip forward (both
heat maps in one focal launch; world offset, image offset and image wh in one L1 launch) and two backward, with no host
synchronise; elsewhere, or with the switch of loss/losses.py off, it is the torch composition of the same formulas.
``train_step_frames`` is the step from decoded frames and device-resident annotations: ingest and targets on the device too."""
from __future__ import annotations

import torch
from torch import nn

from .loss import losses as L

TERMS = ("w_hm", "w_off", "img_hm", "img_off", "img_wh")


def _on(t, ref):
    """The target where the prediction lives: used as it is when already there, else an asynchronous copy."""
    return t if t.device == ref.device else t.to(ref.device, non_blocking=True)


class MVDeTrCriterion(nn.Module):
    """loss = (focal_w + l1_w_off) + (focal_img + l1_img_off + 0.1 l1_img_wh) / N * alpha over the model's output tuple
    ``((world_heatmap, world_offset), (imgs_heatmap, imgs_offset, imgs_wh))`` and the dataloader's target dicts (world_gt[key]:
    [B, ...]; imgs_gt[key]: [B, N, ...]).  ``use_mse=True`` replaces it with MSE(world_heatmap) + alpha MSE(imgs_heatmap) on
    the raw logits, as the reference's trainer does; only the heat maps and their targets are read then.  Returns
    ``(loss, terms)``; terms holds the five detached 0-dim tensors named in TERMS (empty with ``use_mse``, which computes
    none of them)."""

    def __init__(self, alpha=1.0, use_mse=False):
        super().__init__()
        self.alpha, self.use_mse = float(alpha), bool(use_mse)

    def forward(self, outputs, world_gt, imgs_gt):
        (w_hm, w_off), (i_hm, i_off, i_wh) = outputs
        if self.use_mse:
            # only the two heat maps enter: no offset / idx / wh target is needed, and the five terms are not computed
            mse = nn.functional.mse_loss
            w_t, i_t = _on(world_gt["heatmap"], w_hm).to(w_hm.dtype), _on(imgs_gt["heatmap"], i_hm).to(i_hm.dtype)
            return mse(w_hm, w_t) + self.alpha * mse(i_hm, i_t.flatten(0, 1)), {}
        N = imgs_gt["heatmap"].shape[1]
        wg = {k: _on(v, w_hm) for k, v in world_gt.items() if k != "pid"}
        ig = {k: _on(v, i_hm).flatten(0, 1) for k, v in imgs_gt.items() if k != "pid"}
        img_scale = self.alpha / N
        if all(L.fused_loss_available(x) for x in (w_hm, w_off, i_hm, i_off, i_wh)):
            focal = L.focal_loss_segments([w_hm, i_hm], [wg["heatmap"], ig["heatmap"]], weights=(1.0, img_scale))
            l1 = L.reg_l1_loss_segments([w_off, i_off, i_wh], [wg["reg_mask"], ig["reg_mask"], ig["reg_mask"]],
                                        [wg["idx"], ig["idx"], ig["idx"]], [wg["offset"], ig["offset"], ig["wh"]],
                                        weights=(1.0, img_scale, 0.1 * img_scale))
            loss = focal[2] + l1[3]
            f, r = focal.detach(), l1.detach()
            terms = dict(zip(TERMS, (f[0], r[0], f[1], r[1], r[2])))
        else:
            t = (L.focal_loss_composed(w_hm, wg["heatmap"]),
                 L.reg_l1_loss_composed(w_off, wg["reg_mask"], wg["idx"], wg["offset"]),
                 L.focal_loss_composed(i_hm, ig["heatmap"]),
                 L.reg_l1_loss_composed(i_off, ig["reg_mask"], ig["idx"], ig["offset"]),
                 L.reg_l1_loss_composed(i_wh, ig["reg_mask"], ig["idx"], ig["wh"]))
            loss = (t[0] + t[1]) + (t[2] + t[3] + t[4] * 0.1) / N * self.alpha
            terms = {k: v.detach() for k, v in zip(TERMS, t)}
        return loss, terms


def train_step(model, criterion, optimizer, imgs, M, world_gt, imgs_gt):
    """zero_grad, forward, loss, backward, optimizer.step().  Returns the loss tensor (no .item(): nothing here waits for
    the device)."""
    optimizer.zero_grad()
    loss, _ = criterion(model(imgs, M), world_gt, imgs_gt)
    loss.backward()
    optimizer.step()
    return loss.detach()


def train_step_frames(model, criterion, optimizer, frames_u8, M, annotations, angles=None, keep_cams=None):
    """One training step from decoded frames: ``model.ingest(frames_u8, M)`` (uint8 [B, N, Hs, Ws, 3] -> the augmented,
    normalised trunk input), the targets of ``annotations`` (targets.FrameAnnotations, or its first four to six tensors) moved
    by the same ``M`` -- targets.frame_targets on the model's device: two launches, no per-object host work; annotations that
    already live there are used in place -- then ``train_step``.  ``angles`` [B, N] are the rotations that went into ``M``,
    ``keep_cams`` [B, N] the camera dropout of the view targets.  Returns the loss tensor; nothing here waits for the device."""
    from .targets import frame_targets
    imgs = model.ingest(frames_u8, M)
    there = lambda t: None if t is None else _on(t, imgs)  # noqa: E731
    world_gt, imgs_gt = frame_targets(model.geom, *(there(a) for a in annotations), M=M, angles=angles, keep_cams=there(keep_cams))
    return train_step(model, criterion, optimizer, imgs, M, world_gt, imgs_gt)
