"""Training targets: the CenterNet-style ground truth MVDeTr's dataset builds for every map (reference:
datasets/frameDataset.py:19-46 with the gaussian of utils/image_utils.py:86-111).  ``get_gt`` is the host (numpy) definition, one
map at a time; ``frame_targets`` builds the same dicts for whole frames from padded annotation tensors where those live -- on the
device in two launches of ops.map_targets, with no per-object host work.  Seeded synthetic frames of both serve tests and tools
(this package has no dataset classes)."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch


def gaussian_patch(radius, sigma):
    """The [2 radius + 1, 2 radius + 1] fp64 patch exp(-d^2 / (2 sigma^2)) of squared distances d^2 to its middle cell;
    entries under eps * peak are cut to 0."""
    sq = np.square(np.arange(-radius, radius + 1, dtype=np.float64))
    patch = np.exp(-(sq[None, :] + sq[:, None]) / (2.0 * sigma * sigma))
    patch[patch < np.finfo(np.float64).eps * patch.max()] = 0.0
    return patch


def splat_max(heatmap, cx, cy, patch):
    """heatmap[H, W] = max(heatmap, patch centred on cell (cx, cy)) over the part of the patch that lies inside the map."""
    r = patch.shape[0] // 2
    H, W = heatmap.shape
    x0, x1 = max(cx - r, 0), min(cx + r + 1, W)                  # the patch's column / row range intersected with the map's
    y0, y1 = max(cy - r, 0), min(cy + r + 1, H)
    if x0 < x1 and y0 < y1:
        window = heatmap[y0:y1, x0:x1]
        window[...] = np.maximum(window, patch[y0 - cy + r:y1 - cy + r, x0 - cx + r:x1 - cx + r])


def get_gt(Rshape, x_s, y_s, w_s=None, h_s=None, v_s=None, reduce=4, top_k=100, kernel_size=4):
    """Targets of one [H, W] = Rshape map from object positions (x_s, y_s) given at `reduce` times its resolution.

    Slot k belongs to object k (objects outside the map leave their slot empty): reg_mask [top_k] bool, idx [top_k] int64
    = y * W + x of the truncated centre, offset [top_k, 2] = centre - truncated centre (fp32 arithmetic), pid [top_k] int64
    = v_s (zeros without it), wh [top_k, 2] = (w_s, h_s) / reduce only when both are given, heatmap [1, H, W] fp32 with
    a gaussian of sigma = kernel_size / reduce per object.  An object inside the map beyond slot top_k - 1 raises ValueError."""
    H, W = Rshape
    n = len(x_s) if v_s is None else len(v_s)
    centre = np.stack([np.asarray(x_s)[:n] / reduce, np.asarray(y_s)[:n] / reduce], axis=1).astype(np.float32)   # [n, 2] (x, y)
    inside = (centre >= 0).all(axis=1) & (centre[:, 0] < W) & (centre[:, 1] < H)                   # tested on the fp32 centre
    slots = np.flatnonzero(inside)
    if slots.size and slots[-1] >= top_k:
        raise ValueError(f"object {slots[-1]} lies inside the map but there are only top_k = {top_k} slots")
    cell = centre[slots].astype(np.int32)

    sigma = kernel_size / reduce
    patch = gaussian_patch(int(3 * sigma), sigma)                # one patch serves every object of the map
    heatmap = np.zeros((1, H, W), np.float32)
    for cx, cy in cell.tolist():
        splat_max(heatmap[0], cx, cy, patch)

    def slotted(values, dtype, width=()):
        full = np.zeros((top_k, *width), dtype)
        full[slots] = values
        return torch.from_numpy(full)

    gt = {"heatmap": torch.from_numpy(heatmap),
          "reg_mask": slotted(True, bool),
          "idx": slotted(cell[:, 1].astype(np.int64) * W + cell[:, 0], np.int64),
          "pid": slotted(0 if v_s is None else np.asarray(v_s)[slots], np.int64),
          "offset": slotted(centre[slots] - cell.astype(np.float32), np.float32, (2,))}
    if w_s is not None and h_s is not None:
        sizes = np.stack([np.asarray(w_s)[:n], np.asarray(h_s)[:n]], axis=1) / reduce
        gt["wh"] = slotted(sizes[slots], np.float32, (2,))
    return gt


def synthetic_frame_targets(geom, n_people, seed=0, batch=1, top_k=100, world_kernel_size=10, img_kernel_size=10):
    """(world_gt, imgs_gt) of `batch` frames as a dataloader would collate them -- world_gt[key]: [B, ...], imgs_gt[key]:
    [B, N, ...] -- from seeded random ground points and random per-view boxes.  The world and image targets are NOT
    geometrically consistent (no projection is involved): they exercise the objective, nothing more."""
    rng = np.random.default_rng(seed)
    gh, gw = geom.worldgrid_shape
    ih, iw = geom.img_shape
    world, views = [], []
    for _ in range(batch):
        ids = np.arange(n_people)
        world.append(get_gt(geom.Rworld_shape, rng.uniform(0, gw, n_people), rng.uniform(0, gh, n_people), v_s=ids,
                            reduce=geom.world_reduce, top_k=top_k, kernel_size=world_kernel_size))
        per_view = []
        for _ in range(geom.num_cam):
            w, h = rng.uniform(20, iw / 6, n_people), rng.uniform(40, ih / 3, n_people)
            # foot points, some of them a little outside the image as a real view has them
            x, y = rng.uniform(-0.05 * iw, 1.05 * iw, n_people), rng.uniform(-0.05 * ih, 1.05 * ih, n_people)
            per_view.append(get_gt(geom.Rimg_shape, x, y, w, h, v_s=ids, reduce=geom.img_reduce, top_k=top_k,
                                   kernel_size=img_kernel_size))
        views.append({k: torch.stack([v[k] for v in per_view]) for k in per_view[0]})
    world_gt = {k: torch.stack([w[k] for w in world]) for k in world[0]}
    imgs_gt = {k: torch.stack([v[k] for v in views]) for k in views[0]}
    return world_gt, imgs_gt


class FrameAnnotations(NamedTuple):
    """The padded annotations of ``B`` frames that ``frame_targets`` takes, in its argument order (``*annotations``).  Rows past
    a count are padding and never read; the tensors may live on the device for a whole run."""
    world_pts: torch.Tensor          # [B, cap, 2] float64 (x, y) on the ground grid
    world_count: torch.Tensor        # [B] int32
    boxes: torch.Tensor              # [B, N, cap, 4] float64 (x1, y1, x2, y2) in image pixels
    box_count: torch.Tensor          # [B, N] int32
    world_pids: torch.Tensor         # [B, cap] int64
    box_pids: torch.Tensor           # [B, N, cap] int64


def frame_targets(geom, world_pts, world_count, boxes, box_count, world_pids=None, box_pids=None, *, M=None, angles=None,
                  keep_cams=None, top_k=100, world_kernel_size=10, img_kernel_size=10):
    """(world_gt, imgs_gt) of ``B`` frames as a dataloader collates them -- world_gt[key]: [B, ...], imgs_gt[key]: [B, N, ...],
    'wh' only there: the layout MVDeTrCriterion takes -- from padded annotations (FrameAnnotations), built where they live by
    two ops.map_targets calls: one launch for the B world maps, one for the B N view maps.

    ``M`` [B, N, 3, 3] (the matrices augment.random_affine returns; CPU or device) moves the boxes as augment.affine_boxes
    does, with the rotation ``angles`` [B, N] in degrees; ``keep_cams`` [B, N] bool zeroes the view targets of dropped cameras
    and nothing else (the reference's camera dropout, frameDataset.py:226-231).  The world points are not augmented."""
    from .ops import map_targets
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 4:
        raise RuntimeError(f"frame_targets: boxes must be [B, N, cap, 4], got {tuple(getattr(boxes, 'shape', ()))}")
    B, N = boxes.shape[:2]
    per_map = lambda t: None if t is None else t.flatten(0, 1)  # noqa: E731
    world_gt = map_targets(geom.Rworld_shape, points=world_pts, count=world_count, pids=world_pids, reduce=geom.world_reduce,
                           kernel_size=world_kernel_size, top_k=top_k)
    views = map_targets(geom.Rimg_shape, boxes=per_map(boxes), count=per_map(box_count), pids=per_map(box_pids), M=per_map(M),
                        angle=per_map(angles), img_hw=geom.img_shape, keep=per_map(keep_cams), reduce=geom.img_reduce,
                        kernel_size=img_kernel_size, top_k=top_k)
    return world_gt, {k: v.unflatten(0, (B, N)) for k, v in views.items()}


def synthetic_frame_annotations(geom, n_people, seed=0, batch=1, cap=None):
    """The FrameAnnotations (CPU) of the frames synthetic_frame_targets draws: the same rng, the same draws in the same order,
    so ``frame_targets(geom, *synthetic_frame_annotations(...))`` is ``synthetic_frame_targets(...)``.  A view's box is
    (x - w / 2, y - h, x + w / 2, y) around its drawn foot point (x, y): the point and size formed back from it agree with the
    draws to an fp64 ulp, which the targets' fp32 roundings absorb.  ``cap`` (default n_people) pads the object axis."""
    cap = max(n_people, 1) if cap is None else int(cap)
    if cap < n_people:
        raise ValueError(f"cap = {cap} cannot hold {n_people} people")
    rng = np.random.default_rng(seed)
    gh, gw = geom.worldgrid_shape
    ih, iw = geom.img_shape
    N = geom.num_cam
    pts, boxes = np.zeros((batch, cap, 2)), np.zeros((batch, N, cap, 4))
    for b in range(batch):
        pts[b, :n_people, 0], pts[b, :n_people, 1] = rng.uniform(0, gw, n_people), rng.uniform(0, gh, n_people)
        for c in range(N):
            w, h = rng.uniform(20, iw / 6, n_people), rng.uniform(40, ih / 3, n_people)
            x, y = rng.uniform(-0.05 * iw, 1.05 * iw, n_people), rng.uniform(-0.05 * ih, 1.05 * ih, n_people)
            boxes[b, c, :n_people] = np.stack([x - w / 2, y - h, x + w / 2, y], axis=1)
    ids = torch.zeros(cap, dtype=torch.int64)
    ids[:n_people] = torch.arange(n_people)
    return FrameAnnotations(torch.from_numpy(pts), torch.full((batch,), n_people, dtype=torch.int32), torch.from_numpy(boxes),
                            torch.full((batch, N), n_people, dtype=torch.int32), ids.expand(batch, cap).contiguous(),
                            ids.expand(batch, N, cap).contiguous())
