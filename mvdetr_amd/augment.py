"""The host half of the reference's ``random_affine`` augmentation (multiview_detector/utils/image_utils.py:9-83), in plain numpy.

The reference warps the decoded image with ``cv2.warpPerspective`` on the CPU and moves the boxes with the same matrix; here the
image half is ``ops.ingest_frames(frames, M)`` on the GPU, and this module makes ``M`` and moves the boxes:

    boxes, pids, M = random_affine((1080, 1920), boxes, pids)
    imgs = model.ingest(frames, M_of_every_camera)          # the same M goes to model.forward / detect

``M`` maps source pixels to destination pixels (``cv2.warpPerspective``'s convention), float64 [3, 3]."""
from __future__ import annotations

import math
import random

import numpy as np


def rotation_matrix_2d(center, angle, scale):
    """``cv2.getRotationMatrix2D`` by its documented formula: [[a, b, (1 - a) cx - b cy], [-b, a, b cx + (1 - a) cy]] with
    a = scale cos(angle), b = scale sin(angle), angle in degrees (positive = counter-clockwise, origin top-left)."""
    rad = angle * math.pi / 180.0
    a, b = scale * math.cos(rad), scale * math.sin(rad)
    cx, cy = center
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], dtype=np.float64)


def affine_matrix(img_hw, hflip=False, angle=0.0, scale=1.0, tx=0.0, ty=0.0, shear_x=0.0, shear_y=0.0):
    """M = S @ T @ R @ F (image_utils.py:18-42): horizontal flip (x -> width - x, the reference's own matrix, which sends source
    column 0 outside), rotation by ``angle`` degrees and ``scale`` about the image centre, translation by (tx, ty) pixels, shear by
    (shear_x, shear_y) degrees."""
    height, width = img_hw
    F = np.eye(3)
    if hflip:
        F[0, 0] = -1
        F[0, 2] = width
    R = np.eye(3)
    R[:2] = rotation_matrix_2d((width / 2, height / 2), angle, scale)
    T = np.eye(3)
    T[0, 2] = tx
    T[1, 2] = ty
    S = np.eye(3)
    S[0, 1] = math.tan(shear_x * math.pi / 180)
    S[1, 0] = math.tan(shear_y * math.pi / 180)
    return S @ T @ R @ F


def affine_boxes(bboxs, pids, M, img_hw, angle=0.0):
    """Boxes [n, 4] (x1, y1, x2, y2) moved by M, as the reference's augmentation moves them (image_utils.py:46-83):

      1. the four corners of a box go through M (its first two rows: the matrices made here are affine) and the box becomes their
         axis-aligned hull;
      2. the hull is shrunk about its centre by sqrt(max(|sin angle|, |cos angle|)) -- the hull of a rotated box overstates it;
      3. its edges are clipped to [0, width - 1] x [0, height - 1];
      4. a box is kept when, after clipping, both sides exceed 4 px, more than a tenth of its original area is left and its aspect
         ratio stays below 10.

    Returns (boxes, pids) of the kept ones."""
    height, width = img_hw
    bboxs = np.asarray(bboxs, dtype=np.float64).reshape(-1, 4)
    pids = np.asarray(pids)
    lo, hi = bboxs[:, :2], bboxs[:, 2:]                                           # [n, 2] (x, y) of the two given corners
    area_before = np.prod(hi - lo, axis=1)

    # 1. corners [n, 4, 2] -> homogeneous [n, 4, 3] -> through M
    corners = np.stack([lo, hi, np.stack([lo[:, 0], hi[:, 1]], 1), np.stack([hi[:, 0], lo[:, 1]], 1)], axis=1)
    moved = np.concatenate([corners, np.ones(corners.shape[:2] + (1,))], axis=2) @ np.asarray(M, dtype=np.float64).T
    hull_lo, hull_hi = moved[..., :2].min(axis=1), moved[..., :2].max(axis=1)

    # 2. shrink about the centre
    rad = angle * math.pi / 180
    shrink = math.sqrt(max(abs(math.sin(rad)), abs(math.cos(rad))))
    centre, size = (hull_hi + hull_lo) / 2, (hull_hi - hull_lo) * shrink
    limit = np.array([width - 1, height - 1], dtype=np.float64)

    # 3. clip
    new_lo, new_hi = np.clip(centre - size / 2, 0, limit), np.clip(centre + size / 2, 0, limit)

    # 4. keep
    side = new_hi - new_lo
    w, h = side[:, 0], side[:, 1]
    tiny = 1e-16                                                                   # the reference's guard against 0 / 0
    big_enough = (w > 4) & (h > 4)
    mostly_there = w * h / (area_before + tiny) > 0.1
    not_a_sliver = np.maximum(w / (h + tiny), h / (w + tiny)) < 10
    keep = big_enough & mostly_there & not_a_sliver
    return np.concatenate([new_lo, new_hi], axis=1)[keep], pids[keep]


def random_affine(img_hw, bboxs, pids, hflip=0.5, degrees=(-0, 0), translate=(.2, .2), scale=(0.6, 1.4), shear=(-0, 0)):
    """One draw of the reference's augmentation for an image of size ``img_hw`` = (height, width): the random numbers come from
    ``np.random`` (the flip) and ``random`` (everything else) in the reference's order, so a run seeded like the reference's draws
    the same matrices.  Returns (boxes, pids, M); warp the image itself with ``ops.ingest_frames(frames, M)``."""
    height, width = img_hw
    flip = np.random.rand() < hflip
    angle = random.random() * (degrees[1] - degrees[0]) + degrees[0]
    s = random.random() * (scale[1] - scale[0]) + scale[0]
    tx = (random.random() * 2 - 1) * translate[0] * width
    ty = (random.random() * 2 - 1) * translate[1] * height
    shear_x = random.random() * (shear[1] - shear[0]) + shear[0]
    shear_y = random.random() * (shear[1] - shear[0]) + shear[0]
    M = affine_matrix(img_hw, flip, angle, s, tx, ty, shear_x, shear_y)
    bboxs, pids = affine_boxes(bboxs, pids, M, img_hw, angle)
    return bboxs, pids, M
