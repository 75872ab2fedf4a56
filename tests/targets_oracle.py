"""The arithmetic of ops.map_targets (include/mvdetr_ops.h) as plain Python float loops: a Python float is an
fp64, a Python expression is never contracted into an FMA, and there is no numpy matmul here.  fp32 roundings are numpy float32
scalars.  Two switches break it on purpose for the teeth tests: ``ct_fp32_division`` divides the centre in fp32 instead of
rounding the fp64 quotient once, ``compact=False`` leaves a kept box in the slot of its object index."""
import math

import numpy as np
import torch

from mvdetr_amd.targets import gaussian_patch

F = np.float32


def shrink_of(angle):
    rad = angle * math.pi / 180
    return math.sqrt(max(abs(math.sin(rad)), abs(math.cos(rad))))


def move_box(box, M, shrink, img_hw):
    """(moved box, kept) of one box (x1, y1, x2, y2) through the 3x3 nested list M."""
    x1, y1, x2, y2 = box
    corners = ((x1, y1), (x2, y2), (x1, y2), (x2, y1))
    X = [(M[0][0] * x + M[0][1] * y) + M[0][2] for x, y in corners]
    Y = [(M[1][0] * x + M[1][1] * y) + M[1][2] for x, y in corners]
    moved = []
    for lo, hi, lim in ((min(X), max(X), float(img_hw[1] - 1)), (min(Y), max(Y), float(img_hw[0] - 1))):
        c = (hi + lo) / 2
        s = (hi - lo) * shrink
        moved.append((min(max(c - s / 2, 0.0), lim), min(max(c + s / 2, 0.0), lim)))
    (nx1, nx2), (ny1, ny2) = moved
    w, h = nx2 - nx1, ny2 - ny1
    area = (x2 - x1) * (y2 - y1)
    kept = (w > 4 and h > 4) and (w * h / (area + 1e-16) > 0.1) and (max(w / (h + 1e-16), h / (w + 1e-16)) < 10)
    return (nx1, ny1, nx2, ny2), kept


def map_targets(Rshape, *, points=None, boxes=None, count, pids=None, M=None, angle=None, img_hw=None, keep=None, reduce,
                kernel_size, top_k=100, ct_fp32_division=False, compact=True):
    """ops.map_targets' signature and result, on CPU tensors."""
    H, W = Rshape
    coords = (boxes if boxes is not None else points).double().tolist()
    maps = len(coords)
    sigma = kernel_size / reduce
    r = int(3 * sigma)
    patch = gaussian_patch(r, sigma).astype(F)
    gt = {"heatmap": torch.zeros(maps, 1, H, W), "reg_mask": torch.zeros(maps, top_k, dtype=torch.bool),
          "idx": torch.zeros(maps, top_k, dtype=torch.int64), "pid": torch.zeros(maps, top_k, dtype=torch.int64),
          "offset": torch.zeros(maps, top_k, 2)}
    if boxes is not None:
        gt["wh"] = torch.zeros(maps, top_k, 2)
    for m in range(maps):
        if keep is not None and not bool(keep[m]):
            continue
        hm = gt["heatmap"][m, 0].numpy()
        mat = None if M is None else M[m].double().tolist()
        shrink = 1.0 if angle is None else shrink_of(float(angle[m]))
        used = 0
        for i in range(int(count[m])):
            w = h = 0.0
            if boxes is not None:
                box = coords[m][i]
                if mat is not None:
                    box, kept = move_box(box, mat, shrink, img_hw)
                    if not kept:
                        continue
                x, y, w, h = (box[0] + box[2]) / 2, box[3], box[2] - box[0], box[3] - box[1]
            else:
                x, y = coords[m][i]
            slot = used if compact else i
            used += 1
            if ct_fp32_division:
                fx, fy = F(x) / F(reduce), F(y) / F(reduce)
            else:
                fx, fy = F(x / reduce), F(y / reduce)
            if not (fx >= 0 and fy >= 0 and fx < F(W) and fy < F(H)):
                continue
            cx, cy = int(fx), int(fy)
            gt["reg_mask"][m, slot] = True
            gt["idx"][m, slot] = cy * W + cx
            gt["pid"][m, slot] = 0 if pids is None else int(pids[m, i])
            gt["offset"][m, slot, 0], gt["offset"][m, slot, 1] = float(fx - F(cx)), float(fy - F(cy))
            if boxes is not None:
                gt["wh"][m, slot, 0], gt["wh"][m, slot, 1] = float(F(w / reduce)), float(F(h / reduce))
            for py in range(max(cy - r, 0), min(cy + r, H - 1) + 1):
                for px in range(max(cx - r, 0), min(cx + r, W - 1) + 1):
                    hm[py, px] = max(hm[py, px], patch[py - cy + r, px - cx + r])
    return gt
