#!/usr/bin/env python3
"""Golden vectors for mvdetr_amd/augment.py, made by RUNNING the reference's own random_affine (imported from /root/reference
-- build container only; nothing of it is copied).

    python tests/golden/make_golden_affine.py

Writes affine_boxes.npz: ``draws`` seeded draws; for draw i the arguments (``{i}_hw``, ``{i}_boxes``, ``{i}_pids``, ``{i}_seed``,
``{i}_kw`` = hflip, degrees, translate, scale, shear as nine numbers) and what the reference returned (``{i}_out_boxes``,
``{i}_out_pids``, ``{i}_M``).

The reference's module imports cv2 and PIL at module level.  random_affine needs two things of cv2: getRotationMatrix2D, which
the stand-in below supplies by OpenCV's documented formula, and warpPerspective, whose result (the image) is not recorded --
the stand-in returns its input.  The stand-ins are this file's own code."""
import math
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)


def _rotation_matrix_2d(angle, center, scale):
    rad = angle * math.pi / 180.0
    a, b = scale * math.cos(rad), scale * math.sin(rad)
    return np.array([[a, b, (1 - a) * center[0] - b * center[1]], [-b, a, b * center[0] + (1 - a) * center[1]]])


cv2 = types.ModuleType("cv2")
cv2.getRotationMatrix2D = _rotation_matrix_2d
cv2.warpPerspective = lambda img, M, dsize=None, flags=None, borderValue=None: img
cv2.INTER_LINEAR = 1
sys.modules["cv2"] = cv2
if "PIL" not in sys.modules:
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        sys.modules["PIL"] = types.ModuleType("PIL")
        sys.modules["PIL.Image"] = types.ModuleType("PIL.Image")
        sys.modules["PIL"].Image = sys.modules["PIL.Image"]

from multiview_detector.utils.image_utils import random_affine  # noqa: E402


def boxes_for(rng, hw, n):
    """n boxes: most inside, some across an edge (clipped), some slivers and some far outside (rejected)"""
    h, w = hw
    x1, y1 = rng.uniform(-0.2 * w, 1.1 * w, n), rng.uniform(-0.2 * h, 1.1 * h, n)
    bw, bh = rng.uniform(2, 0.25 * w, n), rng.uniform(2, 0.5 * h, n)
    thin = rng.random(n) < 0.15
    bw = np.where(thin, rng.uniform(1, 6, n), bw)
    return np.stack([x1, y1, x1 + bw, y1 + bh], 1)


def main():
    out = {}
    rng = np.random.default_rng(2024)
    draws = 20
    for i in range(draws):
        hw = [(1080, 1920), (720, 1280), (216, 384)][i % 3]
        n = 0 if i == 7 else int(rng.integers(1, 24))
        boxes, pids = boxes_for(rng, hw, n), rng.integers(0, 500, n)
        kw = dict(hflip=0.5, degrees=(-0, 0), translate=(.2, .2), scale=(0.6, 1.4), shear=(-0, 0))      # the reference's defaults
        if i % 4 == 1:
            kw.update(degrees=(-10, 10), shear=(-10, 10))
        if i % 4 == 2:
            kw.update(degrees=(-30, 45), translate=(.1, .3), scale=(0.9, 1.1), hflip=1.0)
        if i % 4 == 3:
            kw.update(shear=(-5, 15), hflip=0.0, scale=(0.5, 2.0))
        seed = 1000 + i
        np.random.seed(seed)
        random.seed(seed)
        img = np.zeros(hw + (3,), dtype=np.uint8)
        _, ob, op, M = random_affine(img, boxes.copy(), pids.copy(), **kw)
        out[f"{i}_hw"], out[f"{i}_boxes"], out[f"{i}_pids"], out[f"{i}_seed"] = np.array(hw), boxes, pids, np.array(seed)
        out[f"{i}_kw"] = np.array([kw["hflip"], *kw["degrees"], *kw["translate"], *kw["scale"], *kw["shear"]], dtype=np.float64)
        out[f"{i}_out_boxes"], out[f"{i}_out_pids"], out[f"{i}_M"] = ob, op, M
        print(i, hw, "boxes", n, "->", len(ob))
    out["draws"] = np.array(draws)
    path = os.path.join(HERE, "affine_boxes.npz")
    np.savez_compressed(path, **out)
    print("affine_boxes.npz:", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
