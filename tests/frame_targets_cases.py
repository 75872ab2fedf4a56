"""Inputs shared by test_frame_targets.py (host path) and test_frame_targets_gpu.py (kernel): every case is (name, kwargs of
ops.map_targets on CPU tensors), and the yardstick of a case is get_gt (after affine_boxes, with M) map by map.  All maps are at
most a few thousand cells."""
import random

import numpy as np
import torch

from conftest import load_golden
from mvdetr_amd import augment
from mvdetr_amd.targets import get_gt

IMG_HW = (216, 384)                      # with reduce 12: maps of [18, 32]
R_IMG = [18, 32]


def padded(rows, width, cap=None, dtype=torch.float64):
    """Per-map arrays [n_m, width] -> ([maps, cap, width], count [maps] int32); padding rows are filled with a value that would
    land inside the map, so a kernel that read past a count would show."""
    cap = max(max((len(r) for r in rows), default=0), 1) if cap is None else cap
    out = torch.full((len(rows), cap, width), 7.0, dtype=torch.float64)
    for m, r in enumerate(rows):
        if len(r):
            out[m, :len(r)] = torch.as_tensor(np.asarray(r, dtype=np.float64)).reshape(-1, width)
    return out.to(dtype), torch.tensor([len(r) for r in rows], dtype=torch.int32)


def pids_of(count, cap, start=1):
    p = torch.zeros(len(count), cap, dtype=torch.int64)
    for m, n in enumerate(count.tolist()):
        p[m, :n] = torch.arange(start, start + n) * (m + 1)
    return p


def yardstick(kw):
    """get_gt (after affine_boxes where the case has M) map by map, collated; keep == 0 maps are all zero."""
    per_map = []
    for m in range(len(kw["count"])):
        n = int(kw["count"][m])
        p = np.zeros(n, np.int64) if kw.get("pids") is None else kw["pids"][m, :n].numpy()
        common = dict(reduce=kw["reduce"], top_k=kw.get("top_k", 100), kernel_size=kw["kernel_size"])
        if kw.get("points") is not None:
            c = kw["points"][m, :n].double().numpy()
            gt = get_gt(kw["Rshape"], c[:, 0], c[:, 1], v_s=p, **common)
        else:
            b = kw["boxes"][m, :n].double().numpy()
            if kw.get("M") is not None:
                angle = 0.0 if kw.get("angle") is None else float(kw["angle"][m])
                b, p = augment.affine_boxes(b, p, kw["M"][m].numpy(), kw["img_hw"], angle)
            gt = get_gt(kw["Rshape"], (b[:, 0] + b[:, 2]) / 2, b[:, 3], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1], v_s=p, **common)
        if kw.get("keep") is not None and not bool(kw["keep"][m]):
            gt = {k: torch.zeros_like(v) for k, v in gt.items()}
        per_map.append(gt)
    return {k: torch.stack([g[k] for g in per_map]) for k in per_map[0]}


# ---- without M ---------------------------------------------------------------------------------------------------------------

def golden_cases():
    """Every get_gt case of tests/golden/loss.npz (the reference's own outputs): (name, kwargs, golden outputs).  A case with
    sizes becomes boxes (x - w / 2, y - h, x + w / 2, y) around its foot points."""
    G = load_golden("loss.npz")
    out = []
    for i in range(int(G["gt_cases"])):
        kin = {k[len(f"gt_{i}_in_"):]: v for k, v in G.items() if k.startswith(f"gt_{i}_in_")}
        want = {k[len(f"gt_{i}_out_"):]: torch.from_numpy(v)[None] for k, v in G.items() if k.startswith(f"gt_{i}_out_")}
        n = len(kin["v_s"]) if "v_s" in kin else len(kin["x_s"])
        x, y = np.asarray(kin["x_s"], np.float64)[:n], np.asarray(kin["y_s"], np.float64)[:n]
        kw = dict(Rshape=[int(v) for v in kin["Rshape"]], reduce=int(kin.get("reduce", 4)),                # get_gt's defaults
                  kernel_size=int(kin.get("kernel_size", 4)), top_k=int(kin.get("top_k", 100)))
        if "w_s" in kin and "h_s" in kin:
            w, h = np.asarray(kin["w_s"], np.float64)[:n], np.asarray(kin["h_s"], np.float64)[:n]
            kw["boxes"], kw["count"] = padded([np.stack([x - w / 2, y - h, x + w / 2, y], 1)], 4)
        else:
            kw["points"], kw["count"] = padded([np.stack([x, y], 1)], 2)
        if "v_s" in kin:
            cap = (kw.get("boxes") if "boxes" in kw else kw["points"]).shape[1]
            kw["pids"] = torch.zeros(1, cap, dtype=torch.int64)
            kw["pids"][0, :n] = torch.from_numpy(np.asarray(kin["v_s"]).astype(np.int64))
        out.append((f"golden_{i}", kw, want))
    return out


def _uniform_points(rng, n, Rshape, reduce):
    H, W = Rshape
    return np.stack([rng.uniform(-0.1 * W * reduce, 1.1 * W * reduce, n), rng.uniform(-0.1 * H * reduce, 1.1 * H * reduce, n)], 1)


def edge_cases():
    """The seeded edge cases without M: (name, kwargs)."""
    rng = np.random.default_rng(11)
    cases = []

    def add(name, rows, Rshape, reduce, kernel_size, top_k=100, cap=None, with_pids=True, dtype=torch.float64, keep=None):
        pts, count = padded(rows, 2, cap, dtype)
        kw = dict(Rshape=list(Rshape), points=pts, count=count, reduce=reduce, kernel_size=kernel_size, top_k=top_k)
        if with_pids:
            kw["pids"] = pids_of(count, pts.shape[1])
        if keep is not None:
            kw["keep"] = torch.tensor(keep, dtype=torch.bool)
        cases.append((name, kw))

    # a map smaller than the patch (r = 7)
    add("map_smaller_than_patch", [[[0.0, 0.0], [19.9, 11.9], [10.0, 6.0], [20.0, 3.0], [3.0, -0.5]]], [3, 5], 4, 10)
    # centres in the last row / column and in cell 0; x = -0.0 is inside; x exactly W reduce and y exactly H reduce are outside
    add("borders", [[[267.9, 51.9], [0.0, 0.0], [-0.0, 17.0], [268.0, 10.0], [10.0, 52.0], [267.999, 0.1], [133.0, -0.0],
                     [-1e-9, 5.0]]], [13, 67], 4, 10)
    # inside in fp64, but fp32(x / 12) is 160.0: outside
    add("fp32_rounds_to_the_edge", [[[1920 - 1e-7, 10.0], [1919.0, 40.0], [5.0, 48 - 1e-9]]], [4, 160], 12, 10)
    add("count_zero", [[], [[5.0, 5.0]], []], [13, 67], 4, 10, cap=3)
    add("full_100", [_uniform_points(rng, 100, [13, 67], 4)], [13, 67], 4, 10, top_k=100)
    add("top_k_37", [_uniform_points(rng, 37, [13, 67], 4), _uniform_points(rng, 20, [13, 67], 4)], [13, 67], 4, 10, top_k=37)
    add("one_cell_patch", [_uniform_points(rng, 12, [5, 7], 4)], [5, 7], 4, 1)                       # sigma = 1 / 4: r = 0
    add("max_radius", [_uniform_points(rng, 9, [13, 67], 4)], [13, 67], 4, 20)                       # sigma = 5: r = 15
    add("fp32_inputs", [_uniform_points(rng, 30, [13, 67], 4)], [13, 67], 4, 10, dtype=torch.float32)
    add("no_pids", [_uniform_points(rng, 10, [5, 7], 4)], [5, 7], 4, 4, with_pids=False)
    add("dropped_between_kept", [_uniform_points(rng, 15, [13, 67], 4) for _ in range(4)], [13, 67], 4, 10, keep=[1, 0, 1, 0])
    add("real_points_reduce_12", [_uniform_points(rng, 60, R_IMG, 12)], R_IMG, 12, 10)                # a quotient that is not exact
    add("duplicate_cell", [[[21.0, 9.0], [22.5, 10.5], [21.0, 9.0], [300.0, 9.0], [23.9, 8.1]]], [13, 67], 4, 10)
    return cases


# ---- with M, exact: integer boxes, angle 0, scale in {0.5, 0.75, 1.25}, integer shifts ------------------------------------------

def exact_cases():
    """(name, kwargs): every product of these matrices with these boxes is exact in fp64, so get_gt(affine_boxes(...)) is a
    bit-exact yardstick whatever the order of numpy's matmul."""
    rng = np.random.default_rng(5)
    H, W = IMG_HW
    hand = np.array([[100, 80, 180, 160],      # ordinary
                     [0, 60, 60, 150],         # at the left border
                     [330, 40, 384, 120],      # at the right border
                     [150, 0, 210, 70],        # at the top border
                     [150, 150, 230, 216],     # at the bottom border
                     [200, 100, 206, 120],     # small: fails w > 4 at scale 0.5
                     [40, 20, 48, 120],        # a sliver: aspect 12.5
                     [-90, 90, 10, 190],       # mostly outside: little area left
                     [120, 60, 220, 200]], dtype=np.float64)
    cases = []
    for flip in (0, 1):
        for scale, (tx, ty) in ((0.5, (0, 0)), (0.75, (-120, 31)), (1.25, (77, -60)), (1.25, (-150, 90)), (0.75, (170, -95)),
                                (0.5, (400, 0))):                       # the last one pushes every box out: no survivor
            n = 12
            x1, y1 = rng.integers(-20, W - 20, n), rng.integers(-20, H - 20, n)
            boxes = np.concatenate([hand, np.stack([x1, y1, x1 + rng.integers(6, 90, n), y1 + rng.integers(10, 110, n)], 1)], 0)
            M = augment.affine_matrix(IMG_HW, hflip=bool(flip), angle=0.0, scale=scale, tx=tx, ty=ty)
            b, count = padded([boxes], 4)
            cases.append((f"exact_flip{flip}_scale{scale}_shift{tx}_{ty}",
                          dict(Rshape=R_IMG, boxes=b, count=count, pids=pids_of(count, b.shape[1]), M=torch.from_numpy(M)[None],
                               img_hw=IMG_HW, reduce=12, kernel_size=10)))
    # the same as ONE segment of twelve maps, a dropped one among them
    kw = {k: torch.cat([c[1][k] for c in cases]) for k in ("boxes", "count", "pids", "M")}
    kw.update(Rshape=R_IMG, img_hw=IMG_HW, reduce=12, kernel_size=10, keep=torch.tensor([1] * 5 + [0] + [1] * 6, dtype=torch.bool))
    cases.append(("exact_all_in_one_segment", kw))
    return cases


# ---- with M, general: seeded random_affine draws, real-valued boxes ------------------------------------------------------------

def general_case(draws=60, seed=1234):
    """(kwargs, yardstick) of ONE segment of `draws` maps: each map has its own random_affine draw (a third of them rotated by up
    to 10 degrees) over real-valued boxes; the yardstick is get_gt over the boxes random_affine itself returns."""
    rng = np.random.default_rng(seed)
    H, W = IMG_HW
    rows, pid_rows, Ms, angles, yard = [], [], [], [], []
    for d in range(draws):
        n = int(rng.integers(0, 25))
        x1, y1 = rng.uniform(-10, W - 20, n), rng.uniform(-10, H - 30, n)
        boxes = np.stack([x1, y1, x1 + rng.uniform(6, 70, n), y1 + rng.uniform(8, 90, n)], 1)
        pids = np.arange(n, dtype=np.int64) + 100 * d
        degrees = (-10, 10) if d % 3 == 0 else (-0, 0)
        random.seed(seed + d)
        np.random.seed(seed + d)
        state = random.getstate()
        angle = random.random() * (degrees[1] - degrees[0]) + degrees[0]          # random_affine's first draw from `random`
        random.setstate(state)
        moved, kept_pids, M = augment.random_affine(IMG_HW, boxes, pids, degrees=degrees)
        yard.append(get_gt(R_IMG, (moved[:, 0] + moved[:, 2]) / 2, moved[:, 3], moved[:, 2] - moved[:, 0], moved[:, 3] - moved[:, 1],
                           v_s=kept_pids, reduce=12, top_k=100, kernel_size=10))
        rows.append(boxes), pid_rows.append(pids), Ms.append(M), angles.append(angle)
    b, count = padded(rows, 4, cap=24)
    p = torch.zeros(draws, 24, dtype=torch.int64)
    for m, r in enumerate(pid_rows):
        p[m, :len(r)] = torch.from_numpy(r)
    kw = dict(Rshape=R_IMG, boxes=b, count=count, pids=p, M=torch.from_numpy(np.stack(Ms)), angle=torch.tensor(angles, dtype=torch.float64),
              img_hw=IMG_HW, reduce=12, kernel_size=10)
    return kw, {k: torch.stack([g[k] for g in yard]) for k in yard[0]}


def all_cases():
    """Every (name, kwargs) above."""
    return ([(n, kw) for n, kw, _ in golden_cases()] + edge_cases() + exact_cases() + [("general", general_case()[0])])
