#!/usr/bin/env python3
"""Golden vectors for the training objective, made by RUNNING the reference's own get_gt, FocalLoss, RegL1Loss, RegCELoss
and GaussianMSE (imported from /root/reference -- build container only; nothing of it is copied).

    python tests/golden/make_golden_loss.py

Writes loss.npz:
  gt_cases, gt_{i}_in_*  / gt_{i}_out_*     get_gt arguments -> every key it returns (datasets/frameDataset.py:19-46)
  focal_cases, focal_{i}_{x,t,m}            logits (fp64), target, optional mask -> loss32, grad32, loss64, grad64
                                            (an input that repeats an earlier one is stored once: {key}_same_as names it)
  l1_cases, l1_{i}_{x,mask,ind,t}           -> loss32, grad32, loss64, grad64           (loss/losses.py:54-64)
  ce_{x,mask,ind,t}, ce_loss*, ce_grad*     RegCELoss; ce_empty = its value for an all-false mask
  gmse_{x,t,k}, gmse_loss, gmse_grad        GaussianMSE
  frame_*                                   head outputs of one mini-sized frame, its get_gt targets ([B, ...] / [B, N, ...]),
                                            the five terms and the total of trainer.py:52-63 in fp32 and fp64, the use_mse total

The reference's dataset module imports cv2, kornia, torchvision and matplotlib at module level, none of which the losses or
get_gt use; empty stand-in modules satisfy those imports (this file's own code)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

if not hasattr(np, "bool"):
    np.bool = bool                                            # the reference predates numpy 1.24
for name in ("cv2", "kornia", "torchvision", "torchvision.datasets", "torchvision.transforms", "matplotlib", "matplotlib.pyplot"):
    if name not in sys.modules:
        sys.modules[name] = types.ModuleType(name)
sys.modules["torchvision.datasets"].VisionDataset = object
sys.modules["torchvision"].datasets = sys.modules["torchvision.datasets"]
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]

from multiview_detector.datasets.frameDataset import get_gt  # noqa: E402
from multiview_detector.loss import FocalLoss, GaussianMSE, RegCELoss, RegL1Loss  # noqa: E402


def run(fn, x, dtype):
    x = x.detach().clone().to(dtype).requires_grad_(True)
    loss = fn(x)
    loss.backward()
    return loss.detach().numpy(), x.grad.numpy()


def both(out, prefix, fn, x):
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        out[f"{prefix}_loss{tag}"], out[f"{prefix}_grad{tag}"] = run(fn, x, dtype)


def put(out, key, tensor, seen):
    """out[key] = the array, or, for an input an earlier key already holds, out[key + "_same_as"] = that key."""
    if id(tensor) in seen:
        out[key + "_same_as"] = np.array(seen[id(tensor)])
    else:
        seen[id(tensor)] = key
        out[key] = tensor.numpy()


def gt_cases():
    world = dict(Rshape=[120, 360], reduce=4, kernel_size=10)
    img = dict(Rshape=[90, 160], reduce=12, kernel_size=10)
    rng = np.random.default_rng(11)
    cases = []
    # centres on every border and just outside it, world settings, no sizes
    xs = np.array([0.0, 1439.9, 1440.0, -0.1, 700.0, 700.0, 700.0, 3.9, 1436.0])
    ys = np.array([0.0, 479.9, 100.0, 100.0, 480.0, -4.0, 479.0, 0.0, 476.1])
    cases.append(dict(world, x_s=xs, y_s=ys, v_s=np.arange(len(xs)) + 5))
    # two objects in one cell, a third in the neighbouring one
    cases.append(dict(world, x_s=np.array([401.0, 402.5, 404.0]), y_s=np.array([200.0, 203.0, 200.0]), v_s=np.array([3, 1, 2])))
    # image settings with sizes: borders, outside, a duplicate cell
    xs = np.array([0.0, 1919.0, 1920.0, 960.0, 965.0, -1.0, 500.5, 11.9])
    ys = np.array([0.0, 1079.0, 500.0, 540.0, 545.0, 500.0, 1080.0, 1079.9])
    cases.append(dict(img, x_s=xs, y_s=ys, w_s=rng.uniform(20, 300, len(xs)), h_s=rng.uniform(40, 400, len(xs)),
                      v_s=np.arange(len(xs))))
    # random crowds at both settings, with and without sizes; integer inputs as the dataset's world grid has them
    xs, ys = rng.integers(-20, 1460, 40), rng.integers(-20, 500, 40)
    cases.append(dict(world, x_s=xs, y_s=ys, v_s=rng.integers(0, 1000, 40)))
    xs, ys = rng.uniform(-50, 1970, 30), rng.uniform(-50, 1130, 30)
    cases.append(dict(img, x_s=xs, y_s=ys, w_s=rng.uniform(20, 300, 30), h_s=rng.uniform(40, 400, 30), v_s=rng.integers(0, 1000, 30)))
    cases.append(dict(img, x_s=xs, y_s=ys, v_s=rng.integers(0, 1000, 30)))
    # the defaults (reduce 4, kernel 4) on a small map, top_k 6 with exactly 6 objects, one of them outside
    cases.append(dict(Rshape=[10, 14], x_s=np.array([3.0, 55.9, 20.0, 60.0, 0.0, 30.0]), y_s=np.array([3.0, 39.9, 20.0, 20.0, 39.0, 0.0]),
                      v_s=np.arange(6), top_k=6))
    return cases


def main():
    out, seen = {}, {}
    g = torch.Generator().manual_seed(77)

    cases = gt_cases()
    for i, kw in enumerate(cases):
        for k, v in kw.items():
            out[f"gt_{i}_in_{k}"] = np.asarray(v)
        for k, v in get_gt(**kw).items():
            out[f"gt_{i}_out_{k}"] = v.numpy()
    out["gt_cases"] = np.array(len(cases))

    # ---- focal ----
    focal = FocalLoss()
    H, W = 24, 72
    rng = np.random.default_rng(5)
    tgt = get_gt([H, W], rng.uniform(0, W * 4, 9), rng.uniform(0, H * 4, 9), v_s=np.arange(9), reduce=4, kernel_size=10)["heatmap"]
    tgt2 = torch.stack([tgt, get_gt([H, W], rng.uniform(0, W * 4, 5), rng.uniform(0, H * 4, 5), v_s=np.arange(5), reduce=4,
                                    kernel_size=10)["heatmap"]])                                   # [2, 1, H, W]
    x = torch.randn(2, 1, H, W, generator=g, dtype=torch.float64) * 3 - 2.19
    x[0, 0, 0, :6] = torch.tensor([-9.5, 9.5, -12.0, 12.0, -9.0, 9.0], dtype=torch.float64)      # both sides of either clamp bound
    mask = (torch.rand(2, 1, H, W, generator=g) < 0.7).float()
    nopos = tgt2.clamp(max=0.98)
    fc = [(x, tgt2, None), (x, tgt2, mask), (x, nopos, None), (x, nopos, mask),
          (torch.randn(3, 2, 5, 7, generator=g, dtype=torch.float64), (torch.rand(3, 2, 5, 7, generator=g) * 1.25).clamp(max=1), None)]
    for i, (xi, ti, mi) in enumerate(fc):
        put(out, f"focal_{i}_x", xi, seen)
        put(out, f"focal_{i}_t", ti, seen)
        if mi is not None:
            put(out, f"focal_{i}_m", mi, seen)
        both(out, f"focal_{i}", lambda z: focal(z, ti, mi), xi)
    out["focal_cases"] = np.array(len(fc))

    # ---- masked L1 ----
    l1 = RegL1Loss()
    B, C, K = 2, 2, 12
    xo = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    ind = torch.randint(0, H * W, (B, K), generator=g)
    ind[0, 3] = ind[0, 1]                                                                          # two people in one cell
    ind[0, 7] = ind[0, 1]
    ind[1, 5] = ind[1, 4]
    m = torch.rand(B, K, generator=g) < 0.7
    m[0, 1] = m[0, 3] = m[0, 7] = m[1, 4] = m[1, 5] = True
    t = torch.rand(B, K, C, generator=g)
    t[0, 2] = xo[0, :, ind[0, 2] // W, ind[0, 2] % W].float()                                      # an exact zero difference in fp32
    m[0, 2] = True
    lc = [(xo, m, ind, t), (xo, torch.zeros_like(m), ind, t), (xo[:, :1].contiguous(), m, ind, t[:, :, :1].contiguous())]
    for i, (xi, mi, ii, ti) in enumerate(lc):
        for k, v in (("x", xi), ("mask", mi), ("ind", ii), ("t", ti)):
            put(out, f"l1_{i}_{k}", v, seen)
        both(out, f"l1_{i}", lambda z: l1(z, mi, ii, ti), xi)
    out["l1_cases"] = np.array(len(lc))

    # ---- RegCELoss, GaussianMSE ----
    ce = RegCELoss()
    xc = torch.randn(2, 5, 6, 7, generator=g, dtype=torch.float64)
    ic, mc, tc = torch.randint(0, 42, (2, 8), generator=g), torch.rand(2, 8, generator=g) < 0.6, torch.randint(0, 5, (2, 8), generator=g)
    out["ce_x"], out["ce_mask"], out["ce_ind"], out["ce_t"] = xc.numpy(), mc.numpy(), ic.numpy(), tc.numpy()
    both(out, "ce", lambda z: ce(z, mc, ic, tc), xc)
    out["ce_empty"] = np.array(float(ce(xc, torch.zeros_like(mc), ic, tc)))
    gm = GaussianMSE()
    xg, tg = torch.randn(1, 1, 6, 9, generator=g), (torch.rand(1, 1, 12, 18, generator=g) < 0.05).float()
    kern = torch.tensor([[1.0, 2.0, 1.0], [2.0, 4.0, 2.0], [1.0, 2.0, 1.0]]).view(1, 1, 3, 3) / 4
    out["gmse_x"], out["gmse_t"], out["gmse_k"] = xg.numpy(), tg.numpy(), kern.numpy()
    out["gmse_loss"], out["gmse_grad"] = run(lambda z: gm(z, tg, kern), xg, torch.float32)

    # ---- one mini-sized frame through trainer.py:52-63 ----
    N, (h, w) = 3, (18, 32)
    wg = get_gt([H, W], rng.uniform(0, W * 4, 8), rng.uniform(0, H * 4, 8), v_s=np.arange(8), reduce=4, kernel_size=10)
    views = [get_gt([h, w], rng.uniform(-10, w * 12 + 10, 8), rng.uniform(-10, h * 12 + 10, 8), rng.uniform(20, 64, 8),
                    rng.uniform(40, 72, 8), v_s=np.arange(8), reduce=12, kernel_size=10) for _ in range(N)]
    world_gt = {k: v[None] for k, v in wg.items()}
    imgs_gt = {k: torch.stack([v[k] for v in views])[None] for k in views[0]}
    heads = {"w_hm": torch.randn(1, 1, H, W, generator=g, dtype=torch.float64) * 2 - 2.19,
             "w_off": torch.randn(1, 2, H, W, generator=g, dtype=torch.float64),
             "i_hm": torch.randn(N, 1, h, w, generator=g, dtype=torch.float64) * 2 - 2.19,
             "i_off": torch.randn(N, 2, h, w, generator=g, dtype=torch.float64),
             "i_wh": torch.randn(N, 2, h, w, generator=g, dtype=torch.float64) * 3 + 4}
    for k, v in heads.items():
        out[f"frame_{k}"] = v.numpy()
    for k, v in world_gt.items():
        out[f"frame_world_{k}"] = v.numpy()
    for k, v in imgs_gt.items():
        out[f"frame_imgs_{k}"] = v.numpy()
    ig = {k: v.view([N] + list(v.shape)[2:]) for k, v in imgs_gt.items()}
    alpha = 1.0
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        p = {k: v.to(dtype) for k, v in heads.items()}
        terms = [focal(p["w_hm"], world_gt["heatmap"]),
                 l1(p["w_off"], world_gt["reg_mask"], world_gt["idx"], world_gt["offset"]),
                 focal(p["i_hm"], ig["heatmap"]),
                 l1(p["i_off"], ig["reg_mask"], ig["idx"], ig["offset"]),
                 l1(p["i_wh"], ig["reg_mask"], ig["idx"], ig["wh"])]
        total = (terms[0] + terms[1]) + (terms[2] + terms[3] + terms[4] * 0.1) / N * alpha
        out[f"frame_terms{tag}"] = np.array([float(v) for v in terms], dtype=np.float64)
        out[f"frame_total{tag}"] = np.array(float(total))
        mse = torch.nn.MSELoss()
        out[f"frame_mse{tag}"] = np.array(float(mse(p["w_hm"], world_gt["heatmap"].to(dtype)) + alpha * mse(p["i_hm"], ig["heatmap"].to(dtype))))

    path = os.path.join(HERE, "loss.npz")
    np.savez_compressed(path, **out)
    print("loss.npz:", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
