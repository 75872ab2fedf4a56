#!/usr/bin/env python3
"""Golden vectors for the peak decoder of the image heads, made by RUNNING the reference's own ``ctdet_decode``
(multiview_detector/utils/decode.py:47-77, imported from a checkout of the reference named by MVDETR_REFERENCE -- build
container only; nothing of it is copied) on the CPU.

    python tests/golden/make_golden_ctdet.py

Writes ctdet.npz: ctdet_{i}_heatmap / _offset / _wh / _top_K -> ctdet_{i}_out, and ctdet_cases.

The inputs make the reference deterministic (``torch.topk``'s order among equal scores is unspecified): every row it returns
with a positive score has a score that no other candidate shares.  Background: the ramp (-256 + x + y) / 32 on 24 x 40, whose
only peak is the bottom-right corner.  Spikes: at odd (row, column) sites other than that corner, so no two are adjacent, with
distinct values k / 32, k in [-192, 256], all above the ramp.  n spikes give n + 1 candidates per channel; rows past the last
candidate have score exactly 0 (non-peaks are multiplied by zero) and are not compared by the tests."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("MVDETR_REFERENCE", "/root/reference"))

from multiview_detector.utils.decode import ctdet_decode  # noqa: E402

H, W = 24, 40


def heatmap(batch, channels, spikes, gen):
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    hm = ((-256 + xs + ys).float() / 32).repeat(batch, channels, 1, 1)
    sites = [(r, c) for r in range(1, H, 2) for c in range(1, W, 2) if (r, c) != (H - 1, W - 1)]
    for b in range(batch):
        values = torch.randperm(449, generator=gen)[:channels * spikes] - 192          # distinct over the channels of a map
        for ch in range(channels):
            where = torch.randperm(len(sites), generator=gen)[:spikes]
            for i, s in enumerate(where.tolist()):
                hm[b, ch, sites[s][0], sites[s][1]] = float(values[ch * spikes + i]) / 32
    return hm


def main():
    g = torch.Generator().manual_seed(7)
    out = {}
    cases = [(1, 150, True, True), (1, 150, True, False), (1, 150, False, True), (1, 150, False, False), (1, 30, True, True),
             (1, 30, False, False), (2, 75, True, True)]
    for i, (channels, spikes, with_off, with_wh) in enumerate(cases):
        hm = heatmap(2, channels, spikes, g)
        off = torch.rand(2, 2, H, W, generator=g) if with_off else None
        wh = torch.rand(2, 2, H, W, generator=g) * 6 + 1 if with_wh else None
        rows = ctdet_decode(hm, off, wh, top_K=100)
        score = rows[..., -1]
        cand = torch.sigmoid(hm) * (torch.nn.functional.max_pool2d(torch.sigmoid(hm), 3, 1, 1) == torch.sigmoid(hm))
        for b in range(2):
            pos = score[b][score[b] > 0]
            assert len(pos) == min(100, channels * (spikes + 1)), len(pos)
            for v in pos.tolist():                                                  # a returned score is nobody else's
                assert int((cand[b] == v).sum()) == 1
        out[f"ctdet_{i}_heatmap"] = hm.numpy()
        if with_off:
            out[f"ctdet_{i}_offset"] = off.numpy()
        if with_wh:
            out[f"ctdet_{i}_wh"] = wh.numpy()
        out[f"ctdet_{i}_top_K"] = np.array(100)
        out[f"ctdet_{i}_out"] = rows.numpy()
    out["ctdet_cases"] = np.array(len(cases))
    path = os.path.join(HERE, "ctdet.npz")
    np.savez_compressed(path, **out)
    print("ctdet.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
