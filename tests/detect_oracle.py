"""Expected values for the fused detection extraction (ops/detect.py): the reference's chain restated from the checker's own
pieces -- ``torch.sigmoid`` on the CPU, ``post_oracle.mvdet_decode``, the threshold rounded to the tensor's dtype, and
``post_oracle.nms(..., order=None)`` (a stable ascending sort popped from the end: equal scores, higher index first, the
library's tie rule).  tests/test_postprocess.py pins those pieces to the reference's own goldens.

Inputs are robust to a last-place difference of ``exp`` between devices: logits come from the lattice k/32, k in [-256, 256],
on which different scores are >= 1e-5 apart and none is within 1e-4 of the threshold, while equal logits give exactly equal
scores everywhere.  ``check_input`` asserts both properties; every case is checked when it is built.

``post_oracle`` computes in fp32.  The fp64 cases keep offsets on the lattice k/64, so every position is exact in both
precisions and squared distances differ from their fp32 roundings by far less than the nearest pair's distance from the
threshold; their scores and the candidate test are taken from the fp64 sigmoid itself.

Results are computed once per case and shared by the CPU and the GPU tests (``expected`` is cached; treat it as read-only)."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import post_oracle  # noqa: E402

CLS_THRES, DIST_THRES, REDUCE = 0.4, 20, 4
MIN_SCORE_GAP, MIN_THRES_GAP = 1e-5, 1e-4
SCORE_TOL = {torch.float32: 1e-6, torch.float64: 1e-14}


def lattice(shape, gen, lo=-256, hi=256):
    return torch.randint(lo, hi + 1, shape, generator=gen).float() / 32


def check_input(logits, cls_thres=CLS_THRES):
    """The two properties that make a case independent of the device's exp: separated scores, none near the threshold."""
    s = torch.unique(torch.sigmoid(logits.detach().double().flatten()))
    if s.numel() > 1:
        assert float((s[1:] - s[:-1]).min()) >= MIN_SCORE_GAP, float((s[1:] - s[:-1]).min())
    assert float((s - cls_thres).abs().min()) >= MIN_THRES_GAP, float((s - cls_thres).abs().min())


def reference(logits, offset, reduce=REDUCE, cls_thres=CLS_THRES, dist_thres=DIST_THRES, top_k=float("inf"), indexing="xy"):
    """-> per frame (cells int64 [count], xy [count, 2], score [count]) in kept order, arrays of the logits' dtype."""
    logits, offset = logits.detach().cpu(), None if offset is None else offset.detach().cpu()
    dt = logits.numpy().dtype.type
    s = torch.sigmoid(logits).contiguous().numpy()
    rows = post_oracle.mvdet_decode(s, None if offset is None else offset.contiguous().numpy(), reduce)
    if dt is np.float64:                         # fp32 restatement: exact only for offsets on the k/64 lattice (asserted)
        off64 = np.zeros((1, 2, 1, 1)) + 0.5 if offset is None else offset.numpy()
        assert np.array_equal(off64 * 64, np.round(off64 * 64)) and float(np.abs(off64).max()) < 1024
    out = []
    for b in range(logits.shape[0]):
        score = s[b, 0].reshape(-1)
        sel = np.nonzero(score > dt(cls_thres))[0]
        pos = rows[b, sel, :2]
        if indexing != "xy":
            pos = pos[:, [1, 0]]
        keep, count = post_oracle.nms(pos.tolist(), score[sel].tolist(), dist_thres, top_k, order=None)
        keep = np.asarray(keep[:count], dtype=np.int64)
        out.append((sel[keep], pos[keep].astype(dt).reshape(-1, 2), score[sel][keep]))
    return out


def _offsets(shape, gen, sigma, dtype=torch.float32):
    B, _, H, W = shape
    if dtype == torch.float64:
        return (torch.randn(B, 2, H, W, generator=gen) * sigma * 64).round().double() / 64
    return torch.randn(B, 2, H, W, generator=gen) * sigma


def _background(shape, gen):
    """lattice logits all below the threshold: sigmoid(-13/32) = 0.3998 is the first score under 0.4"""
    return lattice(shape, gen, -256, -13)


def make_case(name):
    """-> (logits [B,1,H,W], offset [B,2,H,W] or None, keyword arguments of bev_detect)."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    kw = {}
    if name == "one_cell":
        hm, off = torch.full((1, 1, 1, 1), 1.0), _offsets((1, 1, 1, 1), g, 8)
    elif name in ("one_frame_empty", "no_offset", "ij", "top9_of_random"):
        hm = lattice((3, 1, 5, 7), g)
        hm[1] = _background((1, 5, 7), g)
        off = None if name == "no_offset" else _offsets(hm.shape, g, 8)
        if name == "ij":
            kw["indexing"] = "ij"
        if name == "top9_of_random":
            kw["top_k"] = 9
    elif name in ("all_above", "all_above_f64", "all_above_cap5"):
        # 960 candidates, positions sigma = 8 cells away from their cells: many per lane, many sequential keeps, many ties
        hm = lattice((2, 1, 24, 40), g, -12, 256)
        off = _offsets(hm.shape, g, 8, torch.float64 if name.endswith("f64") else torch.float32)
        if name.endswith("f64"):
            hm = hm.double()
        if name.endswith("cap5"):
            kw["max_det"] = 5
    elif name in ("beyond_a_workgroup", "beyond_a_workgroup_f64"):
        hm = lattice((1, 1, 40, 48), g, -12, 256)                          # 1,920 candidates > 1,024 threads (and > 1,728: fp64 leaves LDS)
        off = _offsets(hm.shape, g, 8, torch.float64 if name.endswith("f64") else torch.float32)
        if name.endswith("f64"):
            hm = hm.double()
    elif name == "exact_distance":
        # zero offsets, reduce 4: (3, 4) cells apart is exactly 20 -> suppressed; 6 cells in a row is 24 -> both kept
        hm = torch.full((1, 1, 16, 24), -4.0)
        hm[0, 0, 2, 3], hm[0, 0, 5, 7] = 3.0, 2.0
        hm[0, 0, 12, 3], hm[0, 0, 12, 9] = 2.5, 1.5
        off = torch.zeros(1, 2, 16, 24)
    elif name in ("plateau", "plateau_f64"):
        hm = _background((2, 1, 8, 12), g)
        hm[:, :, 2:6, 3:8] = 2.0
        hm[1, 0, 3, 4] = 2.5
        off = _offsets(hm.shape, g, 2, torch.float64 if name.endswith("f64") else torch.float32)
        if name.endswith("f64"):
            hm = hm.double()
    elif name in ("top9", "top50"):
        # k - 1 distinct scores, then three equal ones straddling the cut, then twenty lower ones
        k = int(name[3:])
        hm = _background((1, 1, 16, 24), g)
        cells = torch.randperm(16 * 24, generator=g)
        flat = hm.view(-1)
        for i in range(k - 1):
            flat[cells[i]] = (256 - i) / 32
        flat[cells[k - 1:k + 2]] = (256 - k) / 32
        for i in range(20):
            flat[cells[k + 2 + i]] = (256 - k - 1 - i) / 32
        off = _offsets(hm.shape, g, 8)
        kw["top_k"], kw["dist_thres"] = k, 6                               # few suppressions: the cut decides who is kept
    else:
        raise KeyError(name)
    check_input(hm)
    return hm, off, kw


def call_kw(kw):
    """bev_detect's keyword arguments for a case: the reference test loop's settings unless the case sets its own."""
    return dict(dict(world_reduce=REDUCE, cls_thres=CLS_THRES, dist_thres=DIST_THRES), **kw)


CASES = ["one_cell", "one_frame_empty", "all_above", "beyond_a_workgroup", "exact_distance", "plateau", "top9", "top50",
         "top9_of_random", "no_offset", "ij", "all_above_cap5", "all_above_f64", "beyond_a_workgroup_f64", "plateau_f64"]


@functools.lru_cache(maxsize=None)
def expected(name):
    hm, off, kw = make_case(name)
    ref_kw = {k: v for k, v in kw.items() if k != "max_det"}
    return reference(hm, off, **ref_kw)


def assert_matches(det, name, hm):
    """A bev_detect result against the case's expectation: cells, counts, positions bit-exact; scores within SCORE_TOL; rows at
    and after min(count, max_det) zero."""
    want = expected(name)
    xy, score, cell, count = [t.cpu() for t in det]
    cap = score.shape[1]
    assert count.dtype == torch.int32 and cell.dtype == torch.int32 and xy.dtype == score.dtype == hm.dtype
    assert count.tolist() == [len(w[0]) for w in want], (count.tolist(), [len(w[0]) for w in want])
    for b, (cells, pos, sc) in enumerate(want):
        m = min(len(cells), cap)
        assert cell[b, :m].tolist() == cells[:m].tolist(), (name, b)
        assert np.array_equal(xy[b, :m].numpy(), pos[:m]), (name, b)
        err = np.abs(score[b, :m].numpy().astype(np.float64) - sc[:m].astype(np.float64)).max() if m else 0.0
        print(f"{name}[{b}]: kept {len(cells)}, score error {err:.3g}")
        assert err <= SCORE_TOL[hm.dtype], (name, b, err)
        assert not xy[b, m:].any() and not score[b, m:].any() and not cell[b, m:].any(), (name, b)
