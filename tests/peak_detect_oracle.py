"""Expected values for the fused peak extraction (ops/peak_detect.py): a numpy restatement of the definition -- CPU
``torch.sigmoid`` (evaluated once per distinct logit, so equal logits are equal scores), a 3x3 maximum over a -inf padded
plane, the threshold rounded to the tensor's dtype, a ``lexsort`` by (-score, -cell) (the library's tie rule: equal scores,
higher row-major cell first), gathers, and the box formula with every operation rounded in the tensor's dtype.
tests/test_peak_detect.py pins ``utils.ctdet_decode`` to the reference's own goldens and the fused path to ``ctdet_decode``.

Inputs are robust to a last-place difference of ``exp`` between devices: logits come from the lattice k/32, |k| <= 256
(``detect_oracle.lattice`` / ``check_input``): different scores are >= 1e-5 apart, none is within 1e-4 of the threshold, and
equal logits are exact ties everywhere.

Bars: cell, count, xy, wh, box and the zero tail bit-exact; score within ``SCORE_TOL`` (1e-6 fp32, 1e-14 fp64, the project's
bar for the same sigmoid).  Results are computed once per case and shared by the CPU and the GPU tests (``expected`` is cached;
treat it as read-only)."""
import functools

import numpy as np
import torch

from detect_oracle import SCORE_TOL, check_input, lattice

RUN = 1024                        # cells per peak_compact workgroup (csrc/peak_detect.hip PK_TILE)


def reference(logits, offset, wh, top_k=100, cls_thres=None, scale=1.0):
    """-> per map a dict: count, and the first min(count, top_k) rows' cell, xy, wh, box, score (arrays of the logits' dtype)."""
    logits = logits.detach().cpu()
    dt = logits.numpy().dtype.type
    B, _, H, W = logits.shape
    uniq, inv = torch.unique(logits, return_inverse=True)
    s_all = torch.sigmoid(uniq)[inv].numpy()
    off = None if offset is None else offset.detach().cpu().numpy()
    size = None if wh is None else wh.detach().cpu().numpy()
    out = []
    for b in range(B):
        s = s_all[b, 0]
        pad = np.full((H + 2, W + 2), -np.inf, dtype=s.dtype)
        pad[1:-1, 1:-1] = s
        hmax = np.max(np.stack([pad[1 + dr:1 + dr + H, 1 + dc:1 + dc + W] for dr in (-1, 0, 1) for dc in (-1, 0, 1)]), axis=0)
        keep = s == hmax
        if cls_thres is not None:
            keep &= s > dt(cls_thres)
        cells = np.nonzero(keep.reshape(-1))[0]
        sc = s.reshape(-1)[cells]
        order = np.lexsort((-cells, -sc.astype(np.float64)))
        cells, sc = cells[order][:top_k], sc[order][:top_k]
        rows, cols = cells // W, cells % W
        dx = dt(0.5) if off is None else off[b, 0, rows, cols]
        dy = dt(0.5) if off is None else off[b, 1, rows, cols]
        x, y = cols.astype(dt) + dx, rows.astype(dt) + dy
        res = {"count": int(keep.sum()), "cell": cells, "xy": np.stack([x, y], 1).astype(dt), "score": sc, "wh": None, "box": None}
        if size is not None:
            w, h = size[b, 0, rows, cols], size[b, 1, rows, cols]
            half = dt(0.5) * w
            k = dt(scale)
            res["wh"] = np.stack([w, h], 1)
            res["box"] = np.stack([(x - half) * k, (y - h) * k, (x + half) * k, y * k], 1).astype(dt)
            assert res["box"].dtype == res["wh"].dtype == s.dtype
        out.append(res)
    return out


def _ramp(B, H, W):
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return ((-256 + xs + ys).float() / 32).repeat(B, 1, 1, 1)


def _maps(shape, gen, dtype):
    B, _, H, W = shape
    off = torch.randn(B, 2, H, W, generator=gen, dtype=dtype)
    wh = torch.rand(B, 2, H, W, generator=gen, dtype=dtype) * 6 + 1
    return off, wh


def make_case(name):
    """-> (logits [B,1,H,W], offset [B,2,H,W] or None, wh [B,2,H,W] or None, keyword arguments of peak_detect)."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    f64 = name.endswith("_f64")
    base = name[:-4] if f64 else name
    kw = {"top_k": 100, "scale": 12.0}
    if base == "one_cell":
        hm = torch.full((1, 1, 1, 1), 1.0)
    elif base == "one_row":
        hm = lattice((2, 1, 1, 9), g)                                      # no row above or below
    elif base == "one_column":
        hm = lattice((2, 1, 9, 1), g)                                      # no column left or right
    elif base in ("corners_and_edges", "top_1", "no_offset", "no_wh", "no_offset_no_wh"):
        # 5 x 7: frame 0 has peaks in all four corners and on every edge, frame 1 is the bare ramp (one peak), frame 2 noise
        hm = _ramp(3, 5, 7)
        for i, (r, c) in enumerate([(0, 0), (0, 6), (4, 0), (4, 6), (0, 3), (2, 0), (2, 6), (4, 3)]):
            hm[0, 0, r, c] = (40 + 7 * i) / 32
        hm[2] = lattice((1, 5, 7), g)
        if base == "top_1":
            kw["top_k"] = 1
    elif base == "plateau":
        hm = lattice((2, 1, 8, 12), g, -256, -13)
        hm[:, :, 2:6, 3:8] = 2.0                                           # 20 equal cells: all of them are kept
        hm[1, 0, 3, 4] = 2.5                                               # one higher cell inside: its 8 neighbours go
    elif base == "seam":
        # 40 x 48: the first run of 1024 cells ends mid-row, at (21, 15); c is the first cell of the second run
        H, W, c = 40, 48, RUN
        hm = lattice((3, 1, H, W), g, -256, 223)                           # noise below every planted value
        flat = hm.view(3, -1)
        assert c % W not in (0, W - 1) and c + W + 4 < H * W
        flat[0, c - 1] = flat[0, c] = 7.5                                  # an equal pair, one cell in either run
        flat[1, c] = flat[1, c - W] = 7.5                                  # an equal pair over the row above the boundary
        flat[1, c - 6] = flat[1, c - 6 + W] = 7.25                         # and over the row below it
        flat[2, c - 1], flat[2, c + W] = 7.5, 7.0                          # a peak before the boundary hides one below, after it
        flat[2, c + 3], flat[2, c + 2 - W] = 7.75, 7.0                     # a peak after the boundary hides one above, before it
    elif base in ("top_9", "top_50"):
        # k - 1 distinct scores, then three equal ones straddling the cut, then twenty lower ones, all on non-adjacent sites
        k = int(base[4:])
        H, W = 16, 24
        hm = lattice((1, 1, H, W), g, -256, -13)
        sites = [r * W + c for r in range(1, H, 2) for c in range(1, W, 2)]
        cells = [sites[i] for i in torch.randperm(len(sites), generator=g).tolist()]
        flat = hm.view(-1)
        for i in range(k - 1):
            flat[cells[i]] = (256 - i) / 32
        for cell in cells[k - 1:k + 2]:
            flat[cell] = (256 - k) / 32
        for i in range(20):
            flat[cells[k + 2 + i]] = (256 - k - 1 - i) / 32
        kw["top_k"] = k
    elif base in ("constant_100", "constant_1024"):
        hm = torch.full((2, 1, 72, 96), 0.25)                              # every cell is a candidate: the workspace route
        hm[1] = -3.0
        kw["top_k"] = int(base[9:])
    elif base == "threshold":
        hm = lattice((2, 1, 24, 40), g)
        kw["cls_thres"] = 0.4
    elif base == "views_full_size":
        hm = lattice((7, 1, 90, 160), g)
    elif base == "world_full_size":
        hm = lattice((1, 1, 120, 360), g)
    else:
        raise KeyError(name)
    check_input(hm)
    dtype = torch.float64 if f64 else torch.float32
    off, wh = _maps(hm.shape, g, dtype)
    if base in ("no_offset", "no_offset_no_wh"):
        off = None
    if base in ("no_wh", "no_offset_no_wh"):
        wh = None
    return hm.to(dtype), off, wh, kw


CASES = ["one_cell", "one_row", "one_column", "corners_and_edges", "plateau", "seam", "top_9", "top_50", "top_1", "constant_100",
         "constant_1024", "threshold", "no_offset", "no_wh", "no_offset_no_wh", "plateau_f64", "seam_f64", "constant_100_f64",
         "views_full_size", "world_full_size"]
WORKSPACE_ROUTE = ["constant_100", "constant_1024", "constant_100_f64"]   # more candidates than the LDS list holds


@functools.lru_cache(maxsize=None)
def expected(name):
    hm, off, wh, kw = make_case(name)
    return reference(hm, off, wh, **kw)


def assert_matches(det, name, hm):
    """A peak_detect result against the case's expectation."""
    want = expected(name)
    xy, wh, box, score, cell, count = [None if t is None else t.cpu() for t in det]
    cap = score.shape[1]
    assert count.dtype == torch.int32 and cell.dtype == torch.int32 and xy.dtype == score.dtype == hm.dtype
    assert count.tolist() == [w["count"] for w in want], (count.tolist(), [w["count"] for w in want])
    assert (wh is None) == (want[0]["wh"] is None) and (box is None) == (want[0]["box"] is None)
    worst = 0.0
    for b, w in enumerate(want):
        m = min(w["count"], cap)
        assert len(w["cell"]) == m
        assert cell[b, :m].tolist() == w["cell"].tolist(), (name, b)
        assert np.array_equal(xy[b, :m].numpy(), w["xy"]), (name, b)
        err = np.abs(score[b, :m].numpy().astype(np.float64) - w["score"].astype(np.float64)).max() if m else 0.0
        worst = max(worst, float(err))
        assert err <= SCORE_TOL[hm.dtype], (name, b, err)
        assert not xy[b, m:].any() and not score[b, m:].any() and not cell[b, m:].any(), (name, b)
        if wh is not None:
            assert wh.dtype == box.dtype == hm.dtype
            assert np.array_equal(wh[b, :m].numpy(), w["wh"]) and np.array_equal(box[b, :m].numpy(), w["box"]), (name, b)
            assert not wh[b, m:].any() and not box[b, m:].any(), (name, b)
    print(f"{name}: counts {count.tolist()}, score error {worst:.3g}")
