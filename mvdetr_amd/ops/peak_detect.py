"""Peak extraction where the maps live: heat-map logits (+ offset, + wh maps) -> the top_k local maxima of every map in one
fused sigmoid + 3x3 peak test + threshold + ordered top-K + gathers (csrc/peak_detect.hip; csrc/host_path.cpp for CPU tensors).

Replaces, for single-channel maps that stay on the device, the reference's ``ctdet_decode`` (multiview_detector/utils/decode.py:
7-77, run on the image heads at trainer.py:173): nothing here waits for the GPU and nothing is read back -- the result is a
fixed-capacity tensor per map plus the number of candidates, all on the device.

A cell is a candidate when its score equals the maximum of the scores of its 3x3 neighbourhood inside the map (compared on the
sigmoid's outputs, as the reference does: a plateau of equal scores is kept whole) and, with ``cls_thres``, lies above it.

Tie rule (this library's, ops/detect.py; ``torch.topk``'s order among equal scores is unspecified): candidates of equal score
come higher row-major cell index first.  On tie-free input the rows are the reference's; rows past ``count`` are zero.

Deviation: a NaN logit is never a candidate and is ignored in its neighbours' maxima, where ``max_pool2d`` propagates the NaN
and so erases the eight cells around it.  Non-finite logits are outside the parity contract; they neither fault nor hang.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import torch

from .. import _lib

MAX_TOP_K = 1024


class PeakDetections(NamedTuple):
    """``peak_detect``'s result; everything lives on the inputs' device.  Rows of a map are in descending score order (equal
    scores: higher cell first); rows at and after ``min(count, top_k)`` are zero."""
    xy: torch.Tensor                # [B, top_k, 2] map cells: column + dx, row + dy
    wh: Optional[torch.Tensor]      # [B, top_k, 2] the gathered sizes, unscaled; None without a wh map
    box: Optional[torch.Tensor]     # [B, top_k, 4] (x1, y1, x2, y2) * scale, the point being the box's bottom centre; None without wh
    score: torch.Tensor             # [B, top_k]
    cell: torch.Tensor              # [B, top_k] int32 row-major index of the heat-map cell
    count: torch.Tensor             # [B] int32: the true number of candidates, also when it exceeds top_k


def _strides(t: torch.Tensor):
    return (ctypes.c_int64 * 4)(*t.stride())


def last_kernel() -> str:
    """The route of the last device call; waits for the device (the candidate counts choose the route there)."""
    return _lib.lib().mvdetr_peak_detect_last_kernel().decode()


def launch_count() -> int:
    return int(_lib.lib().mvdetr_peak_detect_launch_count())


def lds_capacity(dtype) -> int:
    """The number of candidates of one map that the device keeps in LDS; beyond it the list lives in the workspace."""
    return int(_lib.lib().mvdetr_peak_detect_lds_capacity(torch.empty(0, dtype=dtype).element_size()))


def peak_detect(heatmap, offset=None, wh=None, *, top_k=100, cls_thres=None, scale=1.0) -> PeakDetections:
    """heatmap [B,1,H,W] raw logits, offset and wh [B,2,H,W] or None, any strides (channels_last maps are read in place), one
    device and one dtype (float32 / float64).  ``cls_thres=None``: no threshold.  Not differentiable."""
    hm = heatmap.detach()
    if hm.dim() != 4:
        raise RuntimeError(f"heatmap must be [B, 1, H, W], got {tuple(hm.shape)}")
    if hm.shape[1] != 1:
        raise RuntimeError(f"heatmap must have one channel ([B, 1, H, W]), got {tuple(hm.shape)}")
    B, _, H, W = hm.shape
    maps = []
    for name, t in (("offset", offset), ("wh", wh)):
        if t is not None:
            t = t.detach()
            if t.shape != (B, 2, H, W):
                raise RuntimeError(f"{name} must be [{B}, 2, {H}, {W}], got {tuple(t.shape)}")
            if t.device != hm.device or t.dtype != hm.dtype:
                raise RuntimeError(f"heatmap and {name} must share device and dtype")
        maps.append(t)
    off, size = maps
    sfx = _lib.suffix(hm.dtype)
    top_k = int(top_k)
    if top_k < 1 or top_k > MAX_TOP_K:
        raise RuntimeError(f"peak_detect needs 1 <= top_k <= {MAX_TOP_K}, got {top_k}")
    if B < 1 or H * W < 1:
        raise RuntimeError("peak_detect needs a non-empty map")
    new = lambda *shape, dtype=hm.dtype: torch.empty(B, top_k, *shape, dtype=dtype, device=hm.device)  # noqa: E731
    xy, score, cell = new(2), new(), new(dtype=torch.int32)
    wh_out, box = (None, None) if size is None else (new(2), new(4))
    count = torch.empty(B, dtype=torch.int32, device=hm.device)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    args = (hm.data_ptr(), _strides(hm), ptr(off), _strides(hm if off is None else off), ptr(size),
            _strides(hm if size is None else size), B, H, W, top_k, 0.0 if cls_thres is None else float(cls_thres),
            0 if cls_thres is None else 1, float(scale))
    outs = (xy.data_ptr(), ptr(wh_out), ptr(box), score.data_ptr(), cell.data_ptr(), count.data_ptr())
    lib = _lib.lib()
    if hm.is_cuda:
        nbytes = lib.mvdetr_peak_detect_workspace_bytes(B, H, W, hm.element_size())
        if nbytes < 0:
            raise RuntimeError(f"peak_detect: unsupported map size {B} x {H} x {W}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=hm.device)
        with torch.cuda.device(hm.device):
            rc = getattr(lib, f"mvdetr_peak_detect_forward_{sfx}")(_lib.current_stream_ptr(hm.device), *args, ws.data_ptr(), *outs)
    else:
        rc = getattr(lib, f"mvdetr_peak_detect_forward_host_{sfx}")(*args, *outs)
    _lib.check(rc, "peak_detect")
    return PeakDetections(xy, wh_out, box, score, cell, count)
