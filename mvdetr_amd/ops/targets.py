"""map_targets: the training targets of one segment of equally shaped maps, built where the annotations live
(csrc/frame_targets.hip; csrc/host_path.cpp for CPU tensors; the contract is in include/mvdetr_ops.h).

What the reference's dataset does on the CPU per map (multiview_detector/datasets/frameDataset.py:19-46 ``get_gt``, after the box half
of ``random_affine``, utils/image_utils.py:46-83): here one launch per segment over padded, fixed-capacity annotation tensors, so
nothing depends on a count the host would have to read back and nothing waits for the device.  ``mvdetr_amd.targets.get_gt`` and
``mvdetr_amd.augment.affine_boxes`` are the host yardsticks of the same arithmetic.

Two numbers are made on the host, so that the kernel needs no transcendental function and the host path, the kernel and the
yardsticks cannot differ in a last bit: the gaussian patch (``targets.gaussian_patch``, rounded to fp32, cached per
(kernel_size, reduce, device)) and, from ``angle``, the per-map shrink factor sqrt(max(|sin a|, |cos a|)).  An ``angle`` that
already lives on the device is turned into the factor there by torch (fp64), whose sin / cos may differ from libm's in the last bit.
"""
from __future__ import annotations

import math
import threading

import numpy as np
import torch

from .. import _lib
from ..targets import gaussian_patch
from .ingest import _MatUpload

MAX_CAP = 1024
MAX_DIM, MAX_MAPS = 16384, 65535


def launch_count() -> int:
    """Kernel launches of this process so far: one per device ``map_targets`` call."""
    return int(_lib.lib().mvdetr_frame_targets_launch_count())


def max_radius() -> int:
    """The largest patch radius int(3 kernel_size / reduce) the op takes."""
    return int(_lib.lib().mvdetr_frame_targets_max_radius())


_patches = {}
_uploads = {}
_lock = threading.Lock()


def _patch(kernel_size, reduce, dev):
    """(fp32 [2r + 1, 2r + 1] table on ``dev``, r) of get_gt's gaussian; made once per (kernel_size, reduce, device)."""
    sigma = kernel_size / reduce
    radius = int(3 * sigma)
    if radius > max_radius():
        raise RuntimeError(f"map_targets: kernel_size / reduce = {sigma} needs a patch of radius {radius}, the op takes at most "
                           f"{max_radius()}")
    key = (kernel_size, reduce, dev)
    with _lock:
        table = _patches.get(key)
        if table is None:
            table = torch.from_numpy(gaussian_patch(radius, sigma).astype(np.float32))
            if dev.type == "cuda":
                table = table.pin_memory().to(dev, non_blocking=True)
            _patches[key] = table
    return table, radius


def _to_device(t, dev, what):
    """A float64 tensor where the annotations live; a CPU one goes up through this (device, thread, shape)'s pinned ring."""
    t = t.detach().to(torch.float64).contiguous()
    if t.device == dev:
        return t
    if t.device.type != "cpu":
        raise RuntimeError(f"map_targets: {what} lives on {t.device}, the annotations on {dev}")
    key = (dev.index, threading.get_ident(), tuple(t.shape))
    with _lock:
        ring = _uploads.setdefault(key, _MatUpload())
    return ring.upload(t, dev)


def _shrink(angle, dev):
    """[maps] float64 sqrt(max(|sin a|, |cos a|)) of ``angle`` in degrees, as augment.affine_boxes forms it."""
    if angle.device.type == "cpu":
        rad = [a * math.pi / 180 for a in angle.to(torch.float64).tolist()]
        host = torch.tensor([math.sqrt(max(abs(math.sin(r)), abs(math.cos(r)))) for r in rad], dtype=torch.float64)
        return _to_device(host, dev, "angle")
    if angle.device != dev:
        raise RuntimeError(f"map_targets: angle lives on {angle.device}, the annotations on {dev}")
    rad = angle.to(torch.float64) * math.pi / 180
    return torch.sqrt(torch.maximum(torch.sin(rad).abs(), torch.cos(rad).abs())).contiguous()


def map_targets(Rshape, *, points=None, boxes=None, count, pids=None, M=None, angle=None, img_hw=None, keep=None, reduce,
                kernel_size, top_k=100):
    """The targets of ``maps`` maps of shape ``Rshape`` = (H, W) from padded annotations, ``get_gt``'s keys, dtypes and collated
    shapes on the annotations' device: heatmap [maps, 1, H, W] fp32, reg_mask [maps, top_k] bool, idx and pid [maps, top_k]
    int64, offset [maps, top_k, 2] fp32 and, for boxes, wh [maps, top_k, 2] fp32.

    Exactly one of ``points`` [maps, cap, 2] (x, y) and ``boxes`` [maps, cap, 4] (x1, y1, x2, y2; the point is the bottom centre),
    at ``reduce`` times the map's resolution, float64 (float32 is upcast); ``count`` [maps] int32, the valid objects of each map;
    ``pids`` [maps, cap] int64 (zeros without).  Boxes only: ``M`` [maps, 3, 3], the matrices ``augment.random_affine`` returns,
    moves the boxes as ``augment.affine_boxes`` does (hull, shrink by ``angle`` [maps] in degrees, clip to ``img_hw``, the three
    keep rules) and compacts the kept ones in order; without ``M`` slot k is object k.  ``M`` and ``angle`` may be CPU tensors
    with everything else on the device: they go up asynchronously through pinned staging.  ``keep`` [maps] bool: a map with
    keep == 0 gets all-zero outputs (camera dropout).  ``cap <= top_k`` (ValueError otherwise), so no object can overflow.

    CPU tensors run the library's host path, CUDA tensors the kernel (one launch; nothing waits for the device)."""
    if (points is None) == (boxes is None):
        raise RuntimeError("map_targets: give exactly one of points and boxes")
    is_boxes = boxes is not None
    coords, width, name = (boxes, 4, "boxes") if is_boxes else (points, 2, "points")
    if not isinstance(coords, torch.Tensor) or coords.dim() != 3 or coords.shape[2] != width:
        raise RuntimeError(f"map_targets: {name} must be [maps, cap, {width}], got {tuple(getattr(coords, 'shape', ()))}")
    if coords.dtype not in (torch.float64, torch.float32):
        raise RuntimeError(f"map_targets: {name} must be float64 or float32, got {coords.dtype}")
    maps, cap = int(coords.shape[0]), int(coords.shape[1])
    dev = coords.device
    top_k = int(top_k)
    if cap > top_k:
        raise ValueError(f"map_targets: {name} {tuple(coords.shape)} hold up to {cap} objects per map but there are only top_k = "
                         f"{top_k} slots")
    if cap < 1 or cap > MAX_CAP or maps > MAX_MAPS:
        raise RuntimeError(f"map_targets: needs 1 <= cap <= {MAX_CAP} and at most {MAX_MAPS} maps, got {name} {tuple(coords.shape)}")
    H, W = int(Rshape[0]), int(Rshape[1])
    if min(H, W) < 1 or max(H, W) > MAX_DIM:
        raise RuntimeError(f"map_targets: map sizes must lie in [1, {MAX_DIM}], got {(H, W)}")
    if not reduce > 0:
        raise RuntimeError(f"map_targets: reduce must be positive, got {reduce}")

    def resident(t, what, shape, dtype):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise RuntimeError(f"map_targets: {what} must be {list(shape)}, got {tuple(getattr(t, 'shape', ()))}")
        if t.dtype != dtype:
            raise RuntimeError(f"map_targets: {what} must be {dtype}, got {t.dtype}")
        if t.device != dev:
            raise RuntimeError(f"map_targets: {what} lives on {t.device}, {name} on {dev}")
        return t.detach().contiguous()

    count = resident(count, "count", (maps,), torch.int32)
    if pids is not None:
        pids = resident(pids, "pids", (maps, cap), torch.int64)
    if keep is not None:
        keep = resident(keep, "keep", (maps,), torch.bool)
    if not is_boxes and (M is not None or angle is not None):
        raise RuntimeError("map_targets: M and angle move boxes; points take neither")
    shrink = None
    if M is not None:
        if not isinstance(M, torch.Tensor) or tuple(M.shape) != (maps, 3, 3) or not M.is_floating_point():
            raise RuntimeError(f"map_targets: M must be float [{maps}, 3, 3], got {tuple(getattr(M, 'shape', ()))}")
        if img_hw is None:
            raise RuntimeError("map_targets: M needs img_hw = (height, width), the image the moved boxes are clipped to")
        M = _to_device(M, dev, "M")
        if angle is not None:
            if not isinstance(angle, torch.Tensor) or tuple(angle.shape) != (maps,):
                raise RuntimeError(f"map_targets: angle must be [{maps}], got {tuple(getattr(angle, 'shape', ()))}")
            shrink = _shrink(angle.detach(), dev)
    elif angle is not None:
        raise RuntimeError("map_targets: angle without M (the shrink belongs to the move by M)")
    img_h, img_w = (int(img_hw[0]), int(img_hw[1])) if img_hw is not None else (0, 0)
    if M is not None and min(img_h, img_w) < 1:
        raise RuntimeError(f"map_targets: img_hw must be positive, got {(img_h, img_w)}")
    patch, radius = _patch(kernel_size, reduce, dev)
    coords = coords.detach().to(torch.float64).contiguous()

    new = lambda *shape, dtype: torch.empty(maps, *shape, dtype=dtype, device=dev)  # noqa: E731
    gt = {"heatmap": new(1, H, W, dtype=torch.float32), "reg_mask": new(top_k, dtype=torch.bool),
          "idx": new(top_k, dtype=torch.int64), "pid": new(top_k, dtype=torch.int64), "offset": new(top_k, 2, dtype=torch.float32)}
    if is_boxes:
        gt["wh"] = new(top_k, 2, dtype=torch.float32)
    if maps == 0:
        return gt
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    args = (coords.data_ptr(), 1 if is_boxes else 0, count.data_ptr(), ptr(pids), ptr(M), ptr(shrink), ptr(keep), patch.data_ptr(),
            maps, cap, H, W, img_h, img_w, radius, top_k, float(reduce), gt["heatmap"].data_ptr(), gt["reg_mask"].data_ptr(),
            gt["idx"].data_ptr(), gt["pid"].data_ptr(), gt["offset"].data_ptr(), ptr(gt.get("wh")))
    lib = _lib.lib()
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            rc = lib.mvdetr_frame_targets_f64(_lib.current_stream_ptr(dev), *args)
    else:
        rc = lib.mvdetr_frame_targets_host_f64(*args)
    _lib.check(rc, "map_targets")
    return gt
