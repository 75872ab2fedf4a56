"""ingest_frames: decoded camera frames (uint8, HWC) -> the trunk's input in one HIP pass.

What the reference's dataset does on the CPU per camera (multiview_detector/datasets/frameDataset.py:66-67,199-206):
the optional ``random_affine`` image warp (utils/image_utils.py:43, ``cv2.warpPerspective``), ``ToTensor``, ``Normalize`` and
``Resize`` -- here one kernel that reads the uint8 frames once and writes the normalised, resized images once, in the dtype and
memory format the trunk runs in (csrc/ingest.hip; the contract is in include/mvdetr_ops.h).  The matrix ``M`` is the one
``MVDeTr.forward`` takes (the "view-coherent augmentation"); ``mvdetr_amd.augment`` draws it and moves the boxes with it.
"""
from __future__ import annotations

import threading

import torch

from .. import _lib

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HALF_DTYPES = (torch.float16, torch.bfloat16)
MAX_DIM, MAX_FRAMES = 16384, 65535


def last_kernel() -> str:
    """Name of the device kernel the last ingest call of this process launched (tests / bench introspection)."""
    return _lib.lib().mvdetr_ingest_last_kernel().decode()


class _MatUpload:
    """Host matrices -> device without making the host wait for the GPU: a ring of pinned staging buffers, as model.py's
    _ProjUpload (the host only ever waits for the upload issued RING calls ago)."""
    RING = 3

    def __init__(self):
        self.bufs, self.events, self.next = [], [], 0

    def upload(self, mats, dev):
        if not self.bufs or self.bufs[0].shape != mats.shape:
            self.bufs = [torch.empty_like(mats).pin_memory() for _ in range(self.RING)]
            self.events = [None] * self.RING
            self.next = 0
        i = self.next
        self.next = (i + 1) % self.RING
        if self.events[i] is not None:
            self.events[i].synchronize()
        self.bufs[i].copy_(mats)
        out = self.bufs[i].to(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self.events[i] = ev
        return out


_uploads = {}
_uploads_lock = threading.Lock()


def _device_mats(M, dev):
    """[K, 3, 3] float64 on ``dev``; a CPU ``M`` goes through this (device, thread)'s pinned ring."""
    if M.device == dev:
        return M.to(torch.float64).contiguous()
    if M.device.type != "cpu":
        raise RuntimeError(f"ingest_frames: M lives on {M.device}, the frames on {dev}")
    key = (dev.index, threading.get_ident())
    with _uploads_lock:
        ring = _uploads.setdefault(key, _MatUpload())
    return ring.upload(M.to(torch.float64).contiguous(), dev)


def _dense_strides(shape, channels_last):
    k, c, h, w = shape
    return (h * w * c, 1, w * c, c) if channels_last else (c * h * w, h * w, w, 1)


def ingest_frames(frames, M=None, out_hw=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, border=128, dtype=torch.float32,
                  channels_last=True, out=None):
    """``frames`` uint8 [K, Hs, Ws, 3] or [B, N, Hs, Ws, 3] -> [K, 3, Ho, Wo] (or [B, N, 3, Ho, Wo]) of ``dtype``:

        out[k, c] = resize(((A[k, c] / 255) - mean[c]) / std[c])          (Ho, Wo) = ``out_hw``

    ``resize`` is ``F.interpolate(mode="bilinear", align_corners=False, antialias=False)``; ``A`` is the frame, or with
    ``M`` ([K, 3, 3] / [B, N, 3, 3], CPU or device, destination pixel <- source pixel, ``cv2.warpPerspective``'s convention:
    the matrix ``MVDeTr.forward`` takes) the frame warped by it at its own size, bilinear, outside pixels = ``border`` (a grey
    level; the reference's 128) -- kept in float, not rounded back to uint8.  ``M=None`` runs a kernel without warp code.

    Rows and frames of ``frames`` may be strided (a cropped view is read in place); the three bytes of a pixel and the pixels of
    a row must be dense, anything else is copied first.  The result is ``torch.channels_last`` per image by default (NCHW with
    ``channels_last=False``); ``out``, if given, must already have that shape, dtype and memory layout.  CUDA frames:
    float32, float16 or bfloat16, nothing waits for the GPU.  CPU frames: float32 or float64 on the library's host path."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
        raise TypeError(f"ingest_frames: frames must be a uint8 tensor, got {getattr(frames, 'dtype', type(frames))}")
    if frames.dim() not in (4, 5) or frames.shape[-1] != 3:
        raise ValueError(f"ingest_frames: frames must be [K, Hs, Ws, 3] or [B, N, Hs, Ws, 3], got {tuple(frames.shape)}")
    if out_hw is None:
        raise ValueError("ingest_frames: out_hw=(Ho, Wo) is required")
    lead = tuple(frames.shape[:-3])
    K, (Hs, Ws), (Ho, Wo) = int(torch.Size(lead).numel()), frames.shape[-3:-1], (int(out_hw[0]), int(out_hw[1]))
    if min(Hs, Ws, Ho, Wo) < 1 or max(Hs, Ws, Ho, Wo) > MAX_DIM or K > MAX_FRAMES:
        raise ValueError(f"ingest_frames: sizes must lie in [1, {MAX_DIM}] and at most {MAX_FRAMES} frames, got "
                         f"{K} x ({Hs}, {Ws}) -> ({Ho}, {Wo})")
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("ingest_frames: mean and std have three entries")
    dev = frames.device
    if dev.type == "cuda":
        if dtype not in (torch.float32,) + HALF_DTYPES:
            raise RuntimeError(f"ingest_frames: float32, float16 or bfloat16 on the GPU, got {dtype}")
    elif dtype in HALF_DTYPES:
        raise RuntimeError("ingest_frames: float16 / bfloat16 are implemented on the GPU only (CPU frames: float32 or float64)")
    elif dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"ingest_frames: float32 or float64 on the CPU, got {dtype}")
    if M is not None:
        if M.shape[-2:] != (3, 3) or tuple(M.shape[:-2]) not in (lead, (K,)):
            raise ValueError(f"ingest_frames: M must hold one 3x3 matrix per frame ({lead + (3, 3)}), got {tuple(M.shape)}")
        M = M.detach().reshape(K, 3, 3)
        M = _device_mats(M, dev) if dev.type == "cuda" else M.to(device=dev, dtype=torch.float64).contiguous()

    f = frames
    if f.dim() == 5 and f.shape[0] > 1 and f.shape[1] > 1 and f.stride(0) != f.shape[1] * f.stride(1):
        f = f.contiguous()
    if f.stride(-1) != 1 or f.stride(-2) != 3 or (Hs > 1 and f.stride(-3) < Ws * 3):
        f = f.contiguous()
    row_stride = f.stride(-3) if Hs > 1 else Ws * 3
    if f.dim() == 5:
        frame_stride = f.stride(1) if f.shape[1] > 1 else f.stride(0)
    else:
        frame_stride = f.stride(0)
    if K <= 1:
        frame_stride = 0

    shape = (K, 3, Ho, Wo)
    if out is None:
        res = torch.empty(shape, dtype=dtype, device=dev, memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    else:
        if out.dtype != dtype or out.device != dev or tuple(out.shape) not in (shape, lead + (3, Ho, Wo)):
            raise ValueError(f"ingest_frames: out must be {dtype} {shape} on {dev}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        res = out.view(shape)
        want = _dense_strides(shape, channels_last)
        if any(n > 1 and s != w for n, s, w in zip(shape, res.stride(), want)):
            raise ValueError(f"ingest_frames: out must be dense in {'channels_last' if channels_last else 'NCHW'} memory")
    a = [1.0 / (255.0 * float(s)) for s in std]
    b = [-float(m) / float(s) for m, s in zip(mean, std)]
    mats = M.data_ptr() if M is not None else None
    if K > 0:
        if dev.type == "cuda":
            with torch.cuda.device(dev):
                rc = getattr(_lib.lib(), f"mvdetr_ingest_frames_{_lib.suffix(dtype, half_ok=True)}")(
                    _lib.current_stream_ptr(dev), f.data_ptr(), frame_stride, row_stride, mats, *a, *b, K, Hs, Ws, Ho, Wo,
                    1 if channels_last else 0, float(border), res.data_ptr())
        else:
            rc = getattr(_lib.lib(), f"mvdetr_ingest_frames_host_{_lib.suffix(dtype)}")(
                f.data_ptr(), frame_stride, row_stride, mats, *a, *b, K, Hs, Ws, Ho, Wo, 1 if channels_last else 0, float(border),
                res.data_ptr())
        _lib.check(rc, "ingest_frames")
    if out is not None:
        return out
    return res.view(lead + (3, Ho, Wo)) if len(lead) == 2 else res
