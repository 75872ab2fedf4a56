"""norm(x + residual) in one HIP kernel (inference), for the tails of the shadow transformer's encoder layer
(multiview_detector/models/deformable_transformer.py:96-100).  Training keeps torch's differentiable ops."""
from __future__ import annotations

import torch

from .. import _lib

SUPPORTED_COLS = (64, 128, 256)
FUSED_DTYPES = (torch.float32, torch.float16, torch.bfloat16)    # 16-bit: storage only, the arithmetic is fp32


def fused_add_layer_norm_available(x: torch.Tensor, norm: torch.nn.LayerNorm) -> bool:
    """True when add_layer_norm() can run the HIP kernel for this input and module: CUDA fp32, fp16 or bf16 (the norm's
    parameters in the same dtype and on the same device), LayerNorm over a last dimension of 64/128/256 channels, and
    nothing that needs autograd.  (The call's other tensors: _kernel_operands.)"""
    if not (_device_of(x) is not None and x.dtype in FUSED_DTYPES and len(norm.normalized_shape) == 1
            and norm.normalized_shape[0] == x.shape[-1] and x.shape[-1] in SUPPORTED_COLS):
        return False
    if torch.is_grad_enabled() and (x.requires_grad or (norm.weight is not None and norm.weight.requires_grad)):
        return False
    if norm.weight is not None and (norm.bias is None or norm.weight.dtype != x.dtype or norm.bias.dtype != x.dtype):
        return False
    if any(p is not None and _device_of(p) != _device_of(x) for p in (norm.weight, norm.bias)):
        return False                                      # (a host pointer never reaches the kernel: torch's ops raise)
    return (norm.weight is None) == (norm.bias is None)


def last_kernel() -> str:
    """Name of the kernel the last fused add + LayerNorm call of this process launched ("none" before the first)."""
    return _lib.lib().mvdetr_add_layernorm_last_kernel().decode()


def _device_of(t):
    """The device a tensor's pointer belongs to, None for a tensor that is not on a GPU (tests replace this probe)."""
    return t.device if t.is_cuda else None


def _kernel_operands(x, residual, norm, then_add):
    """The whole decision of add_layer_norm: the contiguous ``(x, residual, weight, bias, then_add)`` the HIP kernel reads, or
    None when the module's own torch ops take the call (they raise or promote as they always do): the arguments fail
    fused_add_layer_norm_available(), some tensor of the call is on another device than ``x`` or of another dtype (a
    residual is never cast, a host pointer never reaches the kernel), a shape does not fit, or a pointer is below the
    alignment of one lane's access."""
    if not fused_add_layer_norm_available(x, norm):
        return None
    dev = _device_of(x)
    if residual is not None and not (residual.shape == x.shape and residual.dtype == x.dtype and _device_of(residual) == dev):
        return None
    if then_add is not None and not (_device_of(then_add) == dev and then_add.dtype == x.dtype
                                     and then_add.dim() == x.dim() == 3 and then_add.shape[1:] == x.shape[1:]
                                     and then_add.shape[0] in (1, x.shape[0])):
        return None
    ops = (x.contiguous(), None if residual is None else residual.contiguous(),
           None if norm.weight is None else norm.weight.detach().contiguous(),
           None if norm.bias is None else norm.bias.detach().contiguous(),
           None if then_add is None else then_add.contiguous())
    # a lane reads its cols / 64 consecutive elements as one access: the C entry refuses (hipErrorNotSupported) pointers
    # below that alignment -- a view at an odd storage offset -- and torch's ops take the call instead
    al = x.shape[-1] // 64 * x.element_size()
    if any(t is not None and t.data_ptr() % al != 0 for t in ops):
        return None
    return ops


def add_layer_norm(x: torch.Tensor, residual: torch.Tensor, norm: torch.nn.LayerNorm, then_add: torch.Tensor = None):
    """``norm(x + residual)`` (residual may be None).  One pass over the rows on the GPU when
    fused_add_layer_norm_available() and every tensor of the call shares x's device and dtype; the module's own torch
    ops otherwise (training / other shapes / mixed devices or dtypes, which raise or promote there).
    With ``then_add`` ([1 or B, n, C], e.g. the position embedding) returns ``(y, y + then_add)`` -- the second
    output comes out of the same pass."""
    ops = _kernel_operands(x, residual, norm, then_add)
    if ops is None:
        y = norm(x if residual is None else x + residual)
        return y if then_add is None else (y, y + then_add)
    xc, rc, w, b, a2 = ops
    cols = xc.shape[-1]
    out = torch.empty_like(xc)
    rows = xc.numel() // cols
    out2 = None if then_add is None else torch.empty_like(xc)
    with torch.cuda.device(x.device):
        code = getattr(_lib.lib(), f"mvdetr_add_layernorm_add_{_lib.suffix(x.dtype, half_ok=True)}")(
            _lib.current_stream_ptr(x.device), xc.data_ptr(), 0 if rc is None else rc.data_ptr(),
            0 if w is None else w.data_ptr(), 0 if b is None else b.data_ptr(),
            0 if a2 is None else a2.data_ptr(), 0 if a2 is None else a2.numel() // cols, rows, cols, float(norm.eps),
            out.data_ptr(), 0 if out2 is None else out2.data_ptr())
    _lib.check(code, "add_layer_norm")
    return out if then_add is None else (out, out2)
