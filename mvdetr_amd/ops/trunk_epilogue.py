"""The ResNet trunk's inference epilogues in one HIP pass each (csrc/trunk_epilogue.hip): eval-mode BatchNorm2d fused
with the ReLU / residual add / downsample BatchNorm that follows it in a residual block, and the stem's
BatchNorm + ReLU + MaxPool2d(3, 2, 1).  Channel-last fp32 CUDA tensors (bn_act, bn_relu_maxpool) or channel-last
float16 / bfloat16 ones with the BatchNorm's vectors in fp32, as MVDeTr.to_inference leaves them (bn_act_half,
bn_relu_maxpool_half: fp32 arithmetic on 16-bit storage, one rounding on the way out); everything else -- training,
autograd, other dtypes and layouts, the CPU -- runs the modules' own torch ops (the callers in model.py ask the
predicates first)."""
from __future__ import annotations

import os

import torch
from torch import nn

from .. import _lib

_enabled = os.environ.get("MVDETR_TRUNK_FUSION", "1") != "0"


def set_trunk_fusion(on: bool) -> bool:
    """Switch the fused passes on or off for this process (default on; ``MVDETR_TRUNK_FUSION=0`` starts with them off).
    Returns the previous setting.  Off: the trunk runs torch's ops, exactly as without this module."""
    global _enabled
    prev, _enabled = _enabled, bool(on)
    return prev


def trunk_fusion_enabled() -> bool:
    return _enabled


def last_kernel() -> str:
    """Name of the kernel the last fused call of this process launched ("none" before the first)."""
    return _lib.lib().mvdetr_trunk_last_kernel().decode()


def launch_count() -> int:
    """Number of fused launches of this process so far."""
    return int(_lib.lib().mvdetr_trunk_launch_count())


HALF_DTYPES = (torch.float16, torch.bfloat16)


def _on_device(t) -> bool:
    return t.is_cuda


def _activation_ok(x, dtypes=(torch.float32,), vec=4) -> bool:
    # channel-last memory, dense: the kernels index it as [N*H*W, C]; a lane owns `vec` channels (16 bytes)
    return (isinstance(x, torch.Tensor) and _on_device(x) and x.dtype in dtypes and x.dim() == 4 and x.shape[1] % vec == 0
            and x.numel() > 0 and x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0)


def _overlap(a, b) -> bool:
    # both dense: the byte ranges say it all (x may be overwritten in place while other lanes still read the residual)
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _vector_ok(v, device) -> bool:
    return v.dtype == torch.float32 and v.device == device and v.is_contiguous() and v.data_ptr() % 16 == 0


def _bn_ok(bn, channels, device, requires_grad) -> bool:
    if not (type(bn) is nn.BatchNorm2d and not bn.training and bn.running_mean is not None and bn.running_var is not None
            and bn.num_features == channels):
        return False
    vecs = [bn.running_mean, bn.running_var] + [p for p in (bn.weight, bn.bias) if p is not None]
    if not all(_vector_ok(v, device) for v in vecs):
        return False
    # nothing that needs autograd: the kernels are forward only
    return not (torch.is_grad_enabled() and (requires_grad or any(v.requires_grad for v in vecs)))


def bn_act_conditions(shape, dtype, device, requires_grad, bn, residual=None, residual_bn=None, vec=4) -> bool:
    """The BatchNorm and residual side of fused_bn_act_available() for an activation of this shape, dtype and device
    that need not exist yet (a convolution asks before it allocates its output): BatchNorm2d modules in eval mode with
    running statistics and fp32 vectors, a residual of the same shape, dtype and channel-last layout, nothing that needs
    autograd.  The switch, the activation's own layout and its overlap with the residual are the caller's to check."""
    if not _bn_ok(bn, shape[1], device, requires_grad):
        return False
    if residual is None:
        return residual_bn is None
    if not (_activation_ok(residual, (dtype,), vec) and residual.shape == torch.Size(shape) and residual.device == device):
        return False
    if torch.is_grad_enabled() and residual.requires_grad:
        return False
    return residual_bn is None or _bn_ok(residual_bn, residual.shape[1], residual.device, residual.requires_grad)


def _bn_act_ok(x, bn, residual, residual_bn, dtypes, vec) -> bool:
    if not (_enabled and _activation_ok(x, dtypes, vec)):
        return False
    if not bn_act_conditions(x.shape, x.dtype, x.device, x.requires_grad, bn, residual, residual_bn, vec):
        return False
    return residual is None or not _overlap(residual, x)


def fused_bn_act_available(x: torch.Tensor, bn: nn.Module, residual: torch.Tensor = None, residual_bn: nn.Module = None) -> bool:
    """True when bn_act() runs the HIP kernel for these arguments: the switch is on, CUDA fp32 channel-last activations
    with C % 4 == 0, BatchNorm2d modules in eval mode with running statistics, a residual of the same shape and
    layout, and nothing that needs autograd."""
    return _bn_act_ok(x, bn, residual, residual_bn, (torch.float32,), 4)


def fused_bn_act_half_available(x: torch.Tensor, bn: nn.Module, residual: torch.Tensor = None,
                                residual_bn: nn.Module = None) -> bool:
    """True when bn_act_half() runs the 16-bit HIP kernel: as fused_bn_act_available(), but x is float16 or bfloat16,
    the residual has x's dtype, C % 8 == 0, and the BatchNorm's vectors are fp32 (a BatchNorm cast to 16 bits, as by
    ``model.half()``, is refused and keeps torch's ops)."""
    return _bn_act_ok(x, bn, residual, residual_bn, HALF_DTYPES, 8)


def _bn_args(bn):
    if bn is None:
        return 0, 0, 0, 0, 0.0
    return (bn.running_mean.data_ptr(), bn.running_var.data_ptr(), 0 if bn.weight is None else bn.weight.data_ptr(),
            0 if bn.bias is None else bn.bias.data_ptr(), float(bn.eps))


def _suffix(dtype) -> str:
    return {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}[dtype]


def _run_bn_act(x, bn, residual, residual_bn, relu, inplace):
    y = x if inplace else torch.empty_like(x)
    C = x.shape[1]
    with torch.cuda.device(x.device):
        code = getattr(_lib.lib(), "mvdetr_bn_act_" + _suffix(x.dtype))(
            _lib.current_stream_ptr(x.device), x.data_ptr(), *_bn_args(bn), 0 if residual is None else residual.data_ptr(),
            *_bn_args(residual_bn), x.numel() // C, C, int(bool(relu)), y.data_ptr())
    _lib.check(code, "bn_act")
    return y


def bn_act(x: torch.Tensor, bn: nn.BatchNorm2d, residual: torch.Tensor = None, residual_bn: nn.BatchNorm2d = None,
           relu: bool = True, inplace: bool = False) -> torch.Tensor:
    """``act(bn(x) [+ residual | + residual_bn(residual)])`` in one pass; ``inplace`` overwrites x (pass only a tensor
    the caller has just allocated, e.g. a convolution's output) and returns it.  Raises when
    fused_bn_act_available() is False: callers decide, nothing falls back silently here."""
    if not fused_bn_act_available(x, bn, residual, residual_bn):
        raise RuntimeError("bn_act: these arguments do not take the fused kernel (see fused_bn_act_available)")
    return _run_bn_act(x, bn, residual, residual_bn, relu, inplace)


def bn_act_half(x: torch.Tensor, bn: nn.BatchNorm2d, residual: torch.Tensor = None, residual_bn: nn.BatchNorm2d = None,
                relu: bool = True, inplace: bool = False) -> torch.Tensor:
    """bn_act() over float16 / bfloat16 activations with fp32 BatchNorm vectors: every step in fp32 -- the sum
    ``bn(x) + residual`` is not rounded in between, where torch's 16-bit chain rounds after each op -- and one rounding
    to nearest-even at the store.  Raises when fused_bn_act_half_available() is False."""
    if not fused_bn_act_half_available(x, bn, residual, residual_bn):
        raise RuntimeError("bn_act_half: these arguments do not take the fused kernel (see fused_bn_act_half_available)")
    return _run_bn_act(x, bn, residual, residual_bn, relu, inplace)


def _pool_ok(x, bn, relu, pool, dtypes, vec) -> bool:
    def two(v, want):
        return v == want or v == (want, want)
    if not (_enabled and _activation_ok(x, dtypes, vec) and _bn_ok(bn, x.shape[1], x.device, x.requires_grad)
            and type(relu) is nn.ReLU and type(pool) is nn.MaxPool2d):
        return False
    cg = x.shape[1] // vec
    if not (256 % cg == 0 if cg <= 256 else cg % 256 == 0):
        return False
    return (two(pool.kernel_size, 3) and two(pool.stride, 2) and two(pool.padding, 1) and two(pool.dilation, 1)
            and not pool.ceil_mode and not pool.return_indices)


def fused_bn_relu_maxpool_available(x: torch.Tensor, bn: nn.Module, relu: nn.Module, pool: nn.Module) -> bool:
    """True when bn_relu_maxpool() runs the HIP kernel: as fused_bn_act_available(), a plain ReLU, and the pool exactly
    MaxPool2d(kernel 3, stride 2, padding 1, dilation 1, ceil_mode False) without indices."""
    return _pool_ok(x, bn, relu, pool, (torch.float32,), 4)


def fused_bn_relu_maxpool_half_available(x: torch.Tensor, bn: nn.Module, relu: nn.Module, pool: nn.Module) -> bool:
    """True when bn_relu_maxpool_half() runs the 16-bit HIP kernel: as fused_bn_act_half_available() and the same ReLU
    and pool as fused_bn_relu_maxpool_available(); C / 8 must divide 256 or be a multiple of it."""
    return _pool_ok(x, bn, relu, pool, HALF_DTYPES, 8)


def _run_pool(x, bn):
    N, C, H, W = x.shape
    y = torch.empty((N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=x.dtype, device=x.device,
                    memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        code = getattr(_lib.lib(), "mvdetr_bn_relu_maxpool_" + _suffix(x.dtype))(
            _lib.current_stream_ptr(x.device), x.data_ptr(), *_bn_args(bn), N, H, W, C, y.data_ptr())
    _lib.check(code, "bn_relu_maxpool")
    return y


def bn_relu_maxpool(x: torch.Tensor, bn: nn.BatchNorm2d) -> torch.Tensor:
    """``max_pool2d(relu(bn(x)), 3, 2, 1)`` in one pass over x (channel-last in, channel-last out)."""
    if not fused_bn_relu_maxpool_available(x, bn, _RELU, _POOL):
        raise RuntimeError("bn_relu_maxpool: these arguments do not take the fused kernel (see fused_bn_relu_maxpool_available)")
    return _run_pool(x, bn)


def bn_relu_maxpool_half(x: torch.Tensor, bn: nn.BatchNorm2d) -> torch.Tensor:
    """bn_relu_maxpool() over float16 / bfloat16 activations with fp32 BatchNorm vectors: the max is taken on the fp32
    values and rounded once, which equals ``max_pool2d(bn_act_half(x, bn), 3, 2, 1)`` bit for bit (rounding is monotone)."""
    if not fused_bn_relu_maxpool_half_available(x, bn, _RELU, _POOL):
        raise RuntimeError("bn_relu_maxpool_half: these arguments do not take the fused kernel "
                           "(see fused_bn_relu_maxpool_half_available)")
    return _run_pool(x, bn)


_RELU, _POOL = nn.ReLU(), nn.MaxPool2d(3, 2, 1)
