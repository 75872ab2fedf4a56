"""deform_conv2d / DeformConv2d: torchvision.ops' deformable convolution (v1) on the library's own kernels.

The reference's ``deform_conv`` ground-plane aggregator (multiview_detector/models/conv_world_feat.py:5,55-76) takes
``torchvision.ops.DeformConv2d``, a compiled CUDA op.  These have torchvision's signatures and results:

* ``deform_conv2d(input, offset, weight, bias=None, stride=1, padding=0, dilation=1, mask=None)``
* ``DeformConv2d(in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True)``

Sampling: tap (i, j) of output pixel (h, w) reads the input bilinearly at y = h * stride - padding + i * dilation + dy
(x likewise) in pixel units, 0 outside (-1, H) x (-1, W); offset channel 2 (g * kh * kw + i * kw + j) is dy of offset group
g, the next one dx (include/mvdetr_ops.h).  CUDA tensors run the HIP kernels of csrc/deform_conv.hip; which one is the
library's decision (csrc/deform_conv_route.h): fp32 with a channel-last input (``torch.channels_last``, e.g.
``warp_perspective(..., channels_last_out=True)`` viewed as NCHW) of the MFMA shape takes the MFMA implicit GEMM, an NCHW input
of that shape is transposed to channel-last first, everything else the generic kernels.  CPU tensors run the library's host path.
Gradients flow to input, offset, weight and bias; the backward is not bit-reproducible (atomics), like torchvision's CUDA kernel.

16-bit inference (float16 / bfloat16 CUDA tensors of one dtype, forward only): a call of the 16-bit MFMA shape runs
``dc_fwd_mfma_half`` of csrc/deform_conv_half.hip -- 16-bit storage, fp32 arithmetic, one rounding on the way out -- on a
channel-last input read in place (an NCHW input is copied to channel-last first); the kernel takes the weight permuted to [kh * kw, C_out, C_in], one small copy per call that ``DeformConv2d`` caches in eval mode.
Every other 16-bit CUDA call (odd channel counts, two offset groups, a data pointer that is not 16-byte aligned) is computed
as ``deform_conv2d(x.float(), ...).to(dtype)`` on the fp32 routes above, and ``MVDETR_DEFORM_CONV_HALF=0`` (read per call)
sends the kernel's calls there too.  A 16-bit call with a tensor that requires grad while grad is enabled raises: forward only.
Not provided: the DCNv2 modulation ``mask`` and weight ``groups > 1`` (NotImplementedError), 16-bit CPU tensors (RuntimeError).
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from .. import _lib
from .warp import _transpose


def last_kernel() -> str:
    """Route of the last deformable-convolution call of this process on the device: "dc_fwd_mfma", "dc_fwd_mfma_half",
    "dc_fwd_generic", "dc_bwd_mfma" or "dc_bwd_generic" (tests / tools introspection)."""
    return _lib.lib().mvdetr_deform_conv2d_last_kernel().decode()


def _layout(x, shape):
    """(tensor whose memory the kernels read, nhwc flag): a channel-last input is read in place; an NCHW input whose channel-
    last route is the MFMA kernel is transposed by the library's tiled transpose; anything else is read as NCHW.  ``shape``:
    ``_args`` of the call, the integers the library's route table (csrc/deform_conv_route.h) is asked with."""
    B, C, H, W = x.shape
    if x.is_contiguous():
        # (about the tensor, not the route: a copy that changes something, within the tiled transpose's own grid limits)
        if (x.is_cuda and C > 1 and H * W > 1 and B <= 65535 and (H * W + 63) // 64 <= 65535
                and _lib.dc_route(_lib.ROUTE_FORWARD, x.element_size(), *shape, 1, 1) == "fwd_mfma"):
            t = _transpose(x, B, C, H * W)                                  # memory [B, H*W, C]
            return t.view(B, H, W, C).permute(0, 3, 1, 2), 1
        return x, 0
    if x.is_contiguous(memory_format=torch.channels_last):
        return x, 1
    return x.contiguous(), 0


def _args(x, weight, conf):
    (sh, sw), (ph, pw), (dh, dw), G = conf
    B, C, H, W = x.shape
    return [B, C, H, W, weight.shape[0], weight.shape[2], weight.shape[3], sh, sw, ph, pw, dh, dw, G]


class DeformConv2dFunction(Function):
    @staticmethod
    def forward(ctx, input, offset, weight, bias, stride, padding, dilation, offset_groups):
        conf = (stride, padding, dilation, offset_groups)
        shape = _args(input, weight, conf)
        x, nhwc = _layout(input, shape)
        offset, weight = offset.contiguous(), weight.contiguous()
        bias = None if bias is None else bias.contiguous()
        B, Co = x.shape[0], weight.shape[0]
        out = torch.empty((B, Co, offset.shape[2], offset.shape[3]), dtype=x.dtype, device=x.device)
        sfx = _lib.suffix(x.dtype)
        args = shape + [nhwc, out.data_ptr()]
        bias_ptr = None if bias is None else bias.data_ptr()
        if x.is_cuda:
            with torch.cuda.device(x.device):
                rc = getattr(_lib.lib(), f"mvdetr_deform_conv2d_forward_{sfx}")(
                    _lib.current_stream_ptr(x.device), x.data_ptr(), offset.data_ptr(), weight.data_ptr(), bias_ptr, *args)
        else:
            rc = getattr(_lib.lib(), f"mvdetr_deform_conv2d_forward_host_{sfx}")(
                x.data_ptr(), offset.data_ptr(), weight.data_ptr(), bias_ptr, *args)
        _lib.check(rc, "deform_conv2d_forward")
        ctx.save_for_backward(x, offset, weight)
        ctx.conf, ctx.nhwc, ctx.has_bias = conf, nhwc, bias is not None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, offset, weight = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        # grad_input in the layout the kernels read (channel-last memory for a channel-last or transposed input)
        grad_input = torch.zeros_like(x, memory_format=torch.channels_last if ctx.nhwc else torch.contiguous_format)
        grad_offset = torch.empty_like(offset)
        grad_weight = torch.empty_like(weight)
        sfx = _lib.suffix(x.dtype)
        args = _args(x, weight, ctx.conf) + [ctx.nhwc, grad_input.data_ptr(), grad_offset.data_ptr(), grad_weight.data_ptr()]
        if x.is_cuda:
            with torch.cuda.device(x.device):
                rc = getattr(_lib.lib(), f"mvdetr_deform_conv2d_backward_{sfx}")(
                    _lib.current_stream_ptr(x.device), grad_out.data_ptr(), x.data_ptr(), offset.data_ptr(),
                    weight.data_ptr(), *args)
        else:
            rc = getattr(_lib.lib(), f"mvdetr_deform_conv2d_backward_host_{sfx}")(
                grad_out.data_ptr(), x.data_ptr(), offset.data_ptr(), weight.data_ptr(), *args)
        _lib.check(rc, "deform_conv2d_backward")
        grad_bias = grad_out.sum((0, 2, 3)) if ctx.has_bias else None
        return grad_input, grad_offset, grad_weight, grad_bias, None, None, None, None


_HALF = (torch.float16, torch.bfloat16)


def permute_weight(weight):
    """[C_out, C_in, kh, kw] -> the 16-bit kernel's [kh * kw, C_out, C_in] copy (a weight-tile row is one contiguous run)."""
    Co, C, kh, kw = weight.shape
    return weight.detach().permute(2, 3, 0, 1).reshape(kh * kw, Co, C).contiguous()


def half_kernel_serves(input, weight, offset_groups, stride=(1, 1), padding=(0, 0), dilation=(1, 1), shape=None):
    """True when a 16-bit CUDA call of these shapes and convolution parameters goes to the 16-bit entry (given an aligned or
    copied input): to dc_fwd_mfma_half, or to its refusal of a shape no entry takes (the exception is then the entry's, as it
    always was).  ``shape``: ``_args`` of the call where the caller has them."""
    shape = shape or _args(input, weight, (stride, padding, dilation, offset_groups))
    return (input.is_cuda and input.dtype in _HALF and os.environ.get("MVDETR_DEFORM_CONV_HALF", "1") != "0"
            and _lib.dc_route(_lib.ROUTE_FORWARD_HALF, 2, *shape, 1, 1) in ("fwd_mfma_half", "invalid_value"))


def _forward_half(input, offset, weight, bias, conf, relu=False, out=None, weight_t=None):
    """The 16-bit CUDA forward: dc_fwd_mfma_half where it serves the call, else the fp32 routes on upcast tensors.  ``relu``
    applies max(., 0) (in the kernel's store); ``out`` [B, C_out, H_out, W_out] may be a channel slice of a larger tensor."""
    stride, padding, dilation, G = conf
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (input, offset, weight, bias)):
        raise RuntimeError("deform_conv2d: float16 / bfloat16 calls are forward-only (inference): a tensor requires grad; "
                           "call under torch.no_grad() or use float32")
    B, Co, (Ho, Wo) = input.shape[0], weight.shape[0], offset.shape[2:]
    shape = _args(input, weight, conf)
    x, ok = input, half_kernel_serves(input, weight, G, shape=shape)
    if ok:
        if not x.is_contiguous(memory_format=torch.channels_last):
            x = x.contiguous(memory_format=torch.channels_last)
        ok = x.data_ptr() % 16 == 0
    if ok and out is not None:
        ok = (out.dtype == x.dtype and out.device == x.device and tuple(out.shape) == (B, Co, Ho, Wo)
              and out.stride()[1:] == (Ho * Wo, Wo, 1) and (B == 1 or out.stride(0) >= Co * Ho * Wo))
    if not ok:
        res = deform_conv2d(input.float(), offset.float(), weight.float(), None if bias is None else bias.float(),
                            stride, padding, dilation).to(input.dtype)
        res = F.relu(res) if relu else res
        return res if out is None else out.copy_(res)
    offset = offset.contiguous()
    if weight_t is None:
        weight_t = permute_weight(weight)
    bias = None if bias is None else bias.detach().contiguous()
    if out is None:
        out = torch.empty((B, Co, Ho, Wo), dtype=x.dtype, device=x.device)
    out_batch_stride = out.stride(0) if B > 1 else Co * Ho * Wo
    args = shape + [1, int(bool(relu)), out_batch_stride, out.data_ptr()]
    with torch.cuda.device(x.device):
        rc = getattr(_lib.lib(), f"mvdetr_deform_conv2d_forward_{_lib.suffix(x.dtype, half_ok=True)}")(
            _lib.current_stream_ptr(x.device), x.data_ptr(), offset.data_ptr(), weight_t.data_ptr(),
            None if bias is None else bias.data_ptr(), *args)
    _lib.check(rc, "deform_conv2d_forward (16-bit)")
    return out


def deform_conv2d(input, offset, weight, bias=None, stride=1, padding=0, dilation=1, mask=None):
    """torchvision.ops.deform_conv2d (v1): input [B, C_in, H, W], offset [B, 2 * G * kh * kw, H_out, W_out], weight
    [C_out, C_in, kh, kw], bias [C_out] or None -> [B, C_out, H_out, W_out]."""
    return _deform_conv2d(input, offset, weight, bias, stride, padding, dilation, mask)


def _deform_conv2d(input, offset, weight, bias, stride, padding, dilation, mask, relu=False, out=None, weight_t=None):
    """deform_conv2d; ``relu`` / ``out`` / ``weight_t`` are DeformConv2d's way into the 16-bit kernel's fused store and cached
    permuted weight (16-bit CUDA calls only)."""
    if mask is not None:
        raise NotImplementedError("deform_conv2d: the DCNv2 modulation mask is not implemented")
    if input.dim() != 4 or offset.dim() != 4 or weight.dim() != 4:
        raise ValueError(f"deform_conv2d: expected 4-D input, offset and weight, got {tuple(input.shape)}, "
                         f"{tuple(offset.shape)} and {tuple(weight.shape)}")
    devices = {t.device for t in (input, offset, weight, bias) if t is not None}
    if len(devices) != 1:
        raise RuntimeError(f"deform_conv2d: all tensors must be on one device, got {sorted(map(str, devices))}")
    dtypes = {t.dtype for t in (input, offset, weight, bias) if t is not None}
    if len(dtypes) != 1:
        raise RuntimeError(f"deform_conv2d: all tensors must have one dtype, got {sorted(map(str, dtypes))}")
    half = input.is_cuda and input.dtype in _HALF
    if not half:
        _lib.suffix(input.dtype)                                   # 16-bit CPU tensors raise here
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    B, C, H, W = input.shape
    Co, Cw, kh, kw = weight.shape
    if Cw != C:
        if Cw > 0 and C % Cw == 0:
            raise NotImplementedError("deform_conv2d: weight groups > 1 are not implemented")
        raise ValueError(f"deform_conv2d: weight {tuple(weight.shape)} does not fit {C} input channels")
    if min(stride) < 1 or min(dilation) < 1 or min(padding) < 0:
        raise ValueError(f"deform_conv2d: stride {stride} and dilation {dilation} must be >= 1, padding {padding} >= 0")
    if bias is not None and tuple(bias.shape) != (Co,):
        raise ValueError(f"deform_conv2d: bias {tuple(bias.shape)} does not fit {Co} output channels")
    if offset.shape[1] % (2 * kh * kw) != 0 or offset.shape[1] == 0:
        raise RuntimeError(f"the shape of the offset tensor at dimension 1 is not valid. It should be a multiple of "
                           f"2 * weight.size[2] * weight.size[3].\nGot offset.shape[1]={offset.shape[1]}, while "
                           f"2 * weight.size[2] * weight.size[3]={2 * kh * kw}")
    G = offset.shape[1] // (2 * kh * kw)
    if C % G != 0:
        raise RuntimeError(f"deform_conv2d: {C} input channels are not a multiple of the {G} offset groups")
    if offset.shape[0] != B:
        raise RuntimeError(f"invalid batch size of offset: {offset.shape[0]} for input batch {B}")
    Ho = (H + 2 * padding[0] - dilation[0] * (kh - 1) - 1) // stride[0] + 1
    Wo = (W + 2 * padding[1] - dilation[1] * (kw - 1) - 1) // stride[1] + 1
    if Ho < 1 or Wo < 1:
        raise RuntimeError(f"deform_conv2d: calculated output size {Ho}x{Wo} is too small")
    if tuple(offset.shape[2:]) != (Ho, Wo):
        raise RuntimeError(f"offset output dims: ({offset.shape[2]}, {offset.shape[3]}) - computed output dims: ({Ho}, {Wo})")
    if half:
        return _forward_half(input, offset, weight, bias, (stride, padding, dilation, G), relu=relu, out=out,
                             weight_t=weight_t)
    return DeformConv2dFunction.apply(input, offset, weight, bias, stride, padding, dilation, G)


class DeformConv2d(nn.Module):
    """torchvision.ops.DeformConv2d: ``forward(input, offset, mask=None)``; parameters ``weight`` [C_out, C_in, kh, kw] and
    ``bias`` [C_out], initialised as torchvision does (kaiming-uniform with a = sqrt(5), bias uniform in +-1/sqrt(fan_in))."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True):
        super().__init__()
        if in_channels % groups != 0:
            raise ValueError("in_channels must be divisible by groups")
        if out_channels % groups != 0:
            raise ValueError("out_channels must be divisible by groups")
        if groups != 1:
            raise NotImplementedError("DeformConv2d: weight groups > 1 are not implemented")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride = _pair(kernel_size), _pair(stride)
        self.padding, self.dilation = _pair(padding), _pair(dilation)
        self.groups = groups
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *self.kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self._half_weight_cache = None                          # (key, permuted 16-bit weight): _half_weight
        self.reset_parameters()

    def reset_parameters(self) -> None:
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in, _ = nn.init._calculate_fan_in_and_fan_out(self.weight)
            bound = 1 / math.sqrt(fan_in)
            nn.init.uniform_(self.bias, -bound, bound)

    def _half_weight(self, input):
        """The kernel's permuted copy of the weight for a 16-bit CUDA call in eval mode, cached until the weight is
        replaced, written in place or cast (the key: its data_ptr, _version and dtype); None otherwise."""
        w = self.weight
        if self.training or not (input.is_cuda and input.dtype in _HALF and w.dtype == input.dtype and w.is_cuda):
            return None
        key = (w.data_ptr(), w._version, w.dtype)
        if self._half_weight_cache is None or self._half_weight_cache[0] != key:
            self._half_weight_cache = (key, permute_weight(w))
        return self._half_weight_cache[1]

    def forward(self, input, offset, mask=None):
        return _deform_conv2d(input, offset, self.weight, self.bias, self.stride, self.padding, self.dilation, mask,
                              weight_t=self._half_weight(input))

    def forward_relu_into(self, input, offset, out):
        """16-bit CUDA inference only: ``out.copy_(relu(self(input, offset)))`` where ``out`` may be a channel slice of a
        larger [B, N * C_out, H_out, W_out] tensor; dc_fwd_mfma_half applies the ReLU in its store and writes the slice in
        place.  The same bits as the composition."""
        if not (input.is_cuda and input.dtype in _HALF):
            raise RuntimeError("DeformConv2d.forward_relu_into serves float16 / bfloat16 CUDA tensors only")
        return _deform_conv2d(input, offset, self.weight, self.bias, self.stride, self.padding, self.dilation, None,
                              relu=True, out=out, weight_t=self._half_weight(input))

    def extra_repr(self) -> str:
        s = f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}"
        s += f", padding={self.padding}" if self.padding != (0, 0) else ""
        s += f", dilation={self.dilation}" if self.dilation != (1, 1) else ""
        s += f", groups={self.groups}" if self.groups != 1 else ""
        s += ", bias=False" if self.bias is None else ""
        return s
