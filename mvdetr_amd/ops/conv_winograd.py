"""The trunk's wide 3x3 convolutions as an fp32 Winograd F(2x2, 3x3) MFMA kernel (csrc/conv_winograd.hip): 2.25x fewer
multiplications than the direct form, fp32 inputs, products and sums throughout.  Inference only, channel-last fp32 CUDA
activations, stride 1, padding = dilation in {1, 2, 4}, no bias, and only the (C, K, dilation) families that measured
faster than MIOpen's pick; everything else keeps torch's convolution: the callers in model.py ask the
predicate first.

The block's inference epilogue -- BatchNorm, the residual (as it is or through the downsample BatchNorm) and ReLU -- can be
applied in the kernel's output store (winograd_conv3x3_bn_act): bn_act's arithmetic on the value a lane is about to store,
so the bits of winograd_conv3x3 followed by bn_act in place, without that pass over the output.

The transformed weights U = G g G^T (fp64, rounded once) are built once per weight tensor and cached."""
from __future__ import annotations

import os
import weakref

import torch
from torch import nn

from .. import _lib
from . import trunk_epilogue

_enabled = os.environ.get("MVDETR_TRUNK_WINOGRAD", "1") != "0"
_epilogue = os.environ.get("MVDETR_WINOGRAD_EPILOGUE", "1") != "0"

# F(2x2, 3x3):  Y = A^T [ (G g G^T) .* (B^T d B) ] A.  The kernels hard-code these (winograd_weights_f32 forms G g G^T,
# the convolution's loader B^T d B and its epilogue A^T M A); tests/test_conv_winograd.py pins them against a direct form.
G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))
BT = ((1.0, 0.0, -1.0, 0.0), (0.0, 1.0, 1.0, 0.0), (0.0, -1.0, 1.0, 0.0), (0.0, 1.0, 0.0, -1.0))
AT = ((1.0, 1.0, 1.0, 0.0), (0.0, 1.0, -1.0, -1.0))

# (C, K) -> dilations switched on: the shapes on which the kernel beat MIOpen's pick in every repetition of
# tools/conv_bench.py at the trunk's size (profiles/trunk_winograd_shapes.txt)
FAMILIES: dict = {(128, 256): (1,), (256, 256): (1, 2), (256, 512): (2,), (512, 512): (1, 4)}
DILATIONS = (1, 2, 4)

# Below this many output pixels (N * H * W) torch's convolution stays: 8,192 pixels = 32 blocks of 64 tiles x 8 blocks of
# 64 channels = one workgroup per CU at K = 512.
MIN_PIXELS = 8192
_min_pixels = MIN_PIXELS

# The layer1/2 families: the same rule (the kernel with the block's epilogue in its store against MIOpen + bn_act, every
# repetition: profiles/conv_winograd_families_shapes.txt), a table and a floor of their own.  With 1 or 2 blocks of 64
# channels, one workgroup per CU is 512 / K times as many pixels as above: 65,536 at K = 64, 32,768 at K = 128.  The
# floor above does not move this one (the models of the existing tests keep torch's layer1/2 convolutions at floor 0);
# set_winograd_narrow_min_pixels() does.  A (C, K, dilation) that is in FAMILIES has FAMILIES' floor.
NARROW_FAMILIES: dict = {(64, 64): (1,), (128, 128): (1,)}
_narrow_min_pixels = MIN_PIXELS


def min_pixels(C: int, K: int, dilation: int):
    """The pixel floor of (C, K, dilation) under the current settings; None for a shape outside both tables."""
    if dilation in FAMILIES.get((C, K), ()):
        return _min_pixels
    if dilation in NARROW_FAMILIES.get((C, K), ()):
        return _narrow_min_pixels * 512 // K
    return None


def set_trunk_winograd(on: bool) -> bool:
    """Switch the Winograd convolutions on or off for this process (default on; ``MVDETR_TRUNK_WINOGRAD=0`` starts with
    them off).  Returns the previous setting.  Independent of ``set_trunk_fusion``."""
    global _enabled
    prev, _enabled = _enabled, bool(on)
    return prev


def trunk_winograd_enabled() -> bool:
    return _enabled


def set_winograd_epilogue(on: bool) -> bool:
    """Switch the epilogue in the convolution's store on or off for this process (default on; ``MVDETR_WINOGRAD_EPILOGUE=0``
    starts with it off).  Returns the previous setting.  Off: the convolution stores its plain output and the epilogue is
    the pass of its own (ops/trunk_epilogue.py), bit for bit the same result."""
    global _epilogue
    prev, _epilogue = _epilogue, bool(on)
    return prev


def winograd_epilogue_enabled() -> bool:
    return _epilogue


def set_winograd_min_pixels(pixels: int) -> int:
    """The pixel floor of winograd_conv3x3_available() for FAMILIES (MIN_PIXELS by default); returns the previous one.  For
    tests, which run the model on small images."""
    global _min_pixels
    prev, _min_pixels = _min_pixels, int(pixels)
    return prev


def set_winograd_narrow_min_pixels(pixels: int) -> int:
    """The same for NARROW_FAMILIES, whose floor is ``pixels * 512 / K`` (MIN_PIXELS by default: 65,536 at K = 64, 32,768 at
    K = 128; 0: none); returns the previous setting."""
    global _narrow_min_pixels
    prev, _narrow_min_pixels = _narrow_min_pixels, int(pixels)
    return prev


def last_kernel() -> str:
    """Name of the kernel the last Winograd call of this process launched ("none" before the first)."""
    return _lib.lib().mvdetr_winograd_last_kernel().decode()


def last_epilogue() -> str:
    """What the last Winograd convolution's store applied: "none", "bn", "bn_add" or "bn_bn_add", with "_relu" appended
    under ReLU (trunk_epilogue.last_kernel's names)."""
    return _lib.lib().mvdetr_winograd_last_epilogue().decode()


def launch_count() -> int:
    """Number of Winograd launches (weight transforms included) of this process so far."""
    return int(_lib.lib().mvdetr_winograd_launch_count())


def set_winograd_max_workgroups(n: int) -> int:
    """Cap the convolution's persistent grid at ``n`` workgroups for this process (0: the default, one per CU); returns
    the previous cap.  For tests, so that small shapes run many units per workgroup; results do not depend on it."""
    return int(_lib.lib().mvdetr_winograd_set_max_workgroups(int(n)))


# (C, K, dilation) whose last round runs as half units under the default tail mode: the C library's table (tail_family in
# csrc/conv_winograd.hip; tests/test_conv_winograd_plan.py holds the two together), by the family rule on
# tools/conv_bench.py --tail (profiles/conv_winograd_w16_shapes.txt)
TAIL_FAMILIES = ((64, 64, 1), (128, 128, 1), (128, 256, 1), (256, 256, 1), (256, 256, 2), (512, 512, 1))


def set_winograd_tail(mode: int) -> int:
    """How a convolution's last, partly empty round runs: 0 as whole units in the persistent kernel; 1 (the default) as
    half units in a second launch where at most half the workgroups would be busy, on the shapes that measured faster
    that way; 2 as half units whenever there is a remainder (tests).  Returns the previous mode; the bits of the result
    do not depend on it."""
    return int(_lib.lib().mvdetr_winograd_set_tail(int(mode)))


def set_winograd_variant(variant: int) -> int:
    """Which persistent kernel runs a convolution's whole units: 0 (the default) the one the C library's table names for the
    (C, K, dilation); 1 conv3x3_winograd_f32 (4 waves, 32-channel wave blocks); 2 conv3x3_winograd_w16x2_f32 (8 waves,
    16-channel wave blocks, two waves per SIMD).  Returns the previous setting; the bits of the result do not depend on it."""
    return int(_lib.lib().mvdetr_winograd_set_variant(int(variant)))


def last_variant() -> int:
    """The persistent kernel of the last Winograd convolution: 1 or 2 (0 before the first)."""
    return int(_lib.lib().mvdetr_winograd_last_variant())


def last_tail_units() -> int:
    """The units the last Winograd convolution ran as half units (0: it had no second launch)."""
    return int(_lib.lib().mvdetr_winograd_last_tail_units())


def plan(N: int, H: int, W: int, C: int, K: int, dilation: int, workgroups: int) -> dict:
    """How a convolution call on ``workgroups`` CUs is split, under the current cap and tail mode, without a device:
    units, G (the persistent grid), R = units // G, rem = units % G, the half units of the second launch and the variant."""
    import ctypes
    out = (ctypes.c_int64 * 6)()
    _lib.check(_lib.lib().mvdetr_winograd_plan(N, H, W, C, K, dilation, workgroups, ctypes.cast(out, ctypes.c_void_p)),
               "winograd_plan")
    return dict(zip(("units", "G", "R", "rem", "half_units", "variant"), (int(v) for v in out)))


def _on_device(t) -> bool:
    return t.is_cuda


def _two(v, want) -> bool:
    return v == want or tuple(v) == (want, want)


def _structure_ok(x, conv) -> bool:
    """What the kernel itself needs, whatever the switches say."""
    if not (isinstance(x, torch.Tensor) and x.dim() == 4 and x.dtype == torch.float32 and _on_device(x) and x.numel() > 0
            and x.is_contiguous(memory_format=torch.channels_last) and x.data_ptr() % 16 == 0):
        return False
    if type(conv) is not nn.Conv2d:
        return False
    d = conv.dilation[0]
    if not (_two(conv.kernel_size, 3) and _two(conv.stride, 1) and conv.groups == 1 and conv.bias is None
            and conv.padding_mode == "zeros" and d in DILATIONS and _two(conv.dilation, d)
            and not isinstance(conv.padding, str) and _two(conv.padding, d)):
        return False
    w = conv.weight
    C, K = conv.in_channels, conv.out_channels
    if not (w.dtype == torch.float32 and w.device == x.device and x.shape[1] == C and C % 8 == 0 and K % 64 == 0):
        return False
    if (256 + 2 * x.shape[2] * x.shape[3]) * max(C, K) >= 1 << 30:
        return False
    # nothing that needs autograd: the kernel is forward only
    return not (torch.is_grad_enabled() and (x.requires_grad or w.requires_grad))


def winograd_conv3x3_available(x: torch.Tensor, conv: nn.Module) -> bool:
    """True when the model runs ``conv`` on ``x`` through the Winograd kernel: the switch is on, CUDA fp32 dense
    channel-last x, a plain nn.Conv2d with a 3x3 kernel, stride 1, groups 1, padding == dilation in {1, 2, 4}, no bias,
    zero padding, (C, K, dilation) in a family that measured faster than MIOpen (FAMILIES or NARROW_FAMILIES), nothing that
    needs autograd, ``torch.backends.cudnn.deterministic`` off (a caller who asked for the library's deterministic solvers
    keeps torch's convolution) and at least the family's pixel floor of output pixels (min_pixels())."""
    if not (_enabled and _structure_ok(x, conv)) or torch.backends.cudnn.deterministic:
        return False
    floor = min_pixels(conv.in_channels, conv.out_channels, conv.dilation[0])
    return floor is not None and x.shape[0] * x.shape[2] * x.shape[3] >= floor


class _Entry:
    __slots__ = ("ref", "alias", "version", "U")


_cache: dict = {}


def _transformed_weights(weight: torch.Tensor) -> torch.Tensor:
    """U [16, C, K] of this weight tensor, built on first use and again whenever the tensor was written in place
    (``_version``: ``weight.copy_``, ``load_state_dict``) or given new storage (``.to()``).  One entry per tensor OBJECT, found
    by its id and confirmed through a weak reference; the entry holds an alias of the storage it was built from, so that
    address cannot be handed out again while the entry lives, and goes away with the tensor."""
    key = id(weight)
    e = _cache.get(key)
    if (e is not None and e.ref() is weight and e.alias.data_ptr() == weight.data_ptr() and e.version == weight._version
            and e.alias.device == weight.device and e.alias.stride() == weight.stride()):
        return e.U
    K, C = weight.shape[0], weight.shape[1]
    w = weight.detach()
    dense = w.contiguous()                                                    # [K, C, 3, 3] OIHW memory
    U = torch.empty((16, C, K), dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        code = _lib.lib().mvdetr_winograd_weights_f32(dense.data_ptr(), C, K, U.data_ptr(), _lib.current_stream_ptr(w.device))
    _lib.check(code, "winograd_weights")
    e = _Entry()
    e.ref = weakref.ref(weight, lambda _, key=key: _cache.pop(key, None))
    e.alias, e.version, e.U = w, weight._version, U
    _cache[key] = e
    return U


def cached_weight_count() -> int:
    return len(_cache)


def winograd_conv3x3(x: torch.Tensor, conv: nn.Conv2d, force: bool = False) -> torch.Tensor:
    """``conv(x)`` by the Winograd kernel: a fresh channel-last tensor.  ``force`` skips the switch, the family table, the
    pixel floor and the cudnn.deterministic rule (tests and tools: any shape the kernel itself takes).  Raises when the
    arguments do not take the kernel: callers decide, nothing falls back silently here."""
    if not (_structure_ok(x, conv) if force else winograd_conv3x3_available(x, conv)):
        raise RuntimeError("winograd_conv3x3: these arguments do not take the kernel (see winograd_conv3x3_available)")
    U = _transformed_weights(conv.weight)
    N, C, H, W = x.shape
    K = conv.out_channels
    y = torch.empty((N, K, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        code = _lib.lib().mvdetr_conv3x3_winograd_f32(x.data_ptr(), U.data_ptr(), y.data_ptr(), N, H, W, C, K,
                                                      conv.dilation[0], _lib.current_stream_ptr(x.device))
    _lib.check(code, "conv3x3_winograd")
    return y


def _epilogue_ok(x, conv, bn, residual, residual_bn) -> bool:
    """The epilogue's own conditions, for the output [N, K, H, W] that ``conv(x)`` would have."""
    shape = (x.shape[0], conv.out_channels, x.shape[2], x.shape[3])
    return trunk_epilogue.bn_act_conditions(shape, x.dtype, x.device, x.requires_grad, bn, residual, residual_bn)


def winograd_conv3x3_bn_act_available(x: torch.Tensor, conv: nn.Module, bn: nn.Module, residual: torch.Tensor = None,
                                      residual_bn: nn.Module = None) -> bool:
    """True when the model runs ``act(bn(conv(x)) [+ residual | + residual_bn(residual)])`` as ONE Winograd launch:
    winograd_conv3x3_available(x, conv), the trunk's fused epilogues switched on (``set_trunk_fusion``), this module's
    own switch on (``set_winograd_epilogue``), and the BatchNorm / residual conditions of fused_bn_act_available() for
    the convolution's output.  fp32 only: 16-bit activations never take the kernel."""
    return (_epilogue and trunk_epilogue.trunk_fusion_enabled() and winograd_conv3x3_available(x, conv)
            and _epilogue_ok(x, conv, bn, residual, residual_bn))


def winograd_conv3x3_bn_act(x: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, residual: torch.Tensor = None,
                            residual_bn: nn.BatchNorm2d = None, relu: bool = True, force: bool = False) -> torch.Tensor:
    """``act(bn(conv(x)) [+ residual | + residual_bn(residual)])`` in one launch: a fresh channel-last tensor with the bits
    of ``bn_act(winograd_conv3x3(x, conv), bn, residual, residual_bn, relu=relu, inplace=True)``.  The residual is only
    read.  ``force`` skips the switches, the family table, the pixel floor and the cudnn.deterministic rule, as in
    winograd_conv3x3.  Raises when the arguments do not take the kernel."""
    ok = (_structure_ok(x, conv) and _epilogue_ok(x, conv, bn, residual, residual_bn)) if force \
        else winograd_conv3x3_bn_act_available(x, conv, bn, residual, residual_bn)
    if not ok:
        raise RuntimeError("winograd_conv3x3_bn_act: these arguments do not take the kernel "
                           "(see winograd_conv3x3_bn_act_available)")
    U = _transformed_weights(conv.weight)
    N, C, H, W = x.shape
    K = conv.out_channels
    y = torch.empty((N, K, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    bn_args = trunk_epilogue._bn_args
    with torch.cuda.device(x.device):
        code = _lib.lib().mvdetr_conv3x3_winograd_bn_act_f32(
            x.data_ptr(), U.data_ptr(), y.data_ptr(), N, H, W, C, K, conv.dilation[0], *bn_args(bn),
            0 if residual is None else residual.data_ptr(), *bn_args(residual_bn), int(bool(relu)),
            _lib.current_stream_ptr(x.device))
    _lib.check(code, "conv3x3_winograd_bn_act")
    return y
