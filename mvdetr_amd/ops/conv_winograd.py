"""The trunk's wide 3x3 convolutions as an fp32 Winograd F(2x2, 3x3) MFMA kernel (csrc/conv_winograd.hip): 2.25x fewer
multiplications than the direct form, fp32 inputs, products and sums throughout.  Inference only, channel-last fp32 CUDA
activations, stride 1, padding = dilation in {1, 2, 4}, no bias, and only the (C, K, dilation) families that measured
faster than MIOpen's pick; everything else keeps torch's convolution: the callers in model.py ask the
predicate first.

The block's inference epilogue -- BatchNorm, the residual (as it is or through the downsample BatchNorm) and ReLU -- can be
applied in the kernel's output store (winograd_conv3x3_bn_act): bn_act's arithmetic on the value a lane is about to store,
so the bits of winograd_conv3x3 followed by bn_act in place, without that pass over the output.

The transformed weights U = G g G^T (fp64, rounded once) are built once per weight tensor and cached.

Training (csrc/conv_winograd_backward.hip): winograd_conv3x3_train is the same convolution as an autograd function.  Its data
gradient is the forward kernel on grad_y with the flipped, transposed weights (Ut, cached as U is); its weight gradient is
taken in the Winograd domain by a kernel of its own, split over workgroups and summed in a fixed order.  A table and a
switch of its own (TRAIN_FAMILIES, set_trunk_winograd_training) say where the model takes it."""
from __future__ import annotations

import os
import weakref

import torch
from torch import nn

from .. import _lib
from . import trunk_epilogue

_enabled = os.environ.get("MVDETR_TRUNK_WINOGRAD", "1") != "0"
_epilogue = os.environ.get("MVDETR_WINOGRAD_EPILOGUE", "1") != "0"
_train_enabled = os.environ.get("MVDETR_TRUNK_WINOGRAD_TRAIN", "1") != "0"

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


# (C, K, dilation) whose last round runs as half units under the default tail mode: the C library's table (the tail flag of family_of in
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


# (C, K, dilation) whose 8-wave launch runs the de-phased schedule under the default mode: the C library's table
# (the dephased flag of family_of in csrc/conv_winograd.hip; tests/test_conv_winograd_schedule.py holds the two together), by the family
# rule on tools/conv_bench.py --schedule (profiles/conv_winograd_dephase_shapes.txt)
SCHEDULE_FAMILIES = ((64, 64, 1), (128, 128, 1), (256, 256, 1), (256, 256, 2), (256, 512, 2), (512, 512, 1), (512, 512, 4))


def set_winograd_schedule(schedule: int) -> int:
    """How the 8-wave kernel deals a chunk's loads and input transform to the two waves of a SIMD: 0 (the default) as the C
    library's table says for the (C, K, dilation); 1 lockstep, one program for all eight waves; 2 de-phased, waves 4-7 on a
    program of their own.  Anything else means 0.  Returns the previous setting; the bits of the result do not depend on it."""
    return int(_lib.lib().mvdetr_winograd_set_schedule(int(schedule)))


def last_schedule() -> int:
    """The schedule of the last Winograd convolution: 1 or 2 (0 before the first; 1 where the 4-wave kernel ran)."""
    return int(_lib.lib().mvdetr_winograd_last_schedule())


def schedule_of(C: int, K: int, dilation: int) -> int:
    """The schedule an 8-wave launch of this shape takes under the current setting: 1 or 2."""
    return int(_lib.lib().mvdetr_winograd_schedule_of(int(C), int(K), int(dilation)))


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


def _kernel_ok(x, conv) -> bool:
    """What the kernel itself needs of the tensors and the module, whatever the switches and autograd say."""
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
    return (256 + 2 * x.shape[2] * x.shape[3]) * max(C, K) < 1 << 30


def _needs_autograd(x, conv) -> bool:
    return torch.is_grad_enabled() and (x.requires_grad or conv.weight.requires_grad)


def _structure_ok(x, conv) -> bool:
    """What the inference entries need, whatever the switches say."""
    # nothing that needs autograd: these entries are forward only (winograd_conv3x3_train is the differentiable one)
    return _kernel_ok(x, conv) and not _needs_autograd(x, conv)


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
_cache_dgrad: dict = {}


def _cached_transform(weight: torch.Tensor, cache: dict, entry: str, shape) -> torch.Tensor:
    """The transform ``entry`` of this weight tensor from ``cache``, built on first use and again whenever the tensor was
    written in place (``_version``: ``weight.copy_``, ``load_state_dict``, an optimizer step) or given new storage (``.to()``).
    One entry per tensor OBJECT, found by its id and confirmed through a weak reference; the entry holds an alias of the storage
    it was built from, so that address cannot be handed out again while the entry lives, and goes away with the tensor."""
    key = id(weight)
    e = cache.get(key)
    if (e is not None and e.ref() is weight and e.alias.data_ptr() == weight.data_ptr() and e.version == weight._version
            and e.alias.device == weight.device and e.alias.stride() == weight.stride()):
        return e.U
    K, C = weight.shape[0], weight.shape[1]
    w = weight.detach()
    dense = w.contiguous()                                                    # [K, C, 3, 3] OIHW memory
    U = torch.empty(shape, dtype=torch.float32, device=w.device)
    with torch.cuda.device(w.device):
        code = getattr(_lib.lib(), entry)(dense.data_ptr(), C, K, U.data_ptr(), _lib.current_stream_ptr(w.device))
    _lib.check(code, entry[len("mvdetr_"):-len("_f32")])
    e = _Entry()
    e.ref = weakref.ref(weight, lambda _, key=key: cache.pop(key, None))
    e.alias, e.version, e.U = w, weight._version, U
    cache[key] = e
    return U


def _transformed_weights(weight: torch.Tensor) -> torch.Tensor:
    """U [16, C, K] of this weight tensor (the forward's), cached: see _cached_transform."""
    return _cached_transform(weight, _cache, "mvdetr_winograd_weights_f32", (16, weight.shape[1], weight.shape[0]))


def _transformed_weights_dgrad(weight: torch.Tensor) -> torch.Tensor:
    """Ut [16, K, C] of this weight tensor: the forward transform of the weights flipped in both spatial axes and transposed
    in (C, K), which turns the forward kernel into the data gradient.  Cached by the same rules, in a cache of its own."""
    return _cached_transform(weight, _cache_dgrad, "mvdetr_winograd_weights_dgrad_f32", (16, weight.shape[0], weight.shape[1]))


def cached_weight_count() -> int:
    return len(_cache)


def cached_dgrad_weight_count() -> int:
    return len(_cache_dgrad)


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


# ---- training: the convolution as an autograd function ---------------------------------------------------------------------------
# (C, K) -> {dilation: pieces}: which of "dgrad" and "wgrad" take the kernel in the model's training step; the other piece is
# torch's convolution_backward.  The rule of FAMILIES -- a piece is on where it was faster than torch's under cudnn.benchmark in
# every repetition of tools/conv_bench.py --backward at the trunk's size (profiles/conv_winograd_backward_shapes.txt) -- and a
# family with neither piece on is left out: its forward then stays torch's in training too.
TRAIN_FAMILIES: dict = {
    (64, 64): {1: ("dgrad", "wgrad")}, (128, 128): {1: ("dgrad", "wgrad")}, (128, 256): {1: ("dgrad", "wgrad")},
    (256, 256): {1: ("dgrad", "wgrad"), 2: ("dgrad", "wgrad")}, (256, 512): {2: ("dgrad", "wgrad")},
    (512, 512): {1: ("dgrad", "wgrad"), 4: ("dgrad", "wgrad")},
}
PIECES = ("dgrad", "wgrad")
_train_min_pixels = None                       # None: the inference floors (train_min_pixels)


def set_trunk_winograd_training(on: bool) -> bool:
    """Switch the Winograd convolutions of the training step on or off for this process (default on;
    ``MVDETR_TRUNK_WINOGRAD_TRAIN=0`` starts with them off).  Returns the previous setting.  ``set_trunk_winograd(False)``
    switches them off as well, whatever this says."""
    global _train_enabled
    prev, _train_enabled = _train_enabled, bool(on)
    return prev


def trunk_winograd_training_enabled() -> bool:
    return _enabled and _train_enabled


def set_winograd_train_min_pixels(pixels):
    """The pixel floor of winograd_conv3x3_train_available() for every family of TRAIN_FAMILIES (None, the default: the
    inference floor of the shape, min_pixels(), and MIN_PIXELS * 512 / K for a shape in neither inference table).  Returns the
    previous setting."""
    global _train_min_pixels
    prev, _train_min_pixels = _train_min_pixels, None if pixels is None else int(pixels)
    return prev


def train_min_pixels(C: int, K: int, dilation: int) -> int:
    if _train_min_pixels is not None:
        return _train_min_pixels
    floor = min_pixels(C, K, dilation)
    return floor if floor is not None else MIN_PIXELS * max(1, 512 // K)


def set_winograd_wgrad_splits(n: int) -> int:
    """Force the weight gradient's split S, the workgroups that share a unit's tiles (0: the default, by the unit and CU
    counts; clamped to the number of chunks); returns the previous setting.  For tests: the bits may depend on S."""
    return int(_lib.lib().mvdetr_winograd_set_wgrad_splits(int(n)))


def last_wgrad_splits() -> int:
    """The S of the last weight-gradient call (0 before the first)."""
    return int(_lib.lib().mvdetr_winograd_last_wgrad_splits())


def wgrad_plan(N: int, H: int, W: int, C: int, K: int, dilation: int, workgroups: int) -> dict:
    """How a weight-gradient call on ``workgroups`` CUs is split, under the current settings, without a device: units
    (64 x 64 channel blocks), chunks (of 8 tiles), S, the chunks per split and the chunks of the last split."""
    import ctypes
    out = (ctypes.c_int64 * 5)()
    _lib.check(_lib.lib().mvdetr_winograd_wgrad_plan(N, H, W, C, K, dilation, workgroups, ctypes.cast(out, ctypes.c_void_p)),
               "winograd_wgrad_plan")
    return dict(zip(("units", "chunks", "S", "per_split", "last_split"), (int(v) for v in out)))


_cus: dict = {}


def _device_cus(device) -> int:
    index = device.index if device.index is not None else torch.cuda.current_device()
    if index not in _cus:
        _cus[index] = int(torch.cuda.get_device_properties(index).multi_processor_count)
    return _cus[index]


def _dense_cl(t) -> bool:
    return (isinstance(t, torch.Tensor) and t.dim() == 4 and t.dtype == torch.float32 and _on_device(t) and t.numel() > 0
            and t.is_contiguous(memory_format=torch.channels_last) and t.data_ptr() % 16 == 0)


def winograd_conv3x3_input_grad(gy: torch.Tensor, weight: torch.Tensor, dilation: int) -> torch.Tensor:
    """The data gradient of ``conv2d(x, weight, stride 1, padding = dilation)`` for ``gy`` [N, K, H, W]: the forward kernel on
    gy with Ut (cached per weight tensor): a fresh channel-last [N, C, H, W].  A forward-only call.  Raises when the
    arguments do not take the kernel."""
    if not (_dense_cl(gy) and isinstance(weight, torch.Tensor) and weight.dim() == 4 and weight.dtype == torch.float32
            and weight.device == gy.device and tuple(weight.shape[2:]) == (3, 3) and weight.shape[0] == gy.shape[1]
            and weight.shape[1] % 64 == 0 and weight.shape[0] % 8 == 0 and dilation in DILATIONS
            and (256 + 2 * gy.shape[2] * gy.shape[3]) * max(weight.shape[0], weight.shape[1]) < 1 << 30):
        raise RuntimeError("winograd_conv3x3_input_grad: these arguments do not take the kernel")
    Ut = _transformed_weights_dgrad(weight)
    N, K, H, W = gy.shape
    C = weight.shape[1]
    gx = torch.empty((N, C, H, W), dtype=gy.dtype, device=gy.device, memory_format=torch.channels_last)
    with torch.cuda.device(gy.device):
        code = _lib.lib().mvdetr_conv3x3_winograd_f32(gy.data_ptr(), Ut.data_ptr(), gx.data_ptr(), N, H, W, K, C, int(dilation),
                                                      _lib.current_stream_ptr(gy.device))
    _lib.check(code, "conv3x3_winograd (data gradient)")
    return gx


def winograd_conv3x3_weight_grad(x: torch.Tensor, gy: torch.Tensor, dilation: int) -> torch.Tensor:
    """The weight gradient [K, C, 3, 3] of the same convolution for ``x`` [N, C, H, W] and ``gy`` [N, K, H, W], both dense
    channel-last fp32: the Winograd-domain kernel and its reduction, with a workspace from torch's allocator.  A forward-only
    call.  Raises when the arguments do not take the kernel."""
    if not (_dense_cl(x) and _dense_cl(gy) and x.device == gy.device and x.shape[0] == gy.shape[0]
            and x.shape[2:] == gy.shape[2:] and x.shape[1] % 64 == 0 and gy.shape[1] % 64 == 0 and dilation in DILATIONS
            and (256 + 2 * x.shape[2] * x.shape[3]) * max(x.shape[1], gy.shape[1]) < 1 << 30):
        raise RuntimeError("winograd_conv3x3_weight_grad: these arguments do not take the kernel")
    N, C, H, W = x.shape
    K = gy.shape[1]
    lib = _lib.lib()
    nbytes = int(lib.mvdetr_winograd_wgrad_workspace_bytes(N, H, W, C, K, int(dilation), _device_cus(x.device)))
    if nbytes < 0:
        raise RuntimeError("winograd_conv3x3_weight_grad: the library refuses this shape")
    workspace = torch.empty((nbytes // 4,), dtype=torch.float32, device=x.device)
    gw = torch.empty((K, C, 3, 3), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        code = lib.mvdetr_conv3x3_winograd_wgrad_f32(x.data_ptr(), gy.data_ptr(), gw.data_ptr(), N, H, W, C, K, int(dilation),
                                                     workspace.data_ptr(), nbytes, _lib.current_stream_ptr(x.device))
    _lib.check(code, "conv3x3_winograd_wgrad")
    return gw


def _train_structure_ok(x, conv) -> bool:
    return _kernel_ok(x, conv) and conv.in_channels % 64 == 0 and conv.out_channels % 64 == 0


def winograd_conv3x3_train_available(x: torch.Tensor, conv: nn.Module) -> bool:
    """True when the model runs ``conv`` on ``x`` through the differentiable Winograd convolution: both switches on
    (``set_trunk_winograd``, ``set_trunk_winograd_training``), what winograd_conv3x3_available asks of x and conv except that
    the call DOES need autograd, C and K multiples of 64, ``torch.backends.cudnn.deterministic`` off, (C, K, dilation) in
    TRAIN_FAMILIES and at least train_min_pixels() output pixels.  fp32 only: 16-bit activations never take the route."""
    if not (_enabled and _train_enabled) or torch.backends.cudnn.deterministic:
        return False
    if not (_train_structure_ok(x, conv) and _needs_autograd(x, conv)):
        return False
    C, K, d = conv.in_channels, conv.out_channels, conv.dilation[0]
    if not TRAIN_FAMILIES.get((C, K), {}).get(d):
        return False
    return x.shape[0] * x.shape[2] * x.shape[3] >= train_min_pixels(C, K, d)


class _WinogradConv3x3(torch.autograd.Function):
    """y = conv(x) by the forward kernel; grad_x by the same kernel on Ut, grad_w by the Winograd-domain kernel -- each only
    where it is needed, and each by torch's convolution_backward instead where ``pieces`` leaves it out."""

    @staticmethod
    def forward(ctx, x, weight, conv, pieces):
        U = _transformed_weights(conv.weight)
        N, C, H, W = x.shape
        K, d = conv.out_channels, conv.dilation[0]
        y = torch.empty((N, K, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
        with torch.cuda.device(x.device):
            code = _lib.lib().mvdetr_conv3x3_winograd_f32(x.data_ptr(), U.data_ptr(), y.data_ptr(), N, H, W, C, K, d,
                                                          _lib.current_stream_ptr(x.device))
        _lib.check(code, "conv3x3_winograd")
        ctx.save_for_backward(x, weight)
        ctx.conv, ctx.pieces, ctx.dilation = conv, tuple(pieces), d
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors                                         # raises if either was written in place since
        d = ctx.dilation
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if gy.dtype != torch.float32:
            raise RuntimeError("winograd_conv3x3_train: the output's gradient is not fp32")
        if not (gy.is_contiguous(memory_format=torch.channels_last) and gy.data_ptr() % 16 == 0):
            gy = gy.clone(memory_format=torch.channels_last)                  # one copy: dense channel-last, freshly allocated
        gx = gw = None
        by_torch = [need_x and "dgrad" not in ctx.pieces, need_w and "wgrad" not in ctx.pieces, False]
        if by_torch[0] or by_torch[1]:
            tx, tw, _ = torch.ops.aten.convolution_backward(gy, x, weight, None, (1, 1), (d, d), (d, d), False, (0, 0), 1, by_torch)
            gx, gw = (tx if by_torch[0] else None), (tw if by_torch[1] else None)
        if need_x and not by_torch[0]:
            gx = winograd_conv3x3_input_grad(gy, ctx.conv.weight, d)
        if need_w and not by_torch[1]:
            gw = winograd_conv3x3_weight_grad(x, gy, d)
            if gw.stride() != weight.stride():
                gw = gw.contiguous(memory_format=torch.channels_last) if weight.is_contiguous(memory_format=torch.channels_last) else gw
        return gx, gw, None, None


def winograd_conv3x3_train(x: torch.Tensor, conv: nn.Conv2d, force: bool = False) -> torch.Tensor:
    """``conv(x)`` by the Winograd kernel, differentiable once: a fresh channel-last tensor whose backward runs the data
    gradient only if x needs one and the weight gradient only if the weight does.  ``force`` skips the switches, the family
    table (both pieces then take the kernel), the pixel floor and the cudnn.deterministic rule.  Raises when the arguments do
    not take the kernel: nothing falls back silently."""
    if not (_train_structure_ok(x, conv) if force else winograd_conv3x3_train_available(x, conv)):
        raise RuntimeError("winograd_conv3x3_train: these arguments do not take the kernel (see winograd_conv3x3_train_available)")
    pieces = PIECES if force else TRAIN_FAMILIES[(conv.in_channels, conv.out_channels)][conv.dilation[0]]
    return _WinogradConv3x3.apply(x, conv.weight, conv, pieces)
