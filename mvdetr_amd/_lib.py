"""ctypes binding of libmvdetr_ops.so (C ABI in include/mvdetr_ops.h).

There is NO fallback: if the shared library is missing or does not export the expected symbols
the import of the op layer raises.  GPU tensors only ever reach the HIP kernels; calls whose tensors are ALL on
the CPU run the same library's own host path (csrc/host_path.cpp -- where the reference extension raises
"Not implemented on the CPU", ms_deform_attn.h:38); mixed devices raise.
"""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import torch  # noqa: F401  (must be imported first: it loads the HIP runtime this library binds to)

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# MVDETR_OPS_LIB: another build of the same sources (the phase-stamp build libmvdetr_ops_trace.so of tools/experiments)
LIB_PATH = os.environ.get("MVDETR_OPS_LIB") or os.path.join(CSRC, "libmvdetr_ops.so")
ABI_VERSION = 18

_vp, _i = ctypes.c_void_p, ctypes.c_int
_MSDA_FWD = [_vp] * 6 + [_i] * 7 + [_vp]
_MSDA_BWD = [_vp] * 7 + [_i] * 7 + [_vp] * 3
_WARP = [_vp] * 3 + [_i] * 7 + [_vp]
_MSDA_FWD_HOST = [_vp] * 5 + [_i] * 7 + [_vp]
_MSDA_BWD_HOST = [_vp] * 6 + [_i] * 7 + [_vp] * 3
_WARP_HOST = [_vp] * 2 + [_i] * 8 + [_vp]
_MSDA_FUSED = [_vp] * 5 + [ctypes.c_int64] + [_vp] * 2 + [_i] * 10 + [_vp]
_MSDA_FUSED_HALF = [_vp] * 5 + [ctypes.c_int64, _vp] + [_i] * 7 + [_vp]
_MSDA_FUSED_LEVELS = [_vp] * 5 + [ctypes.c_int64] + [_vp] * 2 + [_i] * 12 + [_vp]
_DC_FWD = [_vp] * 5 + [_i] * 15 + [_vp]
_DC_BWD = [_vp] * 5 + [_i] * 15 + [_vp] * 3
_DC_FWD_HALF = [_vp] * 5 + [_i] * 16 + [ctypes.c_int64, _vp]
_i64p, _d, _u64 = ctypes.POINTER(ctypes.c_int64), ctypes.c_double, ctypes.c_uint64
_ATTN_FWD = [_vp] * 4 + [_i64p] + [_i] * 5 + [_d, _u64] + [_vp] * 2
_ATTN_BWD = [_vp] * 7 + [_i64p] + [_i] * 5 + [_d, _u64] + [_vp] * 4


class FocalSegment(ctypes.Structure):
    """mvdetr_focal_segment of the header: one heat map of a focal-loss launch."""
    _fields_ = [("logits", _vp), ("target", _vp), ("mask", _vp), ("grad", _vp), ("stride", ctypes.c_int64 * 4),
                ("grad_stride", ctypes.c_int64 * 4), ("batch", _i), ("channels", _i), ("height", _i), ("width", _i),
                ("weight", _d)]


class L1Segment(ctypes.Structure):
    """mvdetr_l1_segment of the header: one regression map of a masked-L1 launch."""
    _fields_ = [("output", _vp), ("mask", _vp), ("ind", _vp), ("target", _vp), ("grad", _vp), ("stride", ctypes.c_int64 * 4),
                ("grad_stride", ctypes.c_int64 * 4), ("batch", _i), ("channels", _i), ("height", _i), ("width", _i), ("k", _i),
                ("weight", _d)]


LOSS_MAX_SEGMENTS = 4
_DETECT = [_vp, _vp, _i64p, _vp, _i64p] + [_i] * 3 + [_d] * 3 + [_i] * 3 + [_vp] * 4
_NMS = [_vp] * 3 + [_i, _d, _i] + [_vp] * 3
_PEAK = [_vp, _vp, _i64p, _vp, _i64p, _vp, _i64p] + [_i] * 4 + [_d, _i, _d] + [_vp] * 7
_INGEST = [_vp, _vp, ctypes.c_int64, ctypes.c_int64, _vp] + [ctypes.c_float] * 6 + [_i] * 6 + [ctypes.c_float, _vp]
_INGEST_HOST = [_vp, ctypes.c_int64, ctypes.c_int64, _vp] + [_d] * 6 + [_i] * 6 + [_d, _vp]
_FRAME_TARGETS = [_vp, _vp, _i] + [_vp] * 6 + [_i] * 8 + [_d] + [_vp] * 6
_FSEG, _LSEG = ctypes.POINTER(FocalSegment), ctypes.POINTER(L1Segment)

SIGNATURES = {
    "mvdetr_ops_abi_version": ([], _i),
    "mvdetr_msda_last_forward_impl": ([], ctypes.c_char_p),
    "mvdetr_msda_last_forward_kernel": ([], ctypes.c_char_p),
    "mvdetr_msda_last_backward_route": ([], ctypes.c_char_p),
    "mvdetr_msda_last_forward_resources": ([ctypes.POINTER(ctypes.c_int)] * 3, _i),
    "mvdetr_msda_set_forward_impl": ([_i], _i),
    "mvdetr_msda_set_backward_deterministic": ([_i], _i),
    "mvdetr_msda_get_backward_deterministic": ([], _i),
    "mvdetr_msda_release_scratch": ([], _i),
    "mvdetr_warp_last_kernel": ([], ctypes.c_char_p),
    "mvdetr_warp_release_scratch": ([], _i),
    "mvdetr_msda_forward_f32": (_MSDA_FWD, _i),
    "mvdetr_msda_forward_f64": (_MSDA_FWD, _i),
    "mvdetr_msda_forward_f16": (_MSDA_FWD, _i),
    "mvdetr_msda_forward_bf16": (_MSDA_FWD, _i),
    "mvdetr_msda_fused_supported": ([_i] * 7, _i),
    "mvdetr_msda_forward_fused_f32": (_MSDA_FUSED, _i),
    "mvdetr_msda_fused_half_supported": ([_i] * 7, _i),
    "mvdetr_msda_forward_fused_f16": (_MSDA_FUSED_HALF, _i),
    "mvdetr_msda_forward_fused_bf16": (_MSDA_FUSED_HALF, _i),
    "mvdetr_msda_fused_levels_supported": ([_i] * 9, _i),
    "mvdetr_msda_forward_fused_levels_f32": (_MSDA_FUSED_LEVELS, _i),
    "mvdetr_msda_fused_train_supported": ([_i] * 7, _i),
    "mvdetr_msda_forward_fused_train_f32": ([_vp] * 5 + [ctypes.c_int64, _vp] + [_i] * 7 + [_vp, _vp], _i),
    "mvdetr_msda_backward_fused_f32": ([_vp] * 6 + [ctypes.c_int64, _vp, _i, _vp, _vp] + [_i] * 6 + [_vp, _vp], _i),
    "mvdetr_msda_backward_f32": (_MSDA_BWD, _i),
    "mvdetr_msda_backward_f64": (_MSDA_BWD, _i),
    "mvdetr_add_layernorm_f32": ([_vp] * 5 + [ctypes.c_int64, _i, ctypes.c_float, _vp], _i),
    "mvdetr_add_layernorm_add_f32": ([_vp] * 6 + [ctypes.c_int64, ctypes.c_int64, _i, ctypes.c_float, _vp, _vp], _i),
    "mvdetr_add_layernorm_add_f16": ([_vp] * 6 + [ctypes.c_int64, ctypes.c_int64, _i, ctypes.c_float, _vp, _vp], _i),
    "mvdetr_add_layernorm_add_bf16": ([_vp] * 6 + [ctypes.c_int64, ctypes.c_int64, _i, ctypes.c_float, _vp, _vp], _i),
    "mvdetr_add_layernorm_last_kernel": ([], ctypes.c_char_p),
    "mvdetr_bn_act_f32": ([_vp] * 6 + [ctypes.c_float] + [_vp] * 5 + [ctypes.c_float, ctypes.c_int64, _i, _i, _vp], _i),
    "mvdetr_bn_relu_maxpool_f32": ([_vp] * 6 + [ctypes.c_float] + [_i] * 4 + [_vp], _i),
    "mvdetr_bn_act_f16": ([_vp] * 6 + [ctypes.c_float] + [_vp] * 5 + [ctypes.c_float, ctypes.c_int64, _i, _i, _vp], _i),
    "mvdetr_bn_act_bf16": ([_vp] * 6 + [ctypes.c_float] + [_vp] * 5 + [ctypes.c_float, ctypes.c_int64, _i, _i, _vp], _i),
    "mvdetr_bn_relu_maxpool_f16": ([_vp] * 6 + [ctypes.c_float] + [_i] * 4 + [_vp], _i),
    "mvdetr_bn_relu_maxpool_bf16": ([_vp] * 6 + [ctypes.c_float] + [_i] * 4 + [_vp], _i),
    "mvdetr_trunk_last_kernel": ([], ctypes.c_char_p),
    "mvdetr_trunk_launch_count": ([], ctypes.c_int64),
    "mvdetr_winograd_weights_f32": ([_vp, _i, _i, _vp, _vp], _i),
    "mvdetr_conv3x3_winograd_f32": ([_vp] * 3 + [_i] * 6 + [_vp], _i),
    "mvdetr_conv3x3_winograd_bn_act_f32": ([_vp] * 3 + [_i] * 6 + [_vp] * 4 + [ctypes.c_float] + [_vp] * 5
                                           + [ctypes.c_float, _i, _vp], _i),
    "mvdetr_winograd_last_kernel": ([], ctypes.c_char_p),
    "mvdetr_winograd_last_epilogue": ([], ctypes.c_char_p),
    "mvdetr_winograd_launch_count": ([], ctypes.c_int64),
    "mvdetr_winograd_set_max_workgroups": ([_i], _i),
    "mvdetr_winograd_set_tail": ([_i], _i),
    "mvdetr_winograd_set_variant": ([_i], _i),
    "mvdetr_winograd_last_variant": ([], _i),
    "mvdetr_winograd_last_tail_units": ([], _i),
    "mvdetr_winograd_set_schedule": ([_i], _i),
    "mvdetr_winograd_last_schedule": ([], _i),
    "mvdetr_winograd_schedule_of": ([_i] * 3, _i),
    "mvdetr_winograd_plan": ([_i] * 7 + [_vp], _i),
    "mvdetr_winograd_weights_dgrad_f32": ([_vp, _i, _i, _vp, _vp], _i),
    "mvdetr_conv3x3_winograd_wgrad_f32": ([_vp] * 3 + [_i] * 6 + [_vp, ctypes.c_int64, _vp], _i),
    "mvdetr_winograd_wgrad_workspace_bytes": ([_i] * 7, ctypes.c_int64),
    "mvdetr_winograd_wgrad_plan": ([_i] * 7 + [_vp], _i),
    "mvdetr_winograd_set_wgrad_splits": ([_i], _i),
    "mvdetr_winograd_last_wgrad_splits": ([], _i),
    "mvdetr_warp_perspective_forward_f32": (_WARP, _i),
    "mvdetr_warp_perspective_forward_f64": (_WARP, _i),
    "mvdetr_warp_perspective_forward_f16": (_WARP, _i),
    "mvdetr_warp_perspective_forward_bf16": (_WARP, _i),
    "mvdetr_warp_perspective_backward_f32": (_WARP, _i),
    "mvdetr_warp_perspective_backward_f64": (_WARP, _i),
    "mvdetr_warp_perspective_backward_tagged_f32": ([_vp] * 3 + [_i] * 7 + [ctypes.c_uint64, _vp], _i),
    "mvdetr_warp_perspective_backward_tagged_f64": ([_vp] * 3 + [_i] * 7 + [ctypes.c_uint64, _vp], _i),
    "mvdetr_warp_backward_plan_bytes": ([_i] * 7, ctypes.c_int64),
    "mvdetr_warp_backward_plan_f32": ([_vp, _vp] + [_i] * 6 + [_vp], _i),
    "mvdetr_warp_backward_plan_f64": ([_vp, _vp] + [_i] * 6 + [_vp], _i),
    "mvdetr_warp_perspective_backward_planned_f32": ([_vp] * 4 + [_i] * 7 + [_vp], _i),
    "mvdetr_warp_perspective_backward_planned_f64": ([_vp] * 4 + [_i] * 7 + [_vp], _i),
    "mvdetr_transpose_f32": ([_vp, _vp, _i, _i, _i, _vp], _i),
    "mvdetr_transpose_f64": ([_vp, _vp, _i, _i, _i, _vp], _i),
    "mvdetr_msda_forward_host_f32": (_MSDA_FWD_HOST, _i),
    "mvdetr_msda_forward_host_f64": (_MSDA_FWD_HOST, _i),
    "mvdetr_msda_backward_host_f32": (_MSDA_BWD_HOST, _i),
    "mvdetr_msda_backward_host_f64": (_MSDA_BWD_HOST, _i),
    "mvdetr_warp_perspective_forward_host_f32": (_WARP_HOST, _i),
    "mvdetr_warp_perspective_forward_host_f64": (_WARP_HOST, _i),
    "mvdetr_warp_perspective_backward_host_f32": (_WARP_HOST, _i),
    "mvdetr_warp_perspective_backward_host_f64": (_WARP_HOST, _i),
    "mvdetr_deform_conv2d_last_kernel": ([], ctypes.c_char_p),
    "mvdetr_deform_conv2d_route_kind": ([_i] * 18, _i),
    "mvdetr_deform_conv2d_forward_f32": (_DC_FWD, _i),
    "mvdetr_deform_conv2d_forward_f64": (_DC_FWD, _i),
    "mvdetr_deform_conv2d_forward_f16": (_DC_FWD_HALF, _i),
    "mvdetr_deform_conv2d_forward_bf16": (_DC_FWD_HALF, _i),
    "mvdetr_deform_conv2d_backward_f32": (_DC_BWD, _i),
    "mvdetr_deform_conv2d_backward_f64": (_DC_BWD, _i),
    "mvdetr_deform_conv2d_forward_host_f32": (_DC_FWD[1:], _i),
    "mvdetr_deform_conv2d_forward_host_f64": (_DC_FWD[1:], _i),
    "mvdetr_deform_conv2d_backward_host_f32": (_DC_BWD[1:], _i),
    "mvdetr_deform_conv2d_backward_host_f64": (_DC_BWD[1:], _i),
    "mvdetr_attention_last_kernel": ([], ctypes.c_char_p),
    "mvdetr_attention_workspace_bytes": ([_i] * 6, ctypes.c_int64),
    "mvdetr_attention_route_kind": ([_i] * 7 + [_d, _i, _i], _i),
    "mvdetr_attention_forward_f32": (_ATTN_FWD, _i),
    "mvdetr_attention_forward_f64": (_ATTN_FWD, _i),
    "mvdetr_attn_forward_f16": ([_vp] * 4 + [_i64p] + [_i] * 5 + [_vp], _i),
    "mvdetr_attn_forward_bf16": ([_vp] * 4 + [_i64p] + [_i] * 5 + [_vp], _i),
    "mvdetr_attn_half_set_query_tile": ([_i], _i),
    "mvdetr_attention_backward_f32": (_ATTN_BWD, _i),
    "mvdetr_attention_backward_f64": (_ATTN_BWD, _i),
    "mvdetr_attention_forward_host_f32": (_ATTN_FWD[1:], _i),
    "mvdetr_attention_forward_host_f64": (_ATTN_FWD[1:], _i),
    "mvdetr_attention_backward_host_f32": (_ATTN_BWD[1:15] + _ATTN_BWD[16:], _i),
    "mvdetr_attention_backward_host_f64": (_ATTN_BWD[1:15] + _ATTN_BWD[16:], _i),
    "mvdetr_attention_dropout_mask_host": ([_u64, _d] + [_i] * 4 + [_vp], _i),
    "mvdetr_focal_loss_workspace_bytes": ([_FSEG, _i, _i], ctypes.c_int64),
    "mvdetr_focal_loss_forward_f32": ([_vp, _FSEG, _i, _vp, _vp, _vp, _vp], _i),
    "mvdetr_focal_loss_forward_f64": ([_vp, _FSEG, _i, _vp, _vp, _vp, _vp], _i),
    "mvdetr_focal_loss_backward_f32": ([_vp, _FSEG, _i, _vp, _vp], _i),
    "mvdetr_focal_loss_backward_f64": ([_vp, _FSEG, _i, _vp, _vp], _i),
    "mvdetr_reg_l1_loss_forward_f32": ([_vp, _LSEG, _i, _vp, _vp], _i),
    "mvdetr_reg_l1_loss_forward_f64": ([_vp, _LSEG, _i, _vp, _vp], _i),
    "mvdetr_reg_l1_loss_backward_f32": ([_vp, _LSEG, _i, _vp, _vp], _i),
    "mvdetr_reg_l1_loss_backward_f64": ([_vp, _LSEG, _i, _vp, _vp], _i),
    "mvdetr_loss_last_kernel": ([], ctypes.c_char_p),
    "mvdetr_loss_launch_count": ([], ctypes.c_int64),
    "mvdetr_detect_workspace_bytes": ([_i] * 4, ctypes.c_int64),
    "mvdetr_detect_forward_f32": (_DETECT, _i),
    "mvdetr_detect_forward_f64": (_DETECT, _i),
    "mvdetr_distance_nms_f32": (_NMS, _i),
    "mvdetr_distance_nms_f64": (_NMS, _i),
    "mvdetr_detect_forward_host_f32": (_DETECT[1:15] + _DETECT[16:], _i),
    "mvdetr_detect_forward_host_f64": (_DETECT[1:15] + _DETECT[16:], _i),
    "mvdetr_distance_nms_host_f32": (_NMS[1:6] + _NMS[7:], _i),
    "mvdetr_distance_nms_host_f64": (_NMS[1:6] + _NMS[7:], _i),
    "mvdetr_detect_last_kernel": ([], ctypes.c_char_p),
    "mvdetr_detect_launch_count": ([], ctypes.c_int64),
    "mvdetr_peak_detect_workspace_bytes": ([_i] * 4, ctypes.c_int64),
    "mvdetr_peak_detect_lds_capacity": ([_i], _i),
    "mvdetr_peak_detect_forward_f32": (_PEAK, _i),
    "mvdetr_peak_detect_forward_f64": (_PEAK, _i),
    "mvdetr_peak_detect_forward_host_f32": (_PEAK[1:14] + _PEAK[15:], _i),
    "mvdetr_peak_detect_forward_host_f64": (_PEAK[1:14] + _PEAK[15:], _i),
    "mvdetr_peak_detect_last_kernel": ([], ctypes.c_char_p),
    "mvdetr_peak_detect_launch_count": ([], ctypes.c_int64),
    "mvdetr_ingest_frames_f32": (_INGEST, _i),
    "mvdetr_ingest_frames_f16": (_INGEST, _i),
    "mvdetr_ingest_frames_bf16": (_INGEST, _i),
    "mvdetr_ingest_last_kernel": ([], ctypes.c_char_p),
    "mvdetr_ingest_frames_host_f32": (_INGEST_HOST, _i),
    "mvdetr_ingest_frames_host_f64": (_INGEST_HOST, _i),
    "mvdetr_frame_targets_f64": (_FRAME_TARGETS, _i),
    "mvdetr_frame_targets_host_f64": (_FRAME_TARGETS[1:], _i),
    "mvdetr_frame_targets_max_radius": ([], _i),
    "mvdetr_frame_targets_launch_count": ([], ctypes.c_int64),
}

# mvdetr_deform_conv2d_route_kind / mvdetr_attention_route_kind (include/mvdetr_ops.h): the entries, and the kinds in the order of
# DcKind (csrc/deform_conv_route.h) and AttnKind (csrc/attention_route.h); a refused or empty call answers minus ROUTE_STATUS's index
ROUTE_FORWARD, ROUTE_BACKWARD, ROUTE_FORWARD_HALF = 0, 1, 2
DC_KINDS = ("fwd_generic", "fwd_mfma", "fwd_mfma_half", "bwd_generic", "bwd_mfma", "bwd_zero_fill")
ATTN_KINDS = ("fwd_generic", "fwd_mfma", "fwd_mfma_half", "bwd_generic", "bwd_mfma")
ROUTE_STATUS = ("ok", "empty", "invalid_value", "not_supported")


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j4"] + (["-B"] if force else [])
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        raise RuntimeError("building libmvdetr_ops.so failed:\n" + res.stdout)
    if verbose:
        print(res.stdout)
    return LIB_PATH


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C mvdetr_amd/csrc`). "
                "There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (argtypes, restype) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                raise ImportError(f"{LIB_PATH} does not export {name}") from e
            fn.argtypes, fn.restype = argtypes, restype
        got = handle.mvdetr_ops_abi_version()
        if got != ABI_VERSION:
            raise ImportError(f"{LIB_PATH}: ABI version {got}, expected {ABI_VERSION} (stale build?)")
        _lib = handle
    return _lib


# (cached: the route is a pure function of these integers, and a dictionary look-up costs a fraction of the foreign call on a
# path that is taken once per forward)
@functools.lru_cache(maxsize=1024)
def dc_route(entry: int, elem_size: int, *args) -> str:
    """mvdetr_deform_conv2d_route_kind by name: one of DC_KINDS, or of ROUTE_STATUS for a call that launches nothing."""
    kind = lib().mvdetr_deform_conv2d_route_kind(entry, elem_size, *args)
    return DC_KINDS[kind] if kind >= 0 else ROUTE_STATUS[-kind]


@functools.lru_cache(maxsize=1024)
def attn_route(entry: int, elem_size: int, *args) -> str:
    """mvdetr_attention_route_kind by name: one of ATTN_KINDS, or of ROUTE_STATUS for a call that launches nothing."""
    kind = lib().mvdetr_attention_route_kind(entry, elem_size, *args)
    return ATTN_KINDS[kind] if kind >= 0 else ROUTE_STATUS[-kind]


def check(rc: int, what: str) -> None:
    """Launch failures raise (the reference only printf's them, cuh:948-952)."""
    if rc != 0:
        name = "hipErrorInvalidValue" if rc == 1 else f"hipError {rc}"
        raise RuntimeError(f"{what} failed: {name}")


def current_stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def suffix(dtype, half_ok=False) -> str:
    if dtype == torch.float32:
        return "f32"
    if dtype == torch.float64:
        return "f64"
    if half_ok and dtype == torch.float16:
        return "f16"
    if half_ok and dtype == torch.bfloat16:
        return "bf16"
    # AT_DISPATCH_FLOATING_TYPES in the reference: float and double only (ms_deform_attn_cuda.cu:64)
    raise RuntimeError(f'"mvdetr_ops" not implemented for \'{dtype}\'')
