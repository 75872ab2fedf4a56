"""The op layer: same package shape as the reference's multiview_detector/models/ops
(functions/, modules/, and the extension module ``MultiScaleDeformableAttention``), plus the warp.

This directory can replace multiview_detector/models/ops wholesale: its
internal imports are relative.
"""
import sys as _sys

from . import MultiScaleDeformableAttention as _msda_ext

# the reference installs its extension into site-packages under this top-level name (setup.py:53)
_sys.modules.setdefault("MultiScaleDeformableAttention", _msda_ext)

from .warp import warp_perspective, WarpPerspectiveFunction  # noqa: E402,F401
from .add_layernorm import add_layer_norm  # noqa: E402,F401
from .trunk_epilogue import bn_act, bn_act_half, bn_relu_maxpool, bn_relu_maxpool_half, set_trunk_fusion  # noqa: E402,F401
from .conv_winograd import (winograd_conv3x3, winograd_conv3x3_available, winograd_conv3x3_bn_act,  # noqa: E402,F401
                            winograd_conv3x3_bn_act_available, set_trunk_winograd, set_winograd_epilogue,
                            winograd_conv3x3_train, winograd_conv3x3_train_available, winograd_conv3x3_input_grad,
                            winograd_conv3x3_weight_grad, set_trunk_winograd_training)
from .deform_conv import deform_conv2d, DeformConv2d, DeformConv2dFunction  # noqa: E402,F401
from .attention import attention, MultiheadAttention, AttentionFunction  # noqa: E402,F401
from .detect import bev_detect, distance_nms, Detections  # noqa: E402,F401
from .peak_detect import peak_detect, PeakDetections  # noqa: E402,F401
from .ingest import ingest_frames  # noqa: E402,F401
from .targets import map_targets  # noqa: E402,F401
