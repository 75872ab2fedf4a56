"""Detection post-processing of the BEV head's output: decode + distance NMS."""
from .decode import mvdet_decode, detections_from_heatmap
from .nms import nms
from .fused import detections_from_heatmap_fused, detection_rows, nms_fused

__all__ = ["mvdet_decode", "detections_from_heatmap", "nms", "detections_from_heatmap_fused", "detection_rows", "nms_fused"]
