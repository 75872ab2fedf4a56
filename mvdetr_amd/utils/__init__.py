"""Detection post-processing of the heads' outputs: decode + distance NMS for the BEV maps, peak + top-K
decode (``ctdet_decode``) for the image-plane maps or as the BEV maps' peak-based alternative."""
from .decode import mvdet_decode, detections_from_heatmap, ctdet_decode
from .nms import nms
from .fused import detections_from_heatmap_fused, detection_rows, nms_fused, ctdet_decode_fused

__all__ = ["mvdet_decode", "detections_from_heatmap", "nms", "detections_from_heatmap_fused", "detection_rows", "nms_fused",
           "ctdet_decode", "ctdet_decode_fused"]
