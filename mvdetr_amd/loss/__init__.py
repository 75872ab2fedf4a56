"""The detection losses: ``from mvdetr_amd.loss import *`` gives what the reference's ``multiview_detector.loss`` gives,
the four loss classes and nothing else.  The segment entries, the fusion switch and the launch probes are importable by
name (``from mvdetr_amd.loss import set_loss_fusion``)."""
from .gaussian_mse import GaussianMSE
from .losses import (FocalLoss, RegCELoss, RegL1Loss, focal_loss_segments, fused_loss_available, last_kernel, launch_count,
                     loss_fusion_enabled, reg_l1_loss_segments, set_loss_fusion)

__all__ = ["FocalLoss", "RegL1Loss", "RegCELoss", "GaussianMSE"]
