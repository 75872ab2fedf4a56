#!/usr/bin/env python3
"""Generate tests/golden/trans_world_feat_mini.npz by running the REFERENCE's own TransformerWorldFeat (and its
TransformerEncoderLayer / nn.MultiheadAttention) in eval mode on the CPU.

Runs only where the reference checkout exists; the .npz it writes is committed.  Nothing from the reference is copied: the
script imports its modules (with stub modules for the CUDA extension and for absent third-party packages that are only
touched at import time, as make_golden.py does) and records state dict, input -> output.

    python tests/golden/make_golden_trans.py

Fixture: 3 cameras, 32 channels, 24 x 72 world grid (6 x 18 = 108 tokens), dim_feedforward 64, batch 1.  ONE state dict and
ONE input serve two head counts (the parameter shapes do not depend on nhead): ``out_h8`` (8 heads, head dimension 4) and
``out_h2`` (2 heads, head dimension 16).  The input is drawn on a 1/8 grid and stored as int8 (``x_q8`` = 8 x) to keep the
file small; x = x_q8 / 8 exactly.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)

sys.modules["MultiScaleDeformableAttention"] = types.ModuleType("MultiScaleDeformableAttention")
for name in ("cv2", "kornia", "torchvision", "torchvision.models", "torchvision.transforms", "torchvision.ops"):
    if name not in sys.modules:
        sys.modules[name] = types.ModuleType(name)
sys.modules["torchvision"].models = sys.modules["torchvision.models"]
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
sys.modules["torchvision"].ops = sys.modules["torchvision.ops"]
sys.modules["torchvision.ops"].DeformConv2d = torch.nn.Module
import matplotlib  # noqa: E402
matplotlib.use("Agg")

from multiview_detector.models import trans_world_feat as ref_twf  # noqa: E402


def main():
    num_cam, Rworld, dim, dff = 3, (24, 72), 32, 64
    torch.manual_seed(23)
    x_q8 = torch.randn(1, num_cam, dim, *Rworld).mul(8).round().clamp(-127, 127).to(torch.int8)
    x = x_q8.float() / 8
    arrays, state = {}, None
    for nhead in (8, 2):
        torch.manual_seed(29)
        model = ref_twf.TransformerWorldFeat(num_cam, list(Rworld), dim, hidden_dim=dim, nhead=nhead, dim_feedforward=dff)
        if state is None:
            with torch.no_grad():                                   # biases off their zero initialisation
                for n, p in model.named_parameters():
                    if n.endswith("in_proj_bias") or n.endswith("out_proj.bias"):
                        p.normal_(0, 0.2)
            state = {k: v.clone() for k, v in model.state_dict().items()}
        model.load_state_dict(state, strict=True)
        model.eval()
        with torch.no_grad():
            arrays[f"out_h{nhead}"] = model(x).numpy()
    arrays.update({"p." + k: v.numpy() for k, v in state.items()})
    path = os.path.join(HERE, "trans_world_feat_mini.npz")
    np.savez_compressed(path, x_q8=x_q8.numpy(), dims=np.array([num_cam, Rworld[0], Rworld[1], dim, dff]), **arrays)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
