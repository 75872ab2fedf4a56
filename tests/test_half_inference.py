"""16-bit inference, the part that needs no GPU: the new C-ABI symbols, what MVDeTr.to_inference converts and what it must
leave alone (nn.Module.half() would round the projection matrices and the encoder's reference map), and the limits the ops
state instead of computing something wrong."""
import os
import re

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = [
    "mvdetr_warp_perspective_forward_f16", "mvdetr_warp_perspective_forward_bf16",
    "mvdetr_msda_fused_half_supported", "mvdetr_msda_forward_fused_f16", "mvdetr_msda_forward_fused_bf16",
    "mvdetr_add_layernorm_add_f16", "mvdetr_add_layernorm_add_bf16",
]


def test_new_symbols_are_declared_and_bound_and_the_abi_version_stays():
    from mvdetr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mvdetr_ops.h")).read()
    declared = set(re.findall(r"\b(mvdetr_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 18
    assert re.search(r"#define MVDETR_OPS_ABI_VERSION 18\b", hdr)
    # 16-bit tensors cross the ABI as uint16_t *, the warp's matrices and the reference points stay float
    for name in NEW_SYMBOLS:
        if name.endswith("_supported"):
            continue
        proto = re.search(r"int " + name + r"\((.*?)\);", hdr, re.S).group(1)
        assert "uint16_t *" in proto and "double" not in proto, proto
    assert "const float *M" in re.search(r"int mvdetr_warp_perspective_forward_bf16\((.*?)\);", hdr, re.S).group(1)
    assert "const float *reference_points" in re.search(r"int mvdetr_msda_forward_fused_f16\((.*?)\);", hdr, re.S).group(1)


def test_fused_half_support_rule():
    from mvdetr_amd import _lib
    ok = _lib.lib().mvdetr_msda_fused_half_supported
    assert ok(1, 7 * 60 * 180, 8, 16, 7, 7 * 60 * 180, 4) == 1          # Wildtrack's encoder call
    assert ok(2, 3 * 6 * 9, 4, 32, 3, 3 * 6 * 9, 4) == 1
    assert ok(1, 70, 8, 16, 2, 70, 2) == 0                               # two points
    assert ok(1, 70, 8, 8, 2, 70, 4) == 0                                # 8-channel heads
    assert ok(1, 70, 8, 16, 2, 35, 4) == 0                               # queries are not the tokens
    assert ok(1, 17 * 4, 8, 16, 17, 17 * 4, 4) == 0                      # more than 16 levels


@pytest.fixture(scope="module")
def twins():
    from mvdetr_amd.model import build_model
    plain = build_model("mini", seed=0)
    conv = build_model("mini", seed=0).to_inference(torch.bfloat16)
    return plain, conv


def test_to_inference_casts_the_layers_and_keeps_batchnorm_fp32(twins):
    _, model = twins
    assert model.compute_dtype == torch.bfloat16 and not model.training
    seen = set()
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            seen.add("bn")
            assert m.weight.dtype == m.bias.dtype == torch.float32
            assert m.running_mean.dtype == m.running_var.dtype == torch.float32
        elif isinstance(m, (nn.Conv2d, nn.Linear, nn.LayerNorm)):
            seen.add(type(m).__name__)
            assert all(p.dtype == torch.bfloat16 for p in m.parameters(recurse=False)), type(m)
    assert seen == {"bn", "Conv2d", "Linear", "LayerNorm"}
    assert model.world_feat.lvl_embedding.dtype == torch.bfloat16
    assert model.world_feat.pos_embedding.dtype == torch.bfloat16
    # every parameter outside a BatchNorm was converted
    bn_params = {id(p) for m in model.modules() if isinstance(m, nn.BatchNorm2d) for p in m.parameters(recurse=False)}
    assert all(p.dtype == torch.bfloat16 for p in model.parameters() if id(p) not in bn_params)


def test_to_inference_leaves_the_geometry_bit_for_bit(twins):
    plain, model = twins
    assert model.proj_mats.dtype == torch.float64 and torch.equal(model.proj_mats, plain.proj_mats)
    enc, enc0 = model.world_feat.encoder, plain.world_feat.encoder
    assert enc.reference_points.dtype == enc0.reference_points.dtype == torch.float32
    assert torch.equal(enc.reference_points, enc0.reference_points)
    assert enc.reference_shared is not None and enc.reference_shared.dtype == torch.float32
    assert torch.equal(enc.reference_shared, enc0.reference_shared)
    assert torch.equal(enc.shared_reference(), enc0.shared_reference())
    M = torch.eye(3).repeat(1, model.num_cam, 1, 1)
    M[0, 1, 0, 2] = 3.5                                                  # an augmentation that moves one view
    a, b = model.frame_proj_mats(M), plain.frame_proj_mats(M)
    assert a.dtype == b.dtype == torch.float32 and torch.equal(a, b)


def test_to_inference_refuses_what_it_cannot_serve():
    from mvdetr_amd.model import build_model
    for arch in ("deform_conv", "trans"):
        with pytest.raises(NotImplementedError, match=arch):
            build_model("mini", seed=0, world_feat_arch=arch, channels_last=False).to_inference(torch.float16)
    with pytest.raises(ValueError):
        build_model("mini", seed=0).to_inference(torch.float32)
    conv = build_model("mini", seed=0, world_feat_arch="conv", channels_last=False).to_inference(torch.float16)
    assert conv.world_feat.coord_map.dtype == torch.float16 and conv.proj_mats.dtype == torch.float64


def test_half_warp_on_the_cpu_and_with_grad_is_refused():
    from mvdetr_amd.ops import warp_perspective
    M = torch.eye(3)[None]
    for dtype in (torch.float16, torch.bfloat16):
        with pytest.raises(RuntimeError, match="GPU only"):
            warp_perspective(torch.zeros(1, 8, 4, 4, dtype=dtype), M, (4, 4))
    assert warp_perspective(torch.zeros(1, 8, 4, 4), M, (4, 4)).dtype == torch.float32      # the fp32 host path is as it was


def test_add_layer_norm_predicate_wants_one_dtype():
    """The 16-bit kernel takes x, residual, then_add and the norm's parameters in ONE dtype: a bf16 row with an fp32 norm
    (an unconverted module) keeps torch's ops.  (CPU tensors never qualify.)"""
    from mvdetr_amd.ops.add_layernorm import FUSED_DTYPES, fused_add_layer_norm_available
    assert torch.float16 in FUSED_DTYPES and torch.bfloat16 in FUSED_DTYPES
    norm = nn.LayerNorm(128)
    with torch.no_grad():
        assert not fused_add_layer_norm_available(torch.zeros(4, 128, dtype=torch.bfloat16), norm)
