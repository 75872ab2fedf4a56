"""CPU-side checks of the trunk's 16-bit fused epilogues (mvdetr_amd/ops/trunk_epilogue.py: bn_act_half,
bn_relu_maxpool_half): the four C-ABI symbols are declared, bound and exported without an ABI bump; the C entry points
refuse bad arguments before launching anything; on CPU tensors the new predicates are False and the ops raise; the fp32
predicates keep refusing 16-bit tensors."""
import os
import re

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["mvdetr_bn_act_f16", "mvdetr_bn_act_bf16", "mvdetr_bn_relu_maxpool_f16", "mvdetr_bn_relu_maxpool_bf16"]
HALF = [torch.float16, torch.bfloat16]


def test_new_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from mvdetr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mvdetr_ops.h")).read()
    declared = set(re.findall(r"\b(mvdetr_[a-z0-9_]+)\s*\(", hdr))
    _lib.build()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None                                  # exported by the built library
        # same argument list as the fp32 entry, the tensors as 16-bit words, the BatchNorm vectors as floats
        proto = re.search(r"int " + name + r"\((.*?)\);", hdr, re.S).group(1)
        proto32 = re.search(r"int " + re.sub(r"_b?f16$", "_f32", name) + r"\((.*?)\);", hdr, re.S).group(1)
        norm = lambda p: re.sub(r"\s+", " ", p).strip()  # noqa: E731
        for t in ("x", "res", "y"):
            proto32 = re.sub(r"float \*" + t + r"\b", "uint16_t *" + t, proto32)
        assert norm(proto) == norm(proto32), (name, proto)
        assert "const float *mean" in proto and "const float *var" in proto
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[re.sub(r"_b?f16$", "_f32", name)]
    assert _lib.ABI_VERSION == 18 and lib.mvdetr_ops_abi_version() == 18
    assert re.search(r"#define MVDETR_OPS_ABI_VERSION 18\b", hdr)


@pytest.mark.parametrize("suffix", ["f16", "bf16"])
def test_c_entry_points_refuse_bad_arguments_without_launching(suffix):
    from mvdetr_amd import _lib
    _lib.build()
    lib = _lib.lib()
    act, pool = getattr(lib, "mvdetr_bn_act_" + suffix), getattr(lib, "mvdetr_bn_relu_maxpool_" + suffix)
    before = lib.mvdetr_trunk_launch_count()
    last = lib.mvdetr_trunk_last_kernel()
    a = 4096                                               # (a 16-byte aligned non-null address; nothing dereferences it)
    bad = {
        "x null": act(0, 0, a, a, a, a, 1e-5, 0, 0, 0, 0, 0, 0.0, 8, 64, 1, a),
        "y null": act(0, a, a, a, a, a, 1e-5, 0, 0, 0, 0, 0, 0.0, 8, 64, 1, 0),
        "C % 8 (62)": act(0, a, a, a, a, a, 1e-5, 0, 0, 0, 0, 0, 0.0, 8, 62, 1, a),
        "C % 8 (68: a multiple of 4)": act(0, a, a, a, a, a, 1e-5, 0, 0, 0, 0, 0, 0.0, 8, 68, 1, a),
        "no running mean": act(0, a, 0, a, a, a, 1e-5, 0, 0, 0, 0, 0, 0.0, 8, 64, 1, a),
        "residual BN without residual": act(0, a, a, a, a, a, 1e-5, 0, a, a, 0, 0, 1e-5, 8, 64, 1, a),
        "residual is the output": act(0, a, a, a, a, a, 1e-5, a + 16, 0, 0, 0, 0, 0.0, 8, 64, 1, a + 16),
        "misaligned x": act(0, a + 4, a, a, a, a, 1e-5, 0, 0, 0, 0, 0, 0.0, 8, 64, 1, a),
        "misaligned residual": act(0, a, a, a, a, a, 1e-5, a + 8, 0, 0, 0, 0, 0.0, 8, 64, 1, a),
        "rows < 0": act(0, a, a, a, a, a, 1e-5, 0, 0, 0, 0, 0, 0.0, -1, 64, 1, a),
        "pool in place": pool(0, a, a, a, a, a, 1e-5, 1, 8, 8, 64, a),
        "pool, empty image": pool(0, a, a, a, a, a, 1e-5, 1, 0, 8, 64, a + 16),
        "pool, C % 8 (68)": pool(0, a, a, a, a, a, 1e-5, 1, 8, 8, 68, a + 16),
        "pool, C/8 = 12 does not tile 256": pool(0, a, a, a, a, a, 1e-5, 1, 8, 8, 96, a + 16),
    }
    assert all(rc != 0 for rc in bad.values()), bad
    assert bad["C % 8 (68: a multiple of 4)"] == bad["pool, C % 8 (68)"] == 1             # hipErrorInvalidValue
    assert bad["pool, C/8 = 12 does not tile 256"] == 801                                   # hipErrorNotSupported
    assert act(0, a, a, a, a, a, 1e-5, 0, 0, 0, 0, 0, 0.0, 0, 64, 1, a) == 0                # rows = 0: nothing to do
    assert pool(0, a, a, a, a, a, 1e-5, 0, 8, 8, 64, a + 16) == 0                           # n = 0 likewise
    assert lib.mvdetr_trunk_launch_count() == before and lib.mvdetr_trunk_last_kernel() == last
    with pytest.raises(RuntimeError):
        _lib.check(bad["x null"], "bn_act")


@pytest.mark.parametrize("dtype", HALF)
def test_half_predicates_refuse_cpu_tensors_and_the_ops_raise(dtype):
    from mvdetr_amd import ops
    from mvdetr_amd.ops import trunk_epilogue as te
    assert ops.bn_act_half is te.bn_act_half and ops.bn_relu_maxpool_half is te.bn_relu_maxpool_half
    bn = nn.BatchNorm2d(64).eval()
    x = torch.randn(1, 64, 4, 4).to(dtype).contiguous(memory_format=torch.channels_last)
    assert te.trunk_fusion_enabled()
    assert not te.fused_bn_act_half_available(x, bn)
    assert not te.fused_bn_act_half_available(x, bn, x.clone(memory_format=torch.preserve_format))
    assert not te.fused_bn_relu_maxpool_half_available(x, bn, nn.ReLU(), nn.MaxPool2d(3, 2, 1))
    with pytest.raises(RuntimeError, match="fused kernel"):
        te.bn_act_half(x, bn)
    with pytest.raises(RuntimeError, match="fused kernel"):
        te.bn_relu_maxpool_half(x, bn)
    # the fp32 surface is as it was: 16-bit tensors are not its business, on any device
    assert not te.fused_bn_act_available(x, bn)
    assert not te.fused_bn_relu_maxpool_available(x, bn, nn.ReLU(), nn.MaxPool2d(3, 2, 1))
    with pytest.raises(RuntimeError, match="fused kernel"):
        te.bn_act(x, bn)
    # and fp32 tensors are not the 16-bit surface's
    assert not te.fused_bn_act_half_available(x.float(), bn)


def test_cpu_16_bit_trunk_is_the_children_one_after_another():
    """A bfloat16 trunk on the CPU (BatchNorm kept fp32, as to_inference leaves it) computes exactly what its children
    compute one after another: nothing is fused there."""
    from mvdetr_amd.model import resnet_trunk
    from mvdetr_amd.ops import trunk_epilogue as te
    torch.manual_seed(0)
    trunk = resnet_trunk(18).eval()
    for m in trunk.modules():
        if isinstance(m, nn.Conv2d):
            m.to(torch.bfloat16)
    x = torch.randn(1, 3, 32, 32).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def block(b, x):
        identity = x if b.downsample is None else b.downsample(x)
        out = b.relu(b.bn1(b.conv1(x)))
        return b.relu(b.bn2(b.conv2(out)) + identity)

    with torch.no_grad():
        before = te.launch_count()
        got = trunk(x)
        assert te.launch_count() == before
        want = x
        for i, m in enumerate(trunk.children()):
            if i < 4:
                want = m(want)
            else:
                for b in m:
                    want = block(b, want)
    assert got.dtype == torch.bfloat16 and torch.equal(got, want)
