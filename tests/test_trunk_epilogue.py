"""CPU-side checks of the trunk's fused inference epilogues (mvdetr_amd/ops/trunk_epilogue.py): on CPU tensors nothing
is fused and the trunk computes exactly what running its children one after another computes; its state_dict is the
parent's key for key; the predicates refuse everything the kernels do not take; the C entry points refuse bad arguments
before launching anything."""
import json
import os

import pytest
import torch
from torch import nn

from conftest import GOLDEN


def _children_one_by_one(trunk, x):
    """The trunk as plain torch runs an nn.Sequential of these modules, blocks written out as in torchvision."""
    def block(b, x):
        identity = x if b.downsample is None else b.downsample(x)
        out = b.relu(b.bn1(b.conv1(x)))
        if hasattr(b, "conv3"):
            out = b.relu(b.bn2(b.conv2(out)))
            out = b.bn3(b.conv3(out))
        else:
            out = b.bn2(b.conv2(out))
        return b.relu(out + identity)
    for i, m in enumerate(trunk.children()):
        x = nn.Sequential(*[_Block(b, block) for b in m])(x) if i >= 4 else m(x)
    return x


class _Block(nn.Module):
    def __init__(self, b, fn):
        super().__init__()
        self.b, self.fn = b, fn

    def forward(self, x):
        return self.fn(self.b, x)


def _randomise_bn(trunk, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in trunk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.2)


@pytest.mark.parametrize("depth", [18, 50])
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("channels_last", [True, False])
def test_cpu_forward_is_the_children_one_after_another(depth, mode, channels_last):
    from mvdetr_amd.model import resnet_trunk
    torch.manual_seed(depth)
    trunk = resnet_trunk(depth)
    _randomise_bn(trunk)
    trunk.train(mode == "train")
    x = torch.randn(2, 3, 40, 56)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    state = {k: v.clone() for k, v in trunk.state_dict().items()}
    with torch.no_grad():
        got = trunk(x)
        after = {k: v.clone() for k, v in trunk.state_dict().items()}
        trunk.load_state_dict(state)                       # (train mode moved the running statistics)
        want = _children_one_by_one(trunk, x)
    assert got.shape == (2, 512 if depth == 18 else 2048, 5, 7)
    assert torch.equal(got, want)
    for k, v in trunk.state_dict().items():
        assert torch.equal(v, after[k]), k


def test_cpu_forward_with_gradients_reaches_the_stem():
    from mvdetr_amd.model import resnet_trunk
    torch.manual_seed(1)
    trunk = resnet_trunk(18).eval()
    trunk(torch.randn(1, 3, 32, 32)).square().mean().backward()
    assert trunk[0].weight.grad is not None and trunk[0].weight.grad.abs().sum() > 0


@pytest.mark.parametrize("depth", [18, 50])
def test_state_dict_keys_and_shapes_are_the_parents(depth):
    """The literal list was written by the commit before the fused epilogues (an nn.Sequential of the same children)."""
    from mvdetr_amd.model import resnet_trunk
    want = json.load(open(os.path.join(GOLDEN, "trunk_state_dict_parent.json")))[f"resnet{depth}"]
    got = [[k, list(v.shape)] for k, v in resnet_trunk(depth).state_dict().items()]
    assert got == want
    assert got[0] == ["0.weight", [64, 3, 7, 7]] and ["1.running_mean", [64]] in got
    assert any(k == "5.0.downsample.1.weight" for k, _ in got) and any(k == "4.0.conv1.weight" for k, _ in got)


def test_model_state_dict_names_the_trunk_as_base():
    from mvdetr_amd.model import build_model
    keys = list(build_model("mini", seed=0).state_dict())
    for k in ("base.0.weight", "base.1.running_mean", "base.4.0.conv1.weight", "base.5.0.downsample.1.weight"):
        assert k in keys


def test_trunk_is_a_sequential_that_pickles_and_copies():
    import copy
    import pickle
    from mvdetr_amd.model import resnet_trunk
    trunk = resnet_trunk(18).eval()
    assert isinstance(trunk, nn.Sequential) and len(trunk) == 8
    x = torch.randn(1, 3, 32, 32)
    with torch.no_grad():
        want = trunk(x)
        assert torch.equal(copy.deepcopy(trunk)(x), want)
        assert torch.equal(pickle.loads(pickle.dumps(trunk))(x), want)


def test_predicates_refuse_cpu_tensors_and_the_switch_is_a_process_setting():
    from mvdetr_amd.ops import trunk_epilogue as te
    bn = nn.BatchNorm2d(64).eval()
    x = torch.randn(1, 64, 4, 4).contiguous(memory_format=torch.channels_last)
    assert not te.fused_bn_act_available(x, bn)
    assert not te.fused_bn_relu_maxpool_available(x, bn, nn.ReLU(), nn.MaxPool2d(3, 2, 1))
    with pytest.raises(RuntimeError, match="fused kernel"):
        te.bn_act(x, bn)
    with pytest.raises(RuntimeError, match="fused kernel"):
        te.bn_relu_maxpool(x, bn)
    prev = te.set_trunk_fusion(False)
    try:
        assert te.trunk_fusion_enabled() is False and te.set_trunk_fusion(True) is False and te.trunk_fusion_enabled() is True
    finally:
        te.set_trunk_fusion(prev)


def test_environment_switch_starts_the_process_with_fusion_off():
    import subprocess
    import sys
    from conftest import ROOT
    code = "import sys; sys.path.insert(0, %r)\nfrom mvdetr_amd.ops import trunk_epilogue as te\nprint('ENABLED', te.trunk_fusion_enabled())\n" % ROOT
    for value, want in (("0", "False"), ("1", "True"), (None, "True")):
        env = {k: v for k, v in os.environ.items() if k != "MVDETR_TRUNK_FUSION"}
        if value is not None:
            env["MVDETR_TRUNK_FUSION"] = value
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert f"ENABLED {want}" in out.stdout, out.stdout + out.stderr


def test_c_entry_points_refuse_bad_arguments_without_launching():
    from mvdetr_amd import _lib
    _lib.build()
    lib = _lib.lib()
    before = lib.mvdetr_trunk_launch_count()
    a = 4096                                               # (a 16-byte aligned non-null address; nothing dereferences it)
    bad = [
        lib.mvdetr_bn_act_f32(0, 0, a, a, a, a, 1e-5, 0, 0, 0, 0, 0, 0.0, 8, 64, 1, a),          # x null
        lib.mvdetr_bn_act_f32(0, a, a, a, a, a, 1e-5, 0, 0, 0, 0, 0, 0.0, 8, 62, 1, a),          # C % 4
        lib.mvdetr_bn_act_f32(0, a, 0, a, a, a, 1e-5, 0, 0, 0, 0, 0, 0.0, 8, 64, 1, a),          # no running mean
        lib.mvdetr_bn_act_f32(0, a, a, a, a, a, 1e-5, 0, a, a, 0, 0, 1e-5, 8, 64, 1, a),         # residual BN without residual
        lib.mvdetr_bn_act_f32(0, a, a, a, a, a, 1e-5, a + 16, 0, 0, 0, 0, 0.0, 8, 64, 1, a + 16),  # residual is the output
        lib.mvdetr_bn_act_f32(0, a + 4, a, a, a, a, 1e-5, 0, 0, 0, 0, 0, 0.0, 8, 64, 1, a),      # misaligned
        lib.mvdetr_bn_act_f32(0, a, a, a, a, a, 1e-5, 0, 0, 0, 0, 0, 0.0, -1, 64, 1, a),         # rows < 0
        lib.mvdetr_bn_relu_maxpool_f32(0, a, a, a, a, a, 1e-5, 1, 8, 8, 64, a),                  # in place
        lib.mvdetr_bn_relu_maxpool_f32(0, a, a, a, a, a, 1e-5, 1, 0, 8, 64, a + 16),             # empty image
        lib.mvdetr_bn_relu_maxpool_f32(0, a, a, a, a, a, 1e-5, 1, 8, 8, 96, a + 16),             # C/4 = 24 does not tile 256
    ]
    assert all(rc != 0 for rc in bad), bad
    assert lib.mvdetr_bn_act_f32(0, a, a, a, a, a, 1e-5, 0, 0, 0, 0, 0, 0.0, 0, 64, 1, a) == 0   # nothing to do
    assert lib.mvdetr_trunk_launch_count() == before
    with pytest.raises(RuntimeError):
        _lib.check(bad[0], "bn_act")
