"""CPU-only checks of the Winograd convolution's fused epilogue (mvdetr_amd/ops/conv_winograd.py): the predicate's
refusals and switches, asked about meta tensors standing in for device ones as in test_conv_winograd.py, and the C ABI's
new symbols.  No kernel is launched."""
import os
import re

import pytest
import torch
from torch import nn

from mvdetr_amd import _lib
from mvdetr_amd.ops import conv_winograd as cw
from mvdetr_amd.ops import trunk_epilogue as te

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def on_device(monkeypatch):
    """Meta tensors count as device tensors; one family on, every switch on, cudnn.deterministic off."""
    meta = lambda t: t.device.type == "meta"                                  # noqa: E731
    monkeypatch.setattr(cw, "_on_device", meta)
    monkeypatch.setattr(te, "_on_device", meta)
    monkeypatch.setattr(cw, "FAMILIES", {(64, 128): (1, 2)})
    monkeypatch.setattr(cw, "_enabled", True)
    monkeypatch.setattr(cw, "_epilogue", True)
    monkeypatch.setattr(te, "_enabled", True)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", False)


def _x(C=64, H=64, W=128, N=1, dtype=torch.float32):
    return torch.empty(N, C, H, W, dtype=dtype, device="meta").contiguous(memory_format=torch.channels_last)


def _conv(C=64, K=128, d=1):
    return nn.Conv2d(C, K, 3, 1, d, d, bias=False, device="meta").requires_grad_(False).eval()


def _bn(K=128, **kw):
    return nn.BatchNorm2d(K, device="meta", **kw).requires_grad_(False).eval()


def test_predicate_truth_table(on_device):
    ok = cw.winograd_conv3x3_bn_act_available
    x, conv, res = _x(), _conv(), _x(128)
    with torch.no_grad():
        assert ok(x, conv, _bn()) and ok(x, conv, _bn(), res) and ok(x, conv, _bn(), res, _bn())
        assert ok(x, conv, _bn(affine=False)) and ok(x, _conv(d=2), _bn(), res)
        # the convolution's own conditions
        assert not ok(x, _conv(d=4), _bn()) and not ok(_x(128), _conv(128, 128), _bn())
        assert not ok(_x(dtype=torch.float16), conv, _bn()) and not ok(_x(dtype=torch.bfloat16), conv, _bn(), res.bfloat16())
        # the BatchNorm's
        assert not ok(x, conv, _bn().train())
        assert not ok(x, conv, _bn(64))                                       # the input's channels, not the output's
        assert not ok(x, conv, _bn(track_running_stats=False))
        assert not ok(x, conv, nn.Identity()) and not ok(x, conv, nn.SyncBatchNorm(128, device="meta").eval())
        assert not ok(x, conv, _bn().double())
        assert not ok(x, conv, _bn(), res, _bn().train()) and not ok(x, conv, _bn(), res, _bn(64))
        assert not ok(x, conv, _bn(), None, _bn())                            # a residual BatchNorm without a residual
        # the residual's: shape, layout, dtype, device
        assert not ok(x, conv, _bn(), _x(64)) and not ok(x, conv, _bn(), _x(128, H=32)) and not ok(x, conv, _bn(), _x(128, N=2))
        assert not ok(x, conv, _bn(), res.contiguous())                       # NCHW
        assert not ok(x, conv, _bn(), _x(128, W=256)[..., ::2])               # a strided view
        assert not ok(x, conv, _bn(), res.double()) and not ok(x, conv, _bn(), res.half())
        assert not ok(x, conv, _bn(), torch.empty(1, 128, 64, 128).contiguous(memory_format=torch.channels_last))     # CPU


def test_predicate_refuses_what_needs_autograd(on_device):
    ok = cw.winograd_conv3x3_bn_act_available
    x, conv, res = _x(), _conv(), _x(128)
    with torch.enable_grad():
        assert ok(x, conv, _bn(), res, _bn())                                 # nothing requires grad
        assert not ok(x, conv, _bn().requires_grad_(True))
        assert not ok(x, conv, _bn(), _x(128).requires_grad_(True))
        assert not ok(x, conv, _bn(), res, _bn().requires_grad_(True))
        assert not ok(_x().requires_grad_(True), conv, _bn())
        assert not ok(x, _conv().requires_grad_(True), _bn())
    with torch.no_grad():
        assert ok(x, conv, _bn().requires_grad_(True), _x(128).requires_grad_(True), _bn().requires_grad_(True))


def test_predicate_switches(on_device):
    ok = cw.winograd_conv3x3_bn_act_available
    x, conv, bn, res = _x(), _conv(), _bn(), _x(128)
    with torch.no_grad():
        assert ok(x, conv, bn, res) and cw.winograd_epilogue_enabled()
        prev = cw.set_winograd_epilogue(False)
        assert prev is True and not ok(x, conv, bn, res) and not cw.winograd_epilogue_enabled()
        assert cw.winograd_conv3x3_available(x, conv)                          # the convolution itself is not switched off
        assert cw.set_winograd_epilogue(prev) is False and ok(x, conv, bn, res)
        prev = te.set_trunk_fusion(False)                                      # the epilogues are torch's ops then
        assert not ok(x, conv, bn, res) and cw.winograd_conv3x3_available(x, conv)
        te.set_trunk_fusion(prev)
        assert ok(x, conv, bn, res)
        prev = cw.set_trunk_winograd(False)
        assert not ok(x, conv, bn, res)
        cw.set_trunk_winograd(prev)
        torch.backends.cudnn.deterministic = True                             # (the fixture restores it)
        assert not ok(x, conv, bn, res)
        torch.backends.cudnn.deterministic = False
        assert not ok(_x(H=8, W=8), conv, bn, _x(128, H=8, W=8))              # below the pixel floor
        with pytest.raises(RuntimeError):                                      # the wrapper raises where the predicate is false
            cw.winograd_conv3x3_bn_act(_x(H=8, W=8), conv, bn, _x(128, H=8, W=8))


def test_the_factored_conditions_are_those_of_bn_act(on_device, monkeypatch):
    """fused_bn_act_available(y, ...) on an existing output and bn_act_conditions(...) on its shape agree; what the former
    adds is the overlap of y with the residual (every meta tensor sits at address 0, so that is asked last and alone)."""
    monkeypatch.setattr(te, "_overlap", lambda a, b: False)
    y, res = _x(128), _x(128)
    cases = [(_bn(), None, None), (_bn(), res, None), (_bn(), res, _bn()), (_bn().train(), None, None), (_bn(64), res, None),
             (_bn(), _x(64), None), (_bn(), res.contiguous(), None), (_bn(), res.double(), None), (_bn(), None, _bn()),
             (_bn(), res, _bn().train())]
    with torch.no_grad():
        for bn, r, rbn in cases:
            want = te.bn_act_conditions(tuple(y.shape), y.dtype, y.device, y.requires_grad, bn, r, rbn)
            assert te.fused_bn_act_available(y, bn, r, rbn) == want, (bn, r, rbn)
    monkeypatch.undo()
    monkeypatch.setattr(te, "_on_device", lambda t: t.device.type == "meta")
    assert te._overlap(y, res) and not te.fused_bn_act_available(y, _bn(), res)


def test_the_environment_switch():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from mvdetr_amd.ops import conv_winograd as cw\n"
            "print('EPILOGUE', cw.winograd_epilogue_enabled(), cw.trunk_winograd_enabled())\n") % ROOT
    for value, want in (("0", "EPILOGUE False True"), ("1", "EPILOGUE True True")):
        env = dict(os.environ, MVDETR_WINOGRAD_EPILOGUE=value, MVDETR_TRUNK_WINOGRAD="1")
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert want in out.stdout, out.stdout + out.stderr


def test_the_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "mvdetr_ops.h")).read()
    assert re.search(r"#define\s+MVDETR_OPS_ABI_VERSION\s+18\b", header) and _lib.ABI_VERSION == 18
    for name in ("mvdetr_conv3x3_winograd_bn_act_f32", "mvdetr_winograd_last_epilogue"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
    argtypes, restype = _lib.SIGNATURES["mvdetr_conv3x3_winograd_bn_act_f32"]
    conv_args = _lib.SIGNATURES["mvdetr_conv3x3_winograd_f32"][0]
    bn_args = _lib.SIGNATURES["mvdetr_bn_act_f32"][0]
    # the convolution's arguments, then mvdetr_bn_act_f32's from mean to res_eps, then relu and the stream
    assert argtypes == conv_args[:-1] + bn_args[2:13] + [bn_args[15], conv_args[-1]] and restype is _lib._i
    lib = _lib.lib()                                                           # loads the library and checks every symbol
    assert lib.mvdetr_ops_abi_version() == 18
    assert lib.mvdetr_winograd_last_epilogue() in (b"none", b"bn", b"bn_relu", b"bn_add", b"bn_add_relu", b"bn_bn_add",
                                                   b"bn_bn_add_relu")
