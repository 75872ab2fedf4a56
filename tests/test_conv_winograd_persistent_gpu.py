"""The Winograd convolution's persistent grid (mvdetr_amd/csrc/conv_winograd.hip): a workgroup that runs SEVERAL units of
64 tiles x 64 output channels, the next unit's first chunks staged while the one before it is stored.

The exact suite (test_conv_winograd_exact_gpu.py) has fewer units than CUs in every case, so there each workgroup runs one
unit.  Here set_winograd_max_workgroups() caps the grid, so that small shapes run many units per workgroup: a cap that is
no multiple of the channel blocks (the channel block changes between a workgroup's units), one, two and an odd number of
chunks per unit (with one, the staging side is two units ahead), units that change image inside and between blocks.  One
case has more units than the device has CUs and runs uncapped, as the workload does.

Integer inputs on which float32 F(2x2,3x3) is exact (conv_winograd_oracle.integer_case) against the fp64 direct
convolution with torch.equal, x, U and y each inside a NaN-filled allocation; the fused stores against the uncapped run
and against the plain capped kernel followed by bn_act."""
import functools
import math

import pytest
import torch
from torch import nn

import conv_winograd_oracle as oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 1024                                      # floats of NaN on either side, at the least
SHAPE = (5, 192, 16, 16)                        # N, K, H, W: at d 1, 5 tile blocks x 3 channel blocks = 15 units


@pytest.fixture(scope="module")
def cw():
    from mvdetr_amd.ops import conv_winograd
    return conv_winograd


@pytest.fixture(scope="module")
def te():
    from mvdetr_amd.ops import trunk_epilogue
    return trunk_epilogue


@pytest.fixture(autouse=True)
def _no_cap_left_behind(cw):
    yield
    cw.set_winograd_max_workgroups(0)


@functools.lru_cache(maxsize=None)
def _exact_case(N, C, K, H, W, d):
    """(x, w, the fp64 direct convolution) on the CPU, computed once and never written."""
    x, w = oracle.integer_case(N, C, K, H, W, d)
    want = oracle.direct_fp64(x, w, d)
    oracle.check_sanity(want, C)
    return x, w, want


def _guarded(flat, pad):
    """A copy of the 1-d tensor ``flat`` on the device between two pads of NaN: (the whole buffer, the view of the copy)."""
    pad = (max(pad, PAD) + 3) // 4 * 4                                        # 16 bytes: the copy keeps the alignment
    buf = torch.full((flat.numel() + 2 * pad,), float("nan"), device=DEV)
    inner = buf[pad:pad + flat.numel()]
    inner.copy_(flat)
    assert inner.data_ptr() % 16 == 0
    return buf, inner, pad


def _check_raw(cw, N, C, K, H, W, d, caps):
    """The C entry under every cap of ``caps`` (0: none) on the same guarded x and U, a fresh guarded y per cap."""
    from mvdetr_amd import _lib
    x, w, want = _exact_case(N, C, K, H, W, d)
    reach = (d * W + d) * C                                                   # further than any out-of-image tap
    x_flat = x.permute(0, 2, 3, 1).reshape(-1)                                # NHWC, the memory order of channels-last
    U_flat = torch.from_numpy(oracle.transformed_weights(w.numpy())).reshape(-1)
    xbuf, xin, xpad = _guarded(x_flat, reach)
    Ubuf, Uin, Upad = _guarded(U_flat, reach)
    for cap in caps:
        ybuf = torch.full((N * H * W * K + 2 * PAD,), float("nan"), device=DEV)
        y = ybuf[PAD:PAD + N * H * W * K]
        before = cw.launch_count()
        cw.set_winograd_max_workgroups(cap)
        try:
            code = _lib.lib().mvdetr_conv3x3_winograd_f32(xin.data_ptr(), Uin.data_ptr(), y.data_ptr(), N, H, W, C, K, d,
                                                          _lib.current_stream_ptr(torch.device(DEV)))
        finally:
            assert cw.set_winograd_max_workgroups(0) == cap
        assert code == 0 and cw.launch_count() == before + 1 and cw.last_kernel() == "conv3x3_winograd_f32"
        name = f"N {N} C {C} K {K} {H}x{W} d {d} cap {cap}"
        ybuf = ybuf.cpu()
        got = ybuf[PAD:-PAD].view(N, H, W, K).permute(0, 3, 1, 2)
        assert torch.isnan(ybuf[:PAD]).all() and torch.isnan(ybuf[-PAD:]).all(), name + ": a store outside y"
        assert not torch.isnan(got).any(), name + f": {int(torch.isnan(got).sum())} NaN in y (an element never stored, or a tap outside x read)"
        assert torch.equal(got.double(), want), name + ": " + oracle.first_mismatch(got, want, d)
    xbuf, Ubuf = xbuf.cpu(), Ubuf.cpu()
    assert torch.equal(xbuf[xpad:-xpad], x_flat) and torch.isnan(xbuf[:xpad]).all() and torch.isnan(xbuf[-xpad:]).all()
    assert torch.equal(Ubuf[Upad:-Upad], U_flat) and torch.isnan(Ubuf[:Upad]).all() and torch.isnan(Ubuf[-Upad:]).all()


@pytest.mark.parametrize("C", [8, 16, 24])
@pytest.mark.parametrize("d", [1, 2, 4])
def test_many_units_per_workgroup_are_exact(cw, d, C):
    """Caps 1, 2, 3 and 7 (7 is no multiple of the 3 channel blocks); one, two and three chunks per unit."""
    N, K, H, W = SHAPE
    _check_raw(cw, N, C, K, H, W, d, (1, 2, 3, 7))


@pytest.mark.parametrize("cap", [1, 3])
def test_boundary_grid_under_caps(cw, cap):
    assert len(oracle.BOUNDARY_GRID) == 9
    for case in oracle.BOUNDARY_GRID:
        _check_raw(cw, *case, (cap,))


def test_default_grid_with_more_units_than_cus(cw):
    """Uncapped, as the workload runs: a few workgroups get a second unit."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    th = math.isqrt(64 * cus) + 2                                             # 130 on 256 CUs: 260 x 260, 265 units
    units = (th * th + 63) // 64
    assert cus < units < 2 * cus
    _check_raw(cw, 1, 8, 64, 2 * th, 2 * th, 1, (0,))


def _bn(K, g):
    bn = nn.BatchNorm2d(K)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(K, generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(K, generator=g) + 0.5)
        bn.weight.copy_(torch.randn(K, generator=g))                          # both signs
        bn.bias.copy_(torch.randn(K, generator=g) * 0.3)
    return bn.to(DEV).eval()


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("mode", ["bn", "bn_add", "bn_bn_add"])
def test_fused_stores_under_caps(cw, te, mode, relu):
    """float32 normal inputs, C 24: the capped runs have the bits of the uncapped one and of the plain capped kernel
    followed by bn_act in place; the residual is only read."""
    N, K, H, W = SHAPE
    C, d = 24, 1
    g = torch.Generator().manual_seed(17 + len(mode) + int(relu))
    conv = nn.Conv2d(C, K, 3, 1, d, d, bias=False)
    with torch.no_grad():
        conv.weight.normal_(0, (2.0 / (C * 9)) ** 0.5, generator=g)
    conv = conv.to(DEV).eval()
    x = torch.randn(N, C, H, W, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    bn = _bn(K, g)
    residual = residual_bn = None
    if mode != "bn":
        residual = torch.randn(N, K, H, W, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    if mode == "bn_bn_add":
        residual_bn = _bn(K, g)
    res_keep = None if residual is None else residual.clone(memory_format=torch.preserve_format)
    with torch.no_grad():
        uncapped = cw.winograd_conv3x3_bn_act(x, conv, bn, residual, residual_bn, relu=relu, force=True)
        assert cw.last_epilogue() == mode + ("_relu" if relu else "")
        assert not torch.isnan(uncapped).any() and (uncapped > 0).any() and (relu or (uncapped < 0).any())
        for cap in (1, 3):
            cw.set_winograd_max_workgroups(cap)
            try:
                got = cw.winograd_conv3x3_bn_act(x, conv, bn, residual, residual_bn, relu=relu, force=True)
                plain = cw.winograd_conv3x3(x, conv, force=True)
            finally:
                assert cw.set_winograd_max_workgroups(0) == cap
            two_launch = te.bn_act(plain, bn, residual, residual_bn, relu=relu, inplace=True)
            assert torch.equal(got, uncapped), f"{mode} relu {relu} cap {cap}: differs from the uncapped run"
            assert torch.equal(got, two_launch), f"{mode} relu {relu} cap {cap}: differs from conv + bn_act"
            if residual is not None:
                assert torch.equal(residual, res_keep)


def test_the_hook_returns_the_previous_cap(cw):
    assert cw.set_winograd_max_workgroups(0) == 0                             # the default, and nothing left it capped
    assert cw.set_winograd_max_workgroups(5) == 0
    assert cw.set_winograd_max_workgroups(2) == 5
    assert cw.set_winograd_max_workgroups(-3) == 2                            # below one: no cap
    assert cw.set_winograd_max_workgroups(0) == 0
    _check_raw(cw, 4, 8, 64, 8, 8, 1, (0,))                                   # and the default grid runs
