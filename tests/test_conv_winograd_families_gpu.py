"""The layer1/2 families of the Winograd convolution (64 -> 64 and 128 -> 128, mvdetr_amd/ops/conv_winograd.py's
NARROW_FAMILIES) and the kernel's unit entry and store (mvdetr_amd/csrc/conv_winograd.hip): a workgroup's next unit is found
by addition over the tile grid, with or without a carry of the channel block, and the outputs go out as buffer stores
whose offsets come from a per-tile descriptor.

Exact integer inputs (conv_winograd_oracle.integer_case) against the fp64 direct convolution with torch.equal, x, U and y
each inside a NaN-filled allocation, under workgroup caps 1 and 3 and the default: with K = 128 a cap of 1 or 3 is no multiple
of the two channel blocks, so the channel block wraps on every second unit (both strides of the entry), with K = 64 it never
does.  The same for one shape of each family of the first table.  Then every epilogue the trunk runs behind the new
convolutions against the two-launch form, and the launch counts of a BasicBlock of either width."""
import functools

import pytest
import torch
from torch import nn

import conv_winograd_oracle as oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 1024                                      # floats of NaN on either side, at the least
SIZES = [(2, 2), (5, 7), (6, 10), (9, 65)]      # one tile; odd; even; 5 x 33 tiles an image: blocks that span images, and with
                                                # N 1 a last block of 37 tiles
CAPS = (1, 3, 0)


@pytest.fixture(scope="module")
def cw():
    from mvdetr_amd.ops import conv_winograd
    return conv_winograd


@pytest.fixture(scope="module")
def te():
    from mvdetr_amd.ops import trunk_epilogue
    return trunk_epilogue


@pytest.fixture(autouse=True)
def _nothing_left_behind(cw):
    yield
    cw.set_winograd_max_workgroups(0)


@functools.lru_cache(maxsize=None)
def _exact_case(N, C, K, H, W, d):
    """(x, w, the fp64 direct convolution) on the CPU, computed once and never written."""
    x, w = oracle.integer_case(N, C, K, H, W, d)
    want = oracle.direct_fp64(x, w, d)
    if N * H * W > 4:
        oracle.check_sanity(want, C)
    else:
        assert (want != 0).any()
    return x, w, want


def _guarded(flat, pad):
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


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("C,K", [(64, 64), (128, 128)])
def test_new_families_are_exact_under_caps(cw, C, K, N):
    assert cw.NARROW_FAMILIES[(C, K)] == (1,)
    for H, W in SIZES:
        _check_raw(cw, N, C, K, H, W, 1, CAPS)


@pytest.mark.parametrize("N,C,K,H,W,d", [(3, 128, 256, 5, 7, 1), (3, 256, 256, 6, 10, 2), (1, 256, 512, 9, 65, 2),
                                         (3, 512, 512, 5, 7, 4), (1, 512, 512, 6, 10, 1)])
def test_first_table_families_are_exact_under_caps(cw, N, C, K, H, W, d):
    """4 and 8 channel blocks: caps 1 and 3 wrap the channel block on some units and not on others."""
    assert d in cw.FAMILIES[(C, K)]
    _check_raw(cw, N, C, K, H, W, d, CAPS)


def _bn(K, g):
    bn = nn.BatchNorm2d(K)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(K, generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(K, generator=g) + 0.5)
        bn.weight.copy_(torch.randn(K, generator=g))                          # both signs
        bn.bias.copy_(torch.randn(K, generator=g) * 0.3)
    return bn.to(DEV).eval()


@pytest.mark.parametrize("mode", ["bn", "bn_add", "bn_bn_add"])
@pytest.mark.parametrize("shape", [(2, 64, 6, 10), (2, 128, 5, 7)])
def test_trunk_epilogues_in_the_store_are_the_two_launch_form(cw, te, shape, mode):
    """bn_relu, bn_add_relu and bn_bn_add_relu on random inputs: the bits of winograd_conv3x3 + bn_act in place, under the
    default grid and under caps 1 and 3; the residual is only read."""
    N, K, H, W = shape
    g = torch.Generator().manual_seed(29 + K + len(mode))
    conv = nn.Conv2d(K, K, 3, 1, 1, bias=False)
    with torch.no_grad():
        conv.weight.normal_(0, (2.0 / (K * 9)) ** 0.5, generator=g)
    conv = conv.to(DEV).eval()
    x = torch.randn(N, K, H, W, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    bn = _bn(K, g)
    residual = residual_bn = None
    if mode != "bn":
        residual = torch.randn(N, K, H, W, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    if mode == "bn_bn_add":
        residual_bn = _bn(K, g)
    res_keep = None if residual is None else residual.clone(memory_format=torch.preserve_format)
    with torch.no_grad():
        want = te.bn_act(cw.winograd_conv3x3(x, conv, force=True), bn, residual, residual_bn, relu=True, inplace=True)
        assert not torch.isnan(want).any() and (want > 0).any() and (want == 0).any()
        for cap in CAPS:
            cw.set_winograd_max_workgroups(cap)
            try:
                before, passes = cw.launch_count(), te.launch_count()
                got = cw.winograd_conv3x3_bn_act(x, conv, bn, residual, residual_bn, relu=True, force=True)
                assert cw.launch_count() == before + 1 and te.launch_count() == passes
            finally:
                assert cw.set_winograd_max_workgroups(0) == cap
            assert cw.last_epilogue() == mode + "_relu"
            assert torch.equal(got, want), f"{shape} {mode} cap {cap}: differs from conv + bn_act"
            if residual is not None:
                assert torch.equal(residual, res_keep)


class _NoFloors:
    """Both pixel floors at 0, MIOpen's deterministic solvers off (the kernel's condition)."""
    def __init__(self, cw):
        self.cw = cw

    def __enter__(self):
        self.prev = self.cw.set_winograd_min_pixels(0)
        self.narrow = self.cw.set_winograd_narrow_min_pixels(0)
        self.det = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = False

    def __exit__(self, *exc):
        torch.backends.cudnn.deterministic = self.det
        self.cw.set_winograd_narrow_min_pixels(self.narrow)
        self.cw.set_winograd_min_pixels(self.prev)


@pytest.mark.parametrize("downsample", [False, True])
@pytest.mark.parametrize("planes", [64, 128])
def test_basic_block_is_two_winograd_launches_and_no_pass(cw, te, planes, downsample):
    """BasicBlock(planes, planes) at floor 0: conv1 with BatchNorm + ReLU in its store, conv2 with BatchNorm + residual +
    ReLU -- the residual through the downsample's BatchNorm where there is one (layer2.0's conv2) -- and no bn_act launch."""
    from mvdetr_amd.model import BasicBlock
    torch.manual_seed(planes)
    ds = nn.Sequential(nn.Conv2d(planes, planes, 1, bias=False), nn.BatchNorm2d(planes)) if downsample else None
    block = BasicBlock(planes, planes, downsample=ds)
    g = torch.Generator().manual_seed(planes + 1)
    with torch.no_grad():
        for m in block.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    block = block.to(DEV).eval()
    x = torch.randn(2, planes, 6, 10, generator=g).relu_().to(DEV).contiguous(memory_format=torch.channels_last)
    x_keep = x.clone(memory_format=torch.preserve_format)
    with torch.no_grad(), _NoFloors(cw):
        block(x)                                                              # (builds the transformed weights)
        before, passes = cw.launch_count(), te.launch_count()
        on = block(x)
        assert cw.launch_count() == before + 2 and te.launch_count() == passes
        assert cw.last_kernel() == "conv3x3_winograd_f32"
        assert cw.last_epilogue() == ("bn_bn_add_relu" if downsample else "bn_add_relu")
        if not downsample:
            # the same block by hand, the plain kernel and bn_act in place (with a downsample torch's 1x1 convolution is
            # in the block, and MIOpen's default solvers are not reproducible call to call)
            mid = te.bn_act(cw.winograd_conv3x3(x, block.conv1), block.bn1, relu=True, inplace=True)
            want = te.bn_act(cw.winograd_conv3x3(mid, block.conv2), block.bn2, x, None, relu=True, inplace=True)
    # at the default floors this input keeps torch's convolutions
    with torch.no_grad():
        before = cw.launch_count()
        block(x)
        assert cw.launch_count() == before
    assert torch.equal(x, x_keep) and on.abs().max().item() > 0 and (on == 0).any()
    if not downsample:
        assert torch.equal(on, want)
