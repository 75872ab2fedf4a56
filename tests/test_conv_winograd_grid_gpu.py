"""The Winograd convolution's tile grid and LDS image of V (mvdetr_amd/csrc/conv_winograd.hip).

Every sub-lattice of a dilated convolution has its own tile grid: an image's tiles are one TY x TX grid, the sub-lattice rows
stacked along Y and the sub-lattice columns along X.  Here: grids that differ between the sub-lattices in both axes, empty
sub-lattices, and units of 64 tiles that straddle sub-lattices and images, each under caps of the persistent grid (0: none);
every slot of the chunk's V image (64 and 65 tiles; one, two and three chunks); the fused stores on an unequal grid.

Integer inputs on which float32 F(2x2,3x3) is exact (conv_winograd_oracle.integer_case) against the fp64 direct
convolution with torch.equal, x, U and y each inside a NaN-filled allocation."""
import functools

import pytest
import torch
from torch import nn

import conv_winograd_oracle as oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 1024                                      # floats of NaN on either side, at the least


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


def _tile_rows(extent, d):
    """Tile rows of each sub-lattice row of an axis of ``extent`` pixels: ceil(rows / 2), none where the extent is <= sy."""
    return [(-(-(extent - s) // d) + 1) // 2 if s < extent else 0 for s in range(d)]


UNEQUAL_GRIDS = [
    (5, 16, 128, 9, 10, 4),       # tile rows 2 1 1 1 and columns 2 2 1 1: 30 tiles an image, units straddle both
    (5, 8, 64, 5, 7, 2),          # rows 2 1, columns 2 2: 12 tiles an image, one unit of 60
    (3, 24, 64, 2, 9, 4),         # sub-lattice rows 2 and 3 are empty
    (70, 8, 64, 1, 3, 4),         # one sub-lattice row, three of four columns: 3 tiles an image, 64 tiles span 22 images
]


@pytest.mark.parametrize("case", UNEQUAL_GRIDS, ids=lambda c: "x".join(map(str, c)))
def test_unequal_sublattice_grids_are_exact(cw, case):
    N, C, K, H, W, d = case
    ty, tx = _tile_rows(H, d), _tile_rows(W, d)
    assert len(set(ty)) > 1 or len(set(tx)) > 1                               # the grids do differ
    assert N > 1 and sum(ty) * sum(tx) % 64 != 0                              # a unit's 64 tiles are not whole images
    _check_raw(cw, N, C, K, H, W, d, (0, 1, 3))


@pytest.mark.parametrize("C", [8, 16, 24])
@pytest.mark.parametrize("shape", [(4, 64, 8, 8), (5, 64, 2, 26)], ids=["64_tiles", "65_tiles"])
def test_every_slot_of_v(cw, shape, C):
    """All 64 tiles x 8 channels x 16 positions of the chunk's V image carry their own integers (seeded, in [-3, 3]): a
    swapped slot or a wrong column changes the integers of the result.  One, two and three chunks."""
    N, K, H, W = shape
    x, _, want = _exact_case(N, C, K, H, W, 1)
    oracle.check_sanity(want, C)
    tiles = x.unfold(2, 2, 2).unfold(3, 2, 2).permute(0, 2, 3, 1, 4, 5).reshape(-1, 4)   # the 2 x 2 cores, (tile, channel)
    assert len({tuple(t) for t in tiles.tolist()}) > 200                      # (7^4 patterns: no two slots need differ, most do)
    _check_raw(cw, N, C, K, H, W, 1, (0,))


def _bn(K, g):
    bn = nn.BatchNorm2d(K)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(K, generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(K, generator=g) + 0.5)
        bn.weight.copy_(torch.randn(K, generator=g))                          # both signs
        bn.bias.copy_(torch.randn(K, generator=g) * 0.3)
    return bn.to(DEV).eval()


@pytest.mark.parametrize("mode", ["bn_add", "bn_bn_add"])
def test_fused_stores_on_an_unequal_grid(cw, te, mode):
    """float32 normal inputs, ReLU on: the fused store has the bits of the plain kernel followed by bn_act in place."""
    N, C, K, H, W, d = 3, 24, 128, 9, 10, 4
    g = torch.Generator().manual_seed(23 + len(mode))
    conv = nn.Conv2d(C, K, 3, 1, d, d, bias=False)
    with torch.no_grad():
        conv.weight.normal_(0, (2.0 / (C * 9)) ** 0.5, generator=g)
    conv = conv.to(DEV).eval()
    x = torch.randn(N, C, H, W, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    bn = _bn(K, g)
    residual = torch.randn(N, K, H, W, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    residual_bn = _bn(K, g) if mode == "bn_bn_add" else None
    res_keep = residual.clone(memory_format=torch.preserve_format)
    with torch.no_grad():
        got = cw.winograd_conv3x3_bn_act(x, conv, bn, residual, residual_bn, relu=True, force=True)
        assert cw.last_epilogue() == mode + "_relu"
        assert not torch.isnan(got).any() and (got > 0).any()
        plain = cw.winograd_conv3x3(x, conv, force=True)
        two_launch = te.bn_act(plain, bn, residual, residual_bn, relu=True, inplace=True)
    assert torch.equal(got, two_launch), f"{mode}: differs from conv + bn_act"
    assert torch.equal(residual, res_keep)
