"""The fp32 Winograd F(2x2,3x3) MFMA convolution (mvdetr_amd/csrc/conv_winograd.hip) held to the fp64 direct convolution BIT
FOR BIT, over every geometry edge of the kernel.

On integer activations in [-3, 3] and weights that are integer multiples of 4 in [-8, 8] every intermediate of float32
F(2x2,3x3) is an integer below 2^24 (conv_winograd_oracle.integer_case asserts the bound from the arrays), so there is no
rounding anywhere and no tolerance here: a wrong index, mask, flag or layout shows as a wrong integer.  The CPU suite
(test_conv_winograd.py) checks the same on the float32 emulation, and that every case's reference is non-trivial.

Every case calls the C entry with x, U and y each inside a NaN-filled allocation of its own: y between two pads (a store
outside y lands on a pad), x and U between pads wider than any out-of-image tap could reach ((d W + d) C floats), so a tap
outside the image that is read at its true address and multiplied by zero, not replaced and selected, puts a NaN into y
wherever that address lies outside x.  All reads and writes stay inside one allocation each.

Grids (conv_winograd_oracle.py): geometry -- C 24 (an odd chunk count), K 64, N 3, H and W every pair of {1, 2, 3, 4, 5, 9},
d in {1, 2, 4}: extents smaller than the dilation (empty sub-lattices, tiles whose origin is outside the image), single rows
and columns, odd and even edges, sub-lattices of unequal size; channels -- 9 x 13, C in {8, 16, 24, 40, 72, 256} (one chunk,
odd and even chunk counts) and K in {64, 128, 192}; batch and tile-block boundaries -- 64 tiles spanning 64 images, exactly
64 and 65 tiles, tiles past the end, tile rows outside the image.  The last grid also goes through winograd_conv3x3()."""
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


@functools.lru_cache(maxsize=None)
def _exact_case(N, C, K, H, W, d):
    """(x, w, the fp64 direct convolution, its non-zero share) on the CPU, computed once and never written."""
    x, w = oracle.integer_case(N, C, K, H, W, d)
    want = oracle.direct_fp64(x, w, d)
    return x, w, want, oracle.check_sanity(want, C)


def _guarded(flat, pad):
    """A copy of the 1-d tensor ``flat`` on the device between two pads of NaN: (the whole buffer, the view of the copy)."""
    pad = (max(pad, PAD) + 3) // 4 * 4                                        # 16 bytes: the copy keeps the alignment
    buf = torch.full((flat.numel() + 2 * pad,), float("nan"), device=DEV)
    inner = buf[pad:pad + flat.numel()]
    inner.copy_(flat)
    assert inner.data_ptr() % 16 == 0
    return buf, inner, pad


def _check_raw(cw, N, C, K, H, W, d):
    from mvdetr_amd import _lib
    x, w, want, _ = _exact_case(N, C, K, H, W, d)
    reach = (d * W + d) * C                                                   # further than any out-of-image tap
    x_flat = x.permute(0, 2, 3, 1).reshape(-1)                                # NHWC, the memory order of channels-last
    U_flat = torch.from_numpy(oracle.transformed_weights(w.numpy())).reshape(-1)
    xbuf, xin, xpad = _guarded(x_flat, reach)
    Ubuf, Uin, Upad = _guarded(U_flat, reach)
    ybuf = torch.full((N * H * W * K + 2 * PAD,), float("nan"), device=DEV)
    y = ybuf[PAD:PAD + N * H * W * K]
    before = cw.launch_count()
    code = _lib.lib().mvdetr_conv3x3_winograd_f32(xin.data_ptr(), Uin.data_ptr(), y.data_ptr(), N, H, W, C, K, d,
                                                  _lib.current_stream_ptr(torch.device(DEV)))
    assert code == 0 and cw.launch_count() == before + 1 and cw.last_kernel() == "conv3x3_winograd_f32"
    name = f"N {N} C {C} K {K} {H}x{W} d {d}"
    ybuf, xbuf, Ubuf = ybuf.cpu(), xbuf.cpu(), Ubuf.cpu()
    got = ybuf[PAD:-PAD].view(N, H, W, K).permute(0, 3, 1, 2)
    assert torch.isnan(ybuf[:PAD]).all() and torch.isnan(ybuf[-PAD:]).all(), name + ": a store outside y"
    assert not torch.isnan(got).any(), name + f": {int(torch.isnan(got).sum())} NaN in y (an element never stored, or a tap outside x read)"
    assert torch.equal(got.double(), want), name + ": " + oracle.first_mismatch(got, want, d)
    assert torch.equal(xbuf[xpad:-xpad], x_flat) and torch.isnan(xbuf[:xpad]).all() and torch.isnan(xbuf[-xpad:]).all(), name
    assert torch.equal(Ubuf[Upad:-Upad], U_flat) and torch.isnan(Ubuf[:Upad]).all() and torch.isnan(Ubuf[-Upad:]).all(), name


def _check_grid(cw, cases):
    shares = []
    for case in cases:
        _check_raw(cw, *case)
        shares.append(_exact_case(*case)[3])
    print(f"{len(cases)} cases bit-equal to fp64; non-zero share of the references {min(shares):.3f} - {max(shares):.3f}")


@pytest.mark.parametrize("d", [1, 2, 4])
def test_geometry_grid_is_exact(cw, d):
    cases = [c for c in oracle.GEOMETRY_GRID if c[5] == d]
    assert len(cases) == 36
    _check_grid(cw, cases)


@pytest.mark.parametrize("d", [1, 2, 4])
def test_channel_grid_is_exact(cw, d):
    cases = [c for c in oracle.CHANNEL_GRID if c[5] == d]
    assert len(cases) == 18
    _check_grid(cw, cases)


def test_batch_and_tile_block_boundaries_are_exact(cw):
    assert len(oracle.BOUNDARY_GRID) == 9
    _check_grid(cw, oracle.BOUNDARY_GRID)


def test_boundary_grid_through_the_public_entry(cw):
    """The same bits from winograd_conv3x3(force=True): the device's own weight transform and torch's allocations."""
    for N, C, K, H, W, d in oracle.BOUNDARY_GRID:
        x, w, want, _ = _exact_case(N, C, K, H, W, d)
        conv = nn.Conv2d(C, K, 3, 1, d, d, bias=False)
        with torch.no_grad():
            conv.weight.copy_(w)
        conv = conv.to(DEV).eval()
        xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            before = cw.launch_count()
            got = cw.winograd_conv3x3(xd, conv, force=True)
            assert cw.launch_count() == before + 2 and cw.last_kernel() == "conv3x3_winograd_f32"     # weights, convolution
        assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
        got = got.cpu()
        assert torch.equal(got.double(), want), f"N {N} C {C} K {K} {H}x{W} d {d}: " + oracle.first_mismatch(got, want, d)
        assert torch.equal(xd.cpu(), x) and torch.equal(conv.weight.detach().cpu(), w)
