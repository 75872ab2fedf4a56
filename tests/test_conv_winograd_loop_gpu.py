"""The chunk loop of the fp32 Winograd F(2x2,3x3) MFMA convolution (mvdetr_amd/csrc/conv_winograd.hip), at the shapes where its
pacing can go wrong.

The loop reads the operands of the next k-step behind the MFMAs of the current one into two register sets (the reads behind
k-step 3 are the NEXT chunk's k-step 0, across the barrier), forms the next chunk's B^T d B in pieces between the MFMAs of
k-steps 1 and 2, and issues the loads of the chunk after it behind the barrier into the buffer the current chunk just left.
Pixels outside the image are buffer loads beyond the buffer's range (the hardware returns zero), and the tile column of V is
XOR-swizzled by the channel pair.  What can break is therefore: the prologue (chunk 0 staged, chunk 1 loaded, chunk 0's first
operands read), the buffer parity, the iterations past the last real chunk, which stage the last chunk again, a tap outside
the image that is read after all (x sits between NaN pads), and a tile or channel landing in the wrong column or row of V.

Exact cases: conv_winograd_oracle.integer_case against direct_fp64 with NO tolerance (every intermediate is an integer below
2^24), x, U and y each inside a NaN-filled allocation of its own:
  * C = 8, 16, 24, 72 -- one chunk (the loop body runs once, every load after the prologue is a restage), two chunks, odd and
    even chunk counts -- each with K = 64 and 192 (one and three k-blocks per tile block);
  * exactly 64, 65 and 127 tiles (one full workgroup; one tile in the second; one tile short of two);
  * a workgroup that spans three images (N = 5, 4 x 6: 6 tiles per image);
  * d = 1, 2, 4 with H and W from {1, 3, 9, 18}: extents below the dilation, odd edges, sub-lattices of unequal size.
The tile-to-workgroup mapping is the parent's (64 consecutive tiles), so there are no two-dimensional tile-block cases.

Rounding: the kernel against the float32 emulation (conv_winograd_oracle.emulate_f32) at C = 72, K = 128, d = 1 and 2, on
activations of both signs, within the existing 4 ulp of the largest output; the share of identical elements is printed (1.0000
on the kernel before the loop was re-paced, and after)."""
import functools

import numpy as np
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
    """(x, w, the fp64 direct convolution) on the CPU, computed once and never written."""
    x, w = oracle.integer_case(N, C, K, H, W, d)
    return x, w, oracle.direct_fp64(x, w, d)


def _guarded(flat, pad):
    pad = (max(pad, PAD) + 3) // 4 * 4                                        # 16 bytes: the copy keeps the alignment
    buf = torch.full((flat.numel() + 2 * pad,), float("nan"), device=DEV)
    inner = buf[pad:pad + flat.numel()]
    inner.copy_(flat)
    assert inner.data_ptr() % 16 == 0
    return buf, inner, pad


def _tiles(N, H, W, d):
    return N * d * d * (((H + d - 1) // d + 1) // 2) * (((W + d - 1) // d + 1) // 2)


def _check_exact(cw, N, C, K, H, W, d):
    from mvdetr_amd import _lib
    x, w, want = _exact_case(N, C, K, H, W, d)
    oracle.check_sanity(want, C)                                              # not an empty comparison
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
    name = f"N {N} C {C} K {K} {H}x{W} d {d} ({_tiles(N, H, W, d)} tiles, {C // 8} chunks)"
    ybuf, xbuf, Ubuf = ybuf.cpu(), xbuf.cpu(), Ubuf.cpu()
    got = ybuf[PAD:-PAD].view(N, H, W, K).permute(0, 3, 1, 2)
    assert torch.isnan(ybuf[:PAD]).all() and torch.isnan(ybuf[-PAD:]).all(), name + ": a store outside y"
    assert not torch.isnan(got).any(), name + f": {int(torch.isnan(got).sum())} NaN in y"
    assert torch.equal(got.double(), want), name + ": " + oracle.first_mismatch(got, want, d)
    assert torch.equal(xbuf[xpad:-xpad], x_flat) and torch.isnan(xbuf[:xpad]).all() and torch.isnan(xbuf[-xpad:]).all(), name
    assert torch.equal(Ubuf[Upad:-Upad], U_flat) and torch.isnan(Ubuf[:Upad]).all() and torch.isnan(Ubuf[-Upad:]).all(), name
    return name


@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("C", [8, 16, 24, 72])
def test_chunk_counts_are_exact(cw, C, K):
    """One, two, three and nine chunks: the prologue alone, the first buffer swap, odd and even parity at the last chunk.
    2 x 9 x 13 is 70 tiles: a full workgroup and a partial one."""
    for d in (1, 2):
        print(_check_exact(cw, 2, C, K, 9, 13, d))


@pytest.mark.parametrize("N,H,W,tiles", [(4, 8, 8, 64), (5, 2, 26, 65), (1, 2, 254, 127)])
def test_tile_counts_at_the_workgroup_edge_are_exact(cw, N, H, W, tiles):
    assert _tiles(N, H, W, 1) == tiles
    for C in (8, 24):
        print(_check_exact(cw, N, C, 64, H, W, 1))


def test_a_workgroup_spanning_three_images_is_exact(cw):
    """N = 5, 4 x 6: 6 tiles per image at d = 1 (the one workgroup's 30 tiles are five images) and 8 at d = 2 (40 tiles)."""
    assert _tiles(5, 4, 6, 1) == 30 and _tiles(5, 4, 6, 2) == 5 * 4 * 1 * 2
    for C, K in ((16, 64), (72, 192)):
        for d in (1, 2):
            print(_check_exact(cw, 5, C, K, 4, 6, d))
    # 6 tiles per image at d = 1, batch 27: workgroup 0 holds images 0..10, workgroup 1 images 10..21, workgroup 2 the rest
    print(_check_exact(cw, 27, 16, 64, 4, 6, 1))


@pytest.mark.parametrize("d", [1, 2, 4])
def test_dilations_and_small_extents_are_exact(cw, d):
    for H in (1, 3, 9, 18):
        for W in (1, 3, 9, 18):
            _check_exact(cw, 3, 24, 64, H, W, d)
    print(f"d {d}: 16 extents bit-equal to fp64")


@pytest.mark.parametrize("d", [1, 2])
def test_rounding_is_the_float32_algorithm(cw, d):
    C, K, H, W = 72, 128, 9, 13
    g = torch.Generator().manual_seed(7 + d)
    conv = nn.Conv2d(C, K, 3, 1, d, d, bias=False)
    with torch.no_grad():
        conv.weight.normal_(0, (2.0 / (K * 9)) ** 0.5, generator=g)
    x = torch.randn(2, C, H, W, generator=g)                                  # both signs
    conv, xd = conv.to(DEV).eval(), x.to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        got = cw.winograd_conv3x3(xd, conv, force=True).cpu().numpy()
    emu = oracle.emulate_f32(x.numpy(), conv.weight.detach().cpu().numpy(), d)
    diff = np.abs(got.astype(np.float64) - emu).max()
    ulp = np.spacing(np.float32(np.abs(emu).max()))
    print(f"C {C} K {K} {H}x{W} d {d} mixed sign: kernel vs float32 emulation max {diff:.3e} = {diff / ulp:.2f} ulp of the largest "
          f"output, identical elements {(got == emu).mean():.4f}")
    assert got.shape == emu.shape and np.abs(emu).max() > 0 and (x < 0).any() and (x > 0).any()
    assert diff <= 4 * ulp
