"""The Winograd convolution on 16-channel wave blocks (v_mfma_f32_16x16x4_f32, mvdetr_amd/csrc/conv_winograd.hip): the
half-unit tail (conv3x3_winograd_w16_f32: the units of a launch's last round run as two workgroups of 32 tiles x 64 channels
each) and the 8-wave persistent kernel (conv3x3_winograd_w16x2_f32, variant 2: two waves per SIMD).

Exact: integer inputs on which float32 F(2x2,3x3) has no rounding (conv_winograd_oracle.integer_case) against the fp64
direct convolution with torch.equal, x, U and y each inside a NaN-filled allocation.  Every case runs under tail mode 2
(half units whenever a launch has a remainder) and several caps of the persistent grid; the shapes have three channel
blocks or three tile blocks and more, so that some cap leaves a remainder, and every case asserts that at least one of its
runs did launch the tail, and every run that its tail was what mvdetr_winograd_plan says.

Bit-identity: N(0, 1) inputs of both signs, all seven stores (plain; BatchNorm, + residual, + residual through a second
BatchNorm, each with and without ReLU) and null gamma / beta: tail mode 2 against tail mode 0 with torch.equal.  Both fp32
MFMAs are fused multiply-add chains in the order of the input channels, which is the same in both kernels.

Bit-identity of variant 2 (the 8-wave kernel) against variant 1 is checked in the same test, and every exact case runs under
variant 2 as well, with last_variant / last_tail_units asserted so that no case passes on another path.

A build whose half-unit kernel takes its tiles from a wrong offset (first tile computed with 16 instead of 32 tiles per half) was
run once against the tail tests of this file: 15 of 22 failed, among them every bit-identity test; the seven that passed have no
tail unit with more than 48 tiles, the only ones that build leaves unstored (docs/notes/conv_winograd.md)."""
import functools

import pytest
import torch
from torch import nn

import conv_winograd_oracle as oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 1024                                      # floats of NaN on either side, at the least
CAPS = (1, 2, 3, 7, 4, 5)                       # 3 units: cap 2 leaves one; 4: cap 3; 6: caps 4 and 5 leave G / 2 and one


@pytest.fixture(scope="module")
def cw():
    from mvdetr_amd.ops import conv_winograd
    return conv_winograd


@pytest.fixture(autouse=True)
def _defaults_afterwards(cw):
    yield
    cw.set_winograd_max_workgroups(0)
    cw.set_winograd_tail(1)
    cw.set_winograd_variant(0)


@functools.lru_cache(maxsize=None)
def _exact_case(N, C, K, H, W, d):
    """(x, w, the fp64 direct convolution) on the CPU, computed once and never written."""
    x, w = oracle.integer_case(N, C, K, H, W, d)
    want = oracle.direct_fp64(x, w, d)
    return x, w, want


def _guarded(flat, pad):
    pad = (max(pad, PAD) + 3) // 4 * 4                                        # 16 bytes: the copy keeps the alignment
    buf = torch.full((flat.numel() + 2 * pad,), float("nan"), device=DEV)
    inner = buf[pad:pad + flat.numel()]
    inner.copy_(flat)
    assert inner.data_ptr() % 16 == 0
    return buf, inner, pad


def _check_raw(cw, N, C, K, H, W, d, caps=CAPS, variant=1):
    """The C entry under every cap of ``caps`` on the same guarded x and U, a fresh guarded y per cap: variant 1 (the 4-wave
    persistent kernel) with tail mode 2, or variant 2 (the 8-wave one) without a tail.  Returns the tail units of each run."""
    from mvdetr_amd import _lib
    x, w, want = _exact_case(N, C, K, H, W, d)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reach = (d * W + d) * C                                                   # further than any out-of-image tap
    x_flat = x.permute(0, 2, 3, 1).reshape(-1)                                # NHWC, the memory order of channels-last
    U_flat = torch.from_numpy(oracle.transformed_weights(w.numpy())).reshape(-1)
    xbuf, xin, xpad = _guarded(x_flat, reach)
    Ubuf, Uin, Upad = _guarded(U_flat, reach)
    tails = []
    for cap in caps:
        ybuf = torch.full((N * H * W * K + 2 * PAD,), float("nan"), device=DEV)
        y = ybuf[PAD:PAD + N * H * W * K]
        before = cw.launch_count()
        cw.set_winograd_max_workgroups(cap)
        cw.set_winograd_tail(2 if variant == 1 else 0)
        cw.set_winograd_variant(variant)
        try:
            plan = cw.plan(N, H, W, C, K, d, cus)
            code = _lib.lib().mvdetr_conv3x3_winograd_f32(xin.data_ptr(), Uin.data_ptr(), y.data_ptr(), N, H, W, C, K, d,
                                                          _lib.current_stream_ptr(torch.device(DEV)))
        finally:
            assert cw.set_winograd_max_workgroups(0) == cap and cw.set_winograd_tail(1) == (2 if variant == 1 else 0)
            assert cw.set_winograd_variant(0) == variant
        name = f"N {N} C {C} K {K} {H}x{W} d {d} cap {cap} ({plan})"
        assert plan["variant"] == variant == cw.last_variant(), name
        assert code == 0 and cw.launch_count() == before + 1 and cw.last_kernel() == "conv3x3_winograd_f32", name
        tail = plan["rem"] if variant == 1 else 0
        assert plan["half_units"] == 2 * tail and cw.last_tail_units() == tail, name
        tails.append(tail)
        ybuf = ybuf.cpu()
        got = ybuf[PAD:-PAD].view(N, H, W, K).permute(0, 3, 1, 2)
        assert torch.isnan(ybuf[:PAD]).all() and torch.isnan(ybuf[-PAD:]).all(), name + ": a store outside y"
        assert not torch.isnan(got).any(), name + f": {int(torch.isnan(got).sum())} NaN in y (an element never stored, or a tap outside x read)"
        assert torch.equal(got.double(), want), name + ": " + oracle.first_mismatch(got, want, d)
    xbuf, Ubuf = xbuf.cpu(), Ubuf.cpu()
    assert torch.equal(xbuf[xpad:-xpad], x_flat) and torch.isnan(xbuf[:xpad]).all() and torch.isnan(xbuf[-xpad:]).all()
    assert torch.equal(Ubuf[Upad:-Upad], U_flat) and torch.isnan(Ubuf[:Upad]).all() and torch.isnan(Ubuf[-Upad:]).all()
    assert variant == 2 or any(tails), f"N {N} C {C} K {K} {H}x{W} d {d}: no cap of {caps} left a remainder, the tail never ran"
    return tails


@pytest.mark.parametrize("d", [1, 2, 4])
def test_geometry_grid_is_exact(cw, d):
    """H and W every pair of {1, 2, 3, 5, 9}, N 3, three chunks, three channel blocks: 3 or 6 units."""
    for H in (1, 2, 3, 5, 9):
        for W in (1, 2, 3, 5, 9):
            _check_raw(cw, 3, 24, 192, H, W, d, (2, 4, 5))
            _check_raw(cw, 3, 24, 192, H, W, d, (0, 2), variant=2)


@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("d", [1, 2, 4])
def test_channel_grid_is_exact(cw, d, K):
    """One, two, three and nine chunks; one and three channel blocks; 3 or 4 tile blocks."""
    for C in (8, 16, 24, 72):
        _check_raw(cw, 5, C, K, 9, 13, d, (1, 2, 3, 7))
        _check_raw(cw, 5, C, K, 9, 13, d, (1, 2, 3, 7), variant=2)


BOUNDARIES = [
    (2, 8, 192, 8, 8, 1),         # exactly 32 tiles: the second half of the only tile block is wholly past the last tile
    (3, 8, 192, 2, 22, 1),        # 33 tiles: the second half holds one
    (4, 8, 192, 8, 8, 1),         # exactly 64
    (5, 8, 192, 2, 26, 1),        # 65: a block whose second half is empty, behind a full one
    (6, 8, 192, 8, 8, 1),         # 96: a last block whose second half is empty
    (134, 8, 192, 1, 1, 1),       # a half's 32 tiles across 32 images, starting at images 64, 96 and 128
    (17, 8, 192, 1, 1, 4),        # 17 tiles
    (3, 8, 192, 10, 9, 4),        # a tile row wholly outside the image on the short sub-lattices
    (2, 16, 192, 18, 17, 1), (2, 16, 192, 18, 17, 2), (2, 16, 192, 18, 17, 4),
]


def test_tile_block_and_image_boundaries_are_exact(cw):
    for case in BOUNDARIES:
        _check_raw(cw, *case)
        _check_raw(cw, *case, caps=(0, 1, 3, 7), variant=2)


@pytest.mark.parametrize("C", [8, 24])
def test_remainders_of_one_of_half_the_grid_and_inside_a_tile_block(cw, C):
    """15 units (5 tile blocks x 3 channel blocks): cap 2 leaves 1 = G / 2, cap 7 leaves unit 14, which is the third channel
    block of the last tile block; cap 4 leaves 3, cap 5 none."""
    tails = _check_raw(cw, 5, C, 192, 16, 16, 1, (1, 2, 3, 7, 4, 5))
    assert tails == [0, 1, 0, 1, 3, 0]
    _check_raw(cw, 5, C, 192, 16, 16, 1, (1, 2, 3, 7), variant=2)


def _bn(K, g, affine=True):
    bn = nn.BatchNorm2d(K, affine=affine)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(K, generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(K, generator=g) + 0.5)
        if affine:
            bn.weight.copy_(torch.randn(K, generator=g))                      # both signs
            bn.bias.copy_(torch.randn(K, generator=g) * 0.3)
    return bn.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _normal_case(C, K, d):
    g = torch.Generator().manual_seed(4242 + C + K + d)
    conv = nn.Conv2d(C, K, 3, 1, d, d, bias=False)
    with torch.no_grad():
        conv.weight.normal_(0, (2.0 / (C * 9)) ** 0.5, generator=g)
    x = torch.randn(5, C, 16, 15, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    res = torch.randn(5, K, 16, 15, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    return conv.to(DEV).eval(), x, res, g


@pytest.mark.parametrize("mode,relu,affine", [("none", False, True), ("bn", True, True), ("bn", False, True), ("bn_add", True, True),
                                              ("bn_add", False, True), ("bn_bn_add", True, True), ("bn_bn_add", False, True),
                                              ("bn", True, False), ("bn_bn_add", False, False)])
def test_the_tail_has_the_bits_of_the_persistent_kernel(cw, mode, relu, affine):
    """All seven instantiations, and null gamma / beta: 15 units under caps 2, 4 and 7, d 1 and 2."""
    for d in (1, 2):
        conv, x, res, g = _normal_case(24, 192, d)
        bn, bn2 = _bn(192, g, affine), _bn(192, g, affine)
        residual = None if mode in ("none", "bn") else res
        residual_bn = bn2 if mode == "bn_bn_add" else None

        def run():
            if mode == "none":
                return cw.winograd_conv3x3(x, conv, force=True)
            return cw.winograd_conv3x3_bn_act(x, conv, bn, residual, residual_bn, relu=relu, force=True)

        with torch.no_grad():
            for cap in (2, 4, 7):
                cw.set_winograd_max_workgroups(cap)
                cw.set_winograd_tail(0)
                want = run()
                assert cw.last_tail_units() == 0
                cw.set_winograd_tail(2)
                before = cw.launch_count()
                got = run()
                assert cw.last_tail_units() == 15 % cap > 0 and cw.launch_count() == before + 1
                assert cw.last_epilogue() == (mode + ("_relu" if relu else "") if mode != "none" else "none")
                assert not torch.isnan(want).any() and (want > 0).any() and (relu or (want < 0).any())
                assert torch.equal(got, want), f"{mode} relu {relu} affine {affine} d {d} cap {cap}"
                cw.set_winograd_tail(0)
                cw.set_winograd_variant(2)
                got = run()
                assert cw.set_winograd_variant(0) == 2 and cw.last_variant() == 2 and cw.last_tail_units() == 0
                assert torch.equal(got, want), f"variant 2: {mode} relu {relu} affine {affine} d {d} cap {cap}"


def test_the_default_mode_tails_only_up_to_half_a_round_and_only_its_families(cw):
    """Mode 1 on a shape of the family table (the first of TAIL_FAMILIES, 5 x 16 x 16 pixels: 5 tile blocks): a remainder of at
    most G / 2 runs as half units, a larger one does not, and a shape outside the table never does.  One count per call."""
    assert cw.TAIL_FAMILIES, "no family has the tail on: nothing to check under mode 1"
    C, K, d = sorted(cw.TAIL_FAMILIES)[0]
    conv, x, _, _ = _normal_case(C, K, d)
    units = 5 * (K // 64)                                                     # 16 x 15 pixels are 64 tiles at every dilation
    outside, xo, _, _ = _normal_case(24, 192, 1)
    with torch.no_grad():
        cw.set_winograd_tail(0)
        cw.set_winograd_max_workgroups(units - 1)
        want = cw.winograd_conv3x3(x, conv, force=True)
        cw.set_winograd_tail(1)
        for cap, tail in ((units - 1, 1), (units // 2 + 1, 0), (units, 0)):   # rem 1 of G >= 2; rem just under G; none
            if cap < 2:
                continue
            cw.set_winograd_max_workgroups(cap)
            before = cw.launch_count()
            got = cw.winograd_conv3x3(x, conv, force=True)
            assert cw.launch_count() == before + 1
            rem = units % cap
            assert cw.last_tail_units() == (rem if tail else 0), (cap, rem)
            assert torch.equal(got, want)
        cw.set_winograd_max_workgroups(2)                                     # 15 units: rem 1 = G / 2, but not a family
        cw.winograd_conv3x3(xo, outside, force=True)
        assert cw.last_tail_units() == 0
