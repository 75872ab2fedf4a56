"""The 8-wave Winograd kernel (conv3x3_winograd_w16x2_f32, mvdetr_amd/csrc/conv_winograd.hip) under its de-phased schedule:
waves 4-7 run a program of their own whose loads and input transform sit in other half k-steps than those of waves 0-3,
with the same arithmetic, the same barrier and the same LDS layout.  The result has the bits of the lockstep schedule.

Bit identity: N(0, 1) inputs of both signs, all seven stores and null gamma / beta: schedule 2 against schedule 1 and against
variant 1 (the 4-wave kernel) with torch.equal, at one, two, three and eight chunks (the first-chunk instantiation alone, an
even and an odd count behind it), three channel blocks and three tile blocks that cross images, under caps of the persistent
grid that make one workgroup run units across images and channel blocks, so that the staging cursor (which the early role
moves in the middle of a chunk) crosses unit entries, and the last chunk is staged again.

Exact: integer inputs on which float32 F(2x2,3x3) has no rounding (conv_winograd_oracle.integer_case) against the fp64
direct convolution with torch.equal, x, U and y each inside a NaN-filled allocation.

The residual stores read the residual from a NaN-guarded buffer, and a residual that overlaps y is refused.

Every case asserts last_schedule() and last_variant() == 2, so that none passes on another path.

A build whose early role wrote the first row of the input transform into the other LDS buffer was run once against this file:
16 of 20 tests failed, every bit-identity test among them; the four that passed are the refusal test and three boundary cases
that never read that row from the wrong place or whose row is zero (docs/notes/conv_winograd.md)."""
import functools

import pytest
import torch
from torch import nn

import conv_winograd_oracle as oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 1024                                      # floats of NaN on either side, at the least
SCHEDULE = 2                                    # the de-phased schedule
CAPS = (1, 2, 3, 7, 0)                          # 9 units: one workgroup runs them all, ... , uncapped


@pytest.fixture(scope="module")
def cw():
    from mvdetr_amd.ops import conv_winograd
    return conv_winograd


@pytest.fixture(scope="module")
def te():
    from mvdetr_amd.ops import trunk_epilogue
    return trunk_epilogue


@pytest.fixture(autouse=True)
def _defaults_afterwards(cw):
    yield
    cw.set_winograd_max_workgroups(0)
    cw.set_winograd_tail(1)
    cw.set_winograd_variant(0)
    cw.set_winograd_schedule(0)


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
    """5 x 9 x 13 pixels: 35 tiles per image at d 1, 175 in all: three tile blocks, the first two across images."""
    g = torch.Generator().manual_seed(777 + C + K + d)
    conv = nn.Conv2d(C, K, 3, 1, d, d, bias=False)
    with torch.no_grad():
        conv.weight.normal_(0, (2.0 / (C * 9)) ** 0.5, generator=g)
    x = torch.randn(5, C, 9, 13, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    res = torch.randn(5, K, 9, 13, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    return conv.to(DEV).eval(), x, res, g


def _run_under(cw, fn, variant, schedule, cap):
    """fn() under (variant, schedule, cap, no tail); the knobs restored whatever happens, their previous values checked."""
    cw.set_winograd_max_workgroups(cap)
    cw.set_winograd_tail(0)
    cw.set_winograd_variant(variant)
    cw.set_winograd_schedule(schedule)
    try:
        before = cw.launch_count()
        out = fn()
        assert cw.launch_count() == before + 1 and cw.last_kernel() == "conv3x3_winograd_f32"
        assert cw.last_variant() == variant and cw.last_tail_units() == 0
        assert cw.last_schedule() == (schedule if variant == 2 else 1)
    finally:
        assert cw.set_winograd_schedule(0) == schedule and cw.set_winograd_variant(0) == variant
        assert cw.set_winograd_max_workgroups(0) == cap and cw.set_winograd_tail(1) == 0
    return out


@pytest.mark.parametrize("mode,relu,affine", [("none", False, True), ("bn", True, True), ("bn", False, True), ("bn_add", True, True),
                                              ("bn_add", False, True), ("bn_bn_add", True, True), ("bn_bn_add", False, True),
                                              ("bn_bn_add", True, False)])
def test_the_dephased_schedule_has_the_bits_of_lockstep(cw, mode, relu, affine):
    """All seven instantiations, and null gamma / beta once: K 192, C 8, 16, 24 and 64, under every cap of CAPS."""
    for C in (8, 16, 24, 64):
        conv, x, res, g = _normal_case(C, 192, 1)
        cw._transformed_weights(conv.weight)                                  # cached from here on: one launch per call below
        bn, bn2 = _bn(192, g, affine), _bn(192, g, affine)
        residual = None if mode in ("none", "bn") else res
        residual_bn = bn2 if mode == "bn_bn_add" else None

        def run():
            if mode == "none":
                return cw.winograd_conv3x3(x, conv, force=True)
            return cw.winograd_conv3x3_bn_act(x, conv, bn, residual, residual_bn, relu=relu, force=True)

        with torch.no_grad():
            for cap in CAPS:
                four = _run_under(cw, run, 1, 0, cap)
                lockstep = _run_under(cw, run, 2, 1, cap)
                got = _run_under(cw, run, 2, SCHEDULE, cap)
                assert cw.last_epilogue() == (mode + ("_relu" if relu else "") if mode != "none" else "none")
                assert not torch.isnan(lockstep).any() and (lockstep > 0).any() and (relu or (lockstep < 0).any())
                name = f"{mode} relu {relu} affine {affine} C {C} cap {cap}"
                assert torch.equal(got, lockstep), name + ": schedule 2 against schedule 1"
                assert torch.equal(got, four), name + ": schedule 2 against variant 1"


@pytest.mark.parametrize("d", [2, 4])
def test_the_dephased_schedule_has_the_bits_of_lockstep_under_dilation(cw, d):
    """The plain store and the widest one on the sub-lattice grids of dilation 2 and 4, three chunks, caps 2 and 0."""
    conv, x, res, g = _normal_case(24, 192, d)
    cw._transformed_weights(conv.weight)
    bn, bn2 = _bn(192, g), _bn(192, g)
    with torch.no_grad():
        for run in (lambda: cw.winograd_conv3x3(x, conv, force=True),
                    lambda: cw.winograd_conv3x3_bn_act(x, conv, bn, res, bn2, relu=True, force=True)):
            for cap in (2, 0):
                lockstep = _run_under(cw, run, 2, 1, cap)
                assert torch.equal(_run_under(cw, run, 2, SCHEDULE, cap), lockstep), f"d {d} cap {cap}"
                assert torch.equal(_run_under(cw, run, 1, 0, cap), lockstep), f"d {d} cap {cap}: variant 1"


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


def _check_exact(cw, N, C, K, H, W, d, caps=(0, 1, 2)):
    """The C entry under schedule 2 and every cap of ``caps`` on the same guarded x and U, a fresh guarded y per cap."""
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
        code = _run_under(cw, lambda: _lib.lib().mvdetr_conv3x3_winograd_f32(
            xin.data_ptr(), Uin.data_ptr(), y.data_ptr(), N, H, W, C, K, d, _lib.current_stream_ptr(torch.device(DEV))),
            2, SCHEDULE, cap)
        name = f"N {N} C {C} K {K} {H}x{W} d {d} cap {cap}"
        assert code == 0, name
        ybuf = ybuf.cpu()
        got = ybuf[PAD:-PAD].view(N, H, W, K).permute(0, 3, 1, 2)
        assert torch.isnan(ybuf[:PAD]).all() and torch.isnan(ybuf[-PAD:]).all(), name + ": a store outside y"
        assert not torch.isnan(got).any(), name + f": {int(torch.isnan(got).sum())} NaN in y (an element never stored, or a tap outside x read)"
        assert torch.equal(got.double(), want), name + ": " + oracle.first_mismatch(got, want, d)
    xbuf, Ubuf = xbuf.cpu(), Ubuf.cpu()
    assert torch.equal(xbuf[xpad:-xpad], x_flat) and torch.isnan(xbuf[:xpad]).all() and torch.isnan(xbuf[-xpad:]).all()
    assert torch.equal(Ubuf[Upad:-Upad], U_flat) and torch.isnan(Ubuf[:Upad]).all() and torch.isnan(Ubuf[-Upad:]).all()


@pytest.mark.parametrize("d", [1, 2, 4])
def test_geometry_grid_is_exact(cw, d):
    """H and W every pair of {1, 2, 3, 5, 9}, N 3, C 16 (two chunks), K 64."""
    for H in (1, 2, 3, 5, 9):
        for W in (1, 2, 3, 5, 9):
            _check_exact(cw, 3, 16, 64, H, W, d, (0, 1))


BOUNDARIES = [
    (4, 16, 64, 8, 8, 1),         # exactly 64 tiles
    (5, 16, 64, 2, 26, 1),        # 65: one tile in a second unit
    (134, 16, 64, 1, 1, 1),       # one tile per image: a unit's tiles across 64 images, and a third unit of 6
    (134, 8, 192, 1, 1, 1),       # the same with three channel blocks and a single chunk: every chunk enters a unit
]


@pytest.mark.parametrize("case", BOUNDARIES)
def test_tile_block_and_image_boundaries_are_exact(cw, case):
    _check_exact(cw, *case, caps=(0, 1, 2))


@pytest.mark.parametrize("mode,relu", [("bn_add", True), ("bn_bn_add", False)])
def test_the_residual_is_read_from_a_guarded_buffer(cw, te, mode, relu):
    """The residual inside a NaN-filled allocation, y too: schedule 2 has the bits of schedule 1, no NaN comes in, nothing
    outside y is stored, the residual is unchanged.  Caps 2 and 0."""
    from mvdetr_amd import _lib
    conv, x, res, g = _normal_case(24, 192, 1)
    N, K, H, W = res.shape
    bn, bn2 = _bn(K, g), (_bn(K, g) if mode == "bn_bn_add" else None)
    rbuf = torch.full((res.numel() + 2 * PAD,), float("nan"), device=DEV)
    rview = rbuf[PAD:PAD + res.numel()].view(N, H, W, K).permute(0, 3, 1, 2)
    rview.copy_(res)
    assert rview.is_contiguous(memory_format=torch.channels_last) and rview.data_ptr() % 16 == 0
    keep = rbuf.clone()
    U = cw._transformed_weights(conv.weight)

    def raw(y):
        return _lib.lib().mvdetr_conv3x3_winograd_bn_act_f32(
            x.data_ptr(), U.data_ptr(), y.data_ptr(), N, H, W, 24, K, 1, *te._bn_args(bn), rview.data_ptr(), *te._bn_args(bn2),
            int(relu), _lib.current_stream_ptr(x.device))

    with torch.no_grad():
        for cap in (2, 0):
            outs = []
            for schedule in (1, SCHEDULE):
                ybuf = torch.full((res.numel() + 2 * PAD,), float("nan"), device=DEV)
                assert _run_under(cw, lambda: raw(ybuf[PAD:PAD + res.numel()]), 2, schedule, cap) == 0
                assert cw.last_epilogue() == mode + ("_relu" if relu else "")
                assert torch.isnan(ybuf[:PAD]).all() and torch.isnan(ybuf[-PAD:]).all() and not torch.isnan(ybuf[PAD:-PAD]).any()
                outs.append(ybuf)
            assert torch.equal(outs[0][PAD:-PAD], outs[1][PAD:-PAD]), f"{mode} cap {cap}"
            want = cw.winograd_conv3x3_bn_act(x, conv, bn, rview, bn2, relu=relu, force=True)
            assert torch.equal(outs[1][PAD:-PAD].view(N, H, W, K).permute(0, 3, 1, 2), want)
    assert torch.equal(rbuf[PAD:-PAD], keep[PAD:-PAD]) and torch.isnan(rbuf[:PAD]).all() and torch.isnan(rbuf[-PAD:]).all()


def test_a_residual_that_overlaps_y_is_refused(cw, te):
    from mvdetr_amd import _lib
    conv, x, res, g = _normal_case(24, 192, 1)
    N, K, H, W = res.shape
    bn = _bn(K, g)
    U = cw._transformed_weights(conv.weight)
    n = res.numel()
    buf = torch.zeros(2 * n, device=DEV)

    def raw(y, r):
        return _lib.lib().mvdetr_conv3x3_winograd_bn_act_f32(
            x.data_ptr(), U.data_ptr(), y.data_ptr(), N, H, W, 24, K, 1, *te._bn_args(bn), r.data_ptr(), *te._bn_args(None), 1,
            _lib.current_stream_ptr(x.device))

    cw.set_winograd_variant(2)
    cw.set_winograd_schedule(SCHEDULE)
    try:
        before = cw.launch_count()
        for shift in (0, 4, n - 4):                                           # the same bytes, all but one, the last 16
            assert raw(buf[:n], buf[shift:shift + n]) == 1, shift             # hipErrorInvalidValue
            assert raw(buf[shift:shift + n], buf[:n]) == 1, shift
        assert cw.launch_count() == before
        assert raw(buf[:n], buf[n:]) == 0 and cw.last_schedule() == SCHEDULE and cw.last_variant() == 2
    finally:
        assert cw.set_winograd_schedule(0) == SCHEDULE and cw.set_winograd_variant(0) == 2
