"""The Winograd convolution's backward on the device (mvdetr_amd/csrc/conv_winograd_backward.hip, ops/conv_winograd.py).

Exact.  On conv_winograd_backward_oracle.integer_backward_case every intermediate of both kernels is exact in float32 in
any summation order and any split (the helper asserts the bounds from the arrays), so grad_x and grad_w must equal fp64
torch.nn.grad.conv2d_input / conv2d_weight BIT FOR BIT: over the forward's geometry grid at C = K = 64, (C, K) in
{64, 128, 192}^2 at 9 x 13, the forward's batch and tile-block boundaries, the weight gradient also under forced splits 1, 2,
3, 7 and more than there are chunks and under grids capped at 1 and 3 workgroups.  Every call has its outputs and the
workspace inside NaN-filled allocations and its inputs between NaN pads: nothing outside an output is written, every element
of it is, the inputs are unchanged, and a tap outside the image that was read and multiplied instead of replaced shows as NaN.

Measured bar.  Post-ReLU N(0, 1) x, N(0, 1) grad_y, kaiming weights: r = (the kernel's deviation from fp64) / (the deviation
of torch's fp32 convolution_backward under cudnn.deterministic), max-abs and rms, for grad_x and grad_w over
(C, K) in {(64, 64), (128, 64), (64, 128), (256, 192)} x {10 x 16, 9 x 13, 5 x 7, 18 x 17} x d in {1, 2, 4}; the assertion is
1.5 x the worst r measured on the MI355X: grad_x 13.20 max-abs and 15.01 rms (both at C 64, K 128, 5 x 7, d 4), grad_w 8.38
max-abs (C 128, K 64, 18 x 17, d 2) and 6.14 rms (C 256, K 192, 18 x 17, d 4) -- the forward's own worst are 19.76 and 18.74.

The rest: dgrad IS the forward kernel (bit-equal to winograd_conv3x3 on a Conv2d holding the flipped, transposed weights; Ut
against numpy); two calls are bit-identical; the adjoint identities in fp64 dot products; the autograd function (against fp64
autograd, each needs_input_grad combination by counted launches, NCHW and sliced grad_y, no second backward, the caches
after an in-place update); the small trunk and one train_step of the mini model with the route on against off."""
import copy
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import conv_winograd_backward_oracle as oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 1024
# worst r = kernel's deviation / torch's deviation, (max-abs, rms), measured on the MI355X over the 48 cases of
# test_against_fp64_with_the_measured_bar; the bars are 1.5 x these
R_WORST = {"grad_x": (13.20, 15.01), "grad_w": (8.38, 6.14)}


@pytest.fixture(scope="module")
def cw():
    from mvdetr_amd.ops import conv_winograd
    return conv_winograd


@pytest.fixture()
def settings(cw):
    prev = cw.set_winograd_wgrad_splits(0), cw.set_winograd_max_workgroups(0)
    yield cw
    cw.set_winograd_wgrad_splits(prev[0])
    cw.set_winograd_max_workgroups(prev[1])


def _lib():
    from mvdetr_amd import _lib
    return _lib.lib(), _lib.current_stream_ptr(torch.device(DEV))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _exact_case(N, C, K, H, W, d):
    """(x, gy, w, fp64 grad_x, fp64 grad_w) on the CPU, computed once and never written."""
    x, gy, w = oracle.integer_backward_case(N, C, K, H, W, d)
    return (x, gy, w) + oracle.reference_fp64(x, gy, w, d)


def _guarded(flat, pad=PAD):
    """A copy of the 1-d tensor ``flat`` on the device between two pads of NaN: (the whole buffer, the view, the pad)."""
    pad = (max(pad, PAD) + 3) // 4 * 4
    buf = torch.full((flat.numel() + 2 * pad,), float("nan"), device=DEV)
    inner = buf[pad:pad + flat.numel()]
    inner.copy_(flat)
    assert inner.data_ptr() % 16 == 0
    return buf, inner, pad


def _nan_buffer(n):
    buf = torch.full((n + 2 * PAD,), float("nan"), device=DEV)
    return buf, buf[PAD:PAD + n]


def _pads_untouched(buf, pad, flat=None):
    host = buf.cpu()
    ok = torch.isnan(host[:pad]).all() and torch.isnan(host[-pad:]).all()
    return bool(ok and (flat is None or torch.equal(host[pad:-pad], flat)))


def _check_wgrad(cw, case, name=""):
    """The C entry on guarded buffers against the fp64 reference, bit for bit; returns (gw on the host, S)."""
    N, C, K, H, W, d = case
    x, gy, w, _, want = _exact_case(*case)
    lib, st = _lib()
    reach = (d * W + d) * max(C, K)
    x_flat, g_flat = x.permute(0, 2, 3, 1).reshape(-1), gy.permute(0, 2, 3, 1).reshape(-1)
    xbuf, xin, xpad = _guarded(x_flat, reach)
    gbuf, gin, gpad = _guarded(g_flat, reach)
    need = lib.mvdetr_winograd_wgrad_workspace_bytes(N, H, W, C, K, d, _cus())
    assert need > 0 and need % (C * K * 36) == 0
    wbuf, gw = _nan_buffer(K * C * 9)
    sbuf, ws = _nan_buffer(need // 4)
    before = cw.launch_count()
    code = lib.mvdetr_conv3x3_winograd_wgrad_f32(xin.data_ptr(), gin.data_ptr(), gw.data_ptr(), N, H, W, C, K, d, ws.data_ptr(), need, st)
    name = f"{name} N {N} C {C} K {K} {H}x{W} d {d} S {cw.last_wgrad_splits()}"
    assert code == 0 and cw.launch_count() == before + 1 and cw.last_kernel() == "conv3x3_winograd_wgrad_f32", name
    S = cw.last_wgrad_splits()
    assert S == need // (C * K * 36) == cw.wgrad_plan(N, H, W, C, K, d, _cus())["S"], name
    got = gw.cpu().view(K, C, 3, 3)
    assert _pads_untouched(wbuf, PAD) and _pads_untouched(sbuf, PAD), name + ": a store outside gw or the workspace"
    assert not torch.isnan(got).any(), name + f": {int(torch.isnan(got).sum())} NaN in gw (never stored, or a tap outside the image read)"
    assert not torch.isnan(ws).any(), name + ": a slice of the workspace was not written"
    assert torch.equal(got.double(), want), name + ": " + oracle.first_mismatch_w(got, want)
    assert _pads_untouched(xbuf, xpad, x_flat) and _pads_untouched(gbuf, gpad, g_flat), name + ": an input was written"
    return got, S


def _check_dgrad(cw, case):
    N, C, K, H, W, d = case
    x, gy, w, want, _ = _exact_case(*case)
    lib, st = _lib()
    reach = (d * W + d) * max(C, K)
    g_flat = gy.permute(0, 2, 3, 1).reshape(-1)
    gbuf, gin, gpad = _guarded(g_flat, reach)
    wd = w.to(DEV)
    ubuf, Ut = _nan_buffer(16 * K * C)
    xbuf, gx = _nan_buffer(N * H * W * C)
    before = cw.launch_count()
    assert lib.mvdetr_winograd_weights_dgrad_f32(wd.data_ptr(), C, K, Ut.data_ptr(), st) == 0
    assert cw.last_kernel() == "winograd_weights_dgrad_f32"
    assert lib.mvdetr_conv3x3_winograd_f32(gin.data_ptr(), Ut.data_ptr(), gx.data_ptr(), N, H, W, K, C, d, st) == 0
    assert cw.launch_count() == before + 2
    name = f"dgrad N {N} C {C} K {K} {H}x{W} d {d}"
    assert np.array_equal(Ut.cpu().view(16, K, C).numpy(), oracle.dgrad_weights(w.numpy())), name + ": Ut"
    got = gx.cpu().view(N, H, W, C).permute(0, 3, 1, 2)
    assert _pads_untouched(xbuf, PAD) and _pads_untouched(ubuf, PAD), name + ": a store outside gx or Ut"
    assert not torch.isnan(got).any(), name
    assert torch.equal(got.double(), want), name + ": " + oracle.fwd.first_mismatch(got, want, d)
    assert _pads_untouched(gbuf, gpad, g_flat) and torch.equal(wd.cpu(), w), name + ": an input was written"


def _check_grid(cw, cases, label):
    sx, sw = [], []
    for case in cases:
        _check_dgrad(cw, case)
        _check_wgrad(cw, case)
        _, _, _, gx, gw = _exact_case(*case)
        a, b = oracle.check_sanity(gx, gw, *case[3:])
        assert a >= 0.90 and b >= 0.90, (case, a, b)
        sx.append(a)
        sw.append(b)
    print(f"{label}: {len(cases)} cases, grad_x and grad_w bit-equal to fp64; non-zero share of the references grad_x "
          f"{min(sx):.3f} - {max(sx):.3f}, grad_w (reachable taps) {min(sw):.3f} - {max(sw):.3f}")


@pytest.mark.parametrize("d", [1, 2, 4])
def test_geometry_grid_is_exact(settings, d):
    cases = [c for c in oracle.GEOMETRY_GRID if c[5] == d]
    assert len(cases) == 36
    _check_grid(settings, cases, f"geometry d {d}")


@pytest.mark.parametrize("d", [1, 2, 4])
def test_channel_grid_is_exact(settings, d):
    cases = [c for c in oracle.CHANNEL_GRID if c[5] == d]
    assert len(cases) == 9
    _check_grid(settings, cases, f"channels d {d}")


def test_batch_and_tile_block_boundaries_are_exact(settings):
    assert len(oracle.BOUNDARY_GRID) == 9
    _check_grid(settings, oracle.BOUNDARY_GRID, "boundaries")


def test_wgrad_is_exact_under_every_forced_split(settings):
    cw = settings
    seen = set()
    for case in oracle.BOUNDARY_GRID + [(2, 128, 192, 9, 13, 2), (3, 64, 64, 5, 9, 4)]:
        N, C, K, H, W, d = case
        chunks = -(-oracle.tile_count(N, H, W, d) // 8)
        for forced in oracle.SPLITS:
            cw.set_winograd_wgrad_splits(forced)
            _, S = _check_wgrad(cw, case, f"forced {forced}")
            per = -(-chunks // min(forced, chunks))
            assert S == -(-chunks // per) <= chunks
            seen.add(S)
        cw.set_winograd_wgrad_splits(0)
    assert {1, 2, 3, 7} <= seen and max(seen) > 7, seen


@pytest.mark.parametrize("cap", [1, 3])
def test_wgrad_is_exact_under_a_capped_grid(settings, cap):
    """Fewer workgroups than items: each runs several (unit, split) items one after the other."""
    cw = settings
    cw.set_winograd_max_workgroups(cap)
    for case in ((2, 128, 192, 9, 13, 1), (2, 192, 128, 9, 13, 4), (2, 64, 64, 18, 17, 2)):
        _check_wgrad(cw, case, f"cap {cap}")
        _check_dgrad(cw, case)
    cw.set_winograd_wgrad_splits(3)                                            # 3 splits of every unit on `cap` workgroups
    _, S = _check_wgrad(cw, (2, 128, 128, 9, 13, 2), f"cap {cap} forced 3")
    assert S == 3


def test_public_entries_on_the_boundary_grid(settings):
    """The same bits from winograd_conv3x3_input_grad / _weight_grad: the cached Ut, torch's allocations and workspace."""
    cw = settings
    for case in oracle.BOUNDARY_GRID:
        N, C, K, H, W, d = case
        x, gy, w, want_x, want_w = _exact_case(*case)
        xd, gd, wd = x.to(DEV), gy.to(DEV), w.to(DEV)
        before = cw.launch_count()
        gx = cw.winograd_conv3x3_input_grad(gd, wd, d)
        assert cw.launch_count() == before + 2 and cw.last_kernel() == "conv3x3_winograd_f32"
        gx2 = cw.winograd_conv3x3_input_grad(gd, wd, d)
        assert cw.launch_count() == before + 3                                 # Ut is cached
        gw = cw.winograd_conv3x3_weight_grad(xd, gd, d)
        assert cw.launch_count() == before + 4 and cw.last_kernel() == "conv3x3_winograd_wgrad_f32"
        gw2 = cw.winograd_conv3x3_weight_grad(xd, gd, d)
        assert gx.is_contiguous(memory_format=torch.channels_last) and gw.is_contiguous() and gw.shape == w.shape
        assert torch.equal(gx, gx2) and torch.equal(gw, gw2)
        assert torch.equal(gx.cpu().double(), want_x), oracle.fwd.first_mismatch(gx.cpu(), want_x, d)
        assert torch.equal(gw.cpu().double(), want_w), oracle.first_mismatch_w(gw.cpu(), want_w)
        assert torch.equal(xd.cpu(), x) and torch.equal(gd.cpu(), gy) and torch.equal(wd.cpu(), w)


def test_an_empty_batch_writes_zeros(settings):
    lib, st = _lib()
    x = torch.zeros(64, device=DEV)
    wbuf, gw = _nan_buffer(64 * 64 * 9)
    assert lib.mvdetr_conv3x3_winograd_wgrad_f32(x.data_ptr(), x.data_ptr(), gw.data_ptr(), 0, 4, 4, 64, 64, 1, None, 0, st) == 0
    assert _pads_untouched(wbuf, PAD) and not gw.cpu().any()


# ---- the measured bar --------------------------------------------------------------------------------------------------------------
def _real_case(C, K, H, W, d, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + C + 3 * K + 7 * H + 11 * W + 13 * d + 5)
    w = torch.randn(K, C, 3, 3, generator=g) * (2.0 / (K * 9)) ** 0.5         # kaiming_normal_(fan_out, relu)
    x = torch.randn(2, C, H, W, generator=g).relu_()
    gy = torch.randn(2, K, H, W, generator=g)
    cl = lambda t: t.to(DEV).contiguous(memory_format=torch.channels_last)    # noqa: E731
    return cl(x), cl(gy), w.to(DEV)


def _dev(a, want):
    e = (a.double() - want).abs()
    return e.max().item(), e.square().mean().sqrt().item()


@pytest.mark.parametrize("d", [1, 2, 4])
@pytest.mark.parametrize("H,W", [(10, 16), (9, 13), (5, 7), (18, 17)])
@pytest.mark.parametrize("C,K", [(64, 64), (128, 64), (64, 128), (256, 192)])
def test_against_fp64_with_the_measured_bar(settings, C, K, H, W, d):
    cw = settings
    x, gy, w = _real_case(C, K, H, W, d)
    keep = [t.clone(memory_format=torch.preserve_format) for t in (x, gy, w)]
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        want_x = torch.nn.grad.conv2d_input(x.shape, w.double(), gy.double(), 1, d, d)
        want_w = torch.nn.grad.conv2d_weight(x.double(), w.shape, gy.double(), 1, d, d)
        tx, tw, _ = torch.ops.aten.convolution_backward(gy, x, w, None, (1, 1), (d, d), (d, d), False, (0, 0), 1, [True, True, False])
        gx = cw.winograd_conv3x3_input_grad(gy, w, d)
        gw = cw.winograd_conv3x3_weight_grad(x, gy, d)
        again = cw.winograd_conv3x3_input_grad(gy, w, d), cw.winograd_conv3x3_weight_grad(x, gy, d)
    finally:
        torch.backends.cudnn.deterministic = prev
    assert torch.equal(gx, again[0]) and torch.equal(gw, again[1])            # bit-identical call to call at the same split
    assert all(torch.equal(a, b) for a, b in zip((x, gy, w), keep))
    ratios = {}
    for name, got, ref, want in (("grad_x", gx, tx, want_x), ("grad_w", gw, tw, want_w)):
        got_max, got_rms = _dev(got, want)
        t_max, t_rms = _dev(ref, want)
        assert t_max > 0 and t_rms > 0 and want.abs().max().item() > 1, name
        ratios[name] = got_max / t_max, got_rms / t_rms
        print(f"C {C} K {K} {H}x{W} d {d} {name}: winograd max {got_max:.3e} rms {got_rms:.3e} | torch max {t_max:.3e} rms {t_rms:.3e} "
              f"| r max {ratios[name][0]:.2f} rms {ratios[name][1]:.2f}")
    for name, (r_max, r_rms) in ratios.items():
        assert r_max <= 1.5 * R_WORST[name][0] and r_rms <= 1.5 * R_WORST[name][1], name


# ---- dgrad is the forward kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K,H,W,d", [(64, 64, 9, 13, 1), (128, 64, 10, 16, 2), (64, 192, 5, 7, 4)])
def test_dgrad_is_the_forward_kernel_on_the_flipped_transposed_weights(settings, C, K, H, W, d):
    cw = settings
    x, gy, w = _real_case(C, K, H, W, d)
    twin = nn.Conv2d(K, C, 3, 1, d, d, bias=False).to(DEV).eval()
    with torch.no_grad():
        twin.weight.copy_(w.flip(2, 3).transpose(0, 1))
        want = cw.winograd_conv3x3(gy, twin, force=True)
    got = cw.winograd_conv3x3_input_grad(gy, w, d)
    assert torch.equal(got, want) and got.abs().max().item() > 0.1
    # Ut against numpy on these kaiming weights: both are an fp64 evaluation rounded once, so at most one float32 rounding
    # apart (+ 2^-50 max|w| for the differently ordered fp64 sums), and almost everywhere identical
    Ut = cw._transformed_weights_dgrad(w).cpu().numpy()
    ref = oracle.dgrad_weights(w.cpu().numpy())
    diff = np.abs(Ut.astype(np.float64) - ref.astype(np.float64))
    assert Ut.shape == (16, K, C) and (diff <= np.spacing(np.abs(ref)).astype(np.float64) + 2.0 ** -50 * w.abs().max().item()).all()
    assert (Ut == ref).mean() >= 0.999


# ---- adjoint identities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K,H,W,d", [(64, 128, 9, 13, 1), (128, 64, 18, 17, 2), (64, 64, 10, 9, 4)])
def test_adjoint_identities(settings, C, K, H, W, d):
    """<gy, conv(x)> = <dgrad(gy), x> = <wgrad(x, gy), w>: all three are the SAME triple sum of gy x w products, evaluated in
    float32 in three groupings and dotted in fp64.  Bar, from the term count: with S = the sum of the |gy x w| (fp64, as
    <|gy|, conv(|x|, |w|)>), every term goes through at most n + 16 float32 roundings -- n the longest accumulation chain of
    the three (C, K, or the tiles) plus the transforms' adds -- each relative to a partial sum that the transforms' coefficients
    (absolute row sums <= 2 per axis) bound by 4 x the absolute sum: 4 (n + 16) 2^-24 S."""
    cw = settings
    x, gy, w = _real_case(C, K, H, W, d)
    conv = nn.Conv2d(C, K, 3, 1, d, d, bias=False).to(DEV).eval()
    with torch.no_grad():
        conv.weight.copy_(w)
        y = cw.winograd_conv3x3(x, conv, force=True)
    gx, gw = cw.winograd_conv3x3_input_grad(gy, w, d), cw.winograd_conv3x3_weight_grad(x, gy, d)
    dot = lambda a, b: (a.double() * b.double()).sum().item()                 # noqa: E731
    lhs, via_x, via_w = dot(gy, y), dot(gx, x), dot(gw, w)
    S = dot(gy.abs(), F.conv2d(x.double().abs(), w.double().abs(), None, 1, d, d))
    truth = dot(gy, F.conv2d(x.double(), w.double(), None, 1, d, d))
    n = max(C, K, oracle.tile_count(2, H, W, d))
    bar = 4 * (n + 16) * 2.0 ** -24 * S
    print(f"C {C} K {K} {H}x{W} d {d}: <gy, y> {lhs:.9e} <gx, x> {via_x:.9e} <gw, w> {via_w:.9e} fp64 {truth:.9e} | bar {bar:.3e} "
          f"worst {max(abs(v - truth) for v in (lhs, via_x, via_w)):.3e}")
    assert abs(truth) > 1 and S > abs(truth)
    for v in (lhs, via_x, via_w):
        assert abs(v - truth) <= bar


# ---- the autograd function -------------------------------------------------------------------------------------------------------------
def _conv_for(w, d):
    conv = nn.Conv2d(w.shape[1], w.shape[0], 3, 1, d, d, bias=False).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w)
    return conv


# Gradients of these tests' scale (|x|, |gy| ~ 1, |w| ~ sqrt(2 / 9 K): grad_x ~ 1, grad_w ~ 15, float32 errors ~ 1e-5) against
# fp64.  The measured-bar test holds the kernels to torch's own error; this is a coarse absolute bar for the plumbing, which any
# wrong index, layout or stale cache misses by orders of magnitude.
COARSE = 1e-3


@pytest.mark.parametrize("need_x,need_w", [(True, True), (True, False), (False, True)])
def test_autograd_against_fp64_and_only_the_needed_pieces_run(settings, need_x, need_w):
    cw = settings
    C, K, H, W, d = 64, 128, 9, 13, 2
    x, gy, w = _real_case(C, K, H, W, d)
    conv = _conv_for(w, d)
    conv.weight.requires_grad_(need_w)
    xin = x.clone(memory_format=torch.preserve_format).requires_grad_(need_x)
    y = cw.winograd_conv3x3_train(xin, conv, force=True)
    assert y.requires_grad and y.is_contiguous(memory_format=torch.channels_last)
    cw._transformed_weights_dgrad(conv.weight)                                 # (Ut: a launch of its own on first use)
    before = cw.launch_count()
    inputs = ([xin] if need_x else []) + ([conv.weight] if need_w else [])
    grads = torch.autograd.grad(y, inputs, gy)
    assert cw.launch_count() == before + need_x + need_w                       # the piece that is not needed is not run
    assert cw.last_kernel() == ("conv3x3_winograd_wgrad_f32" if need_w else "conv3x3_winograd_f32")
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    want = dict(zip("xw", torch.autograd.grad(F.conv2d(x64, w64, None, 1, d, d), (x64, w64), gy.double())))
    with torch.no_grad():
        assert torch.equal(y, cw.winograd_conv3x3(x, copy.deepcopy(conv).requires_grad_(False), force=True))
    for name, got in zip([n for n, need in (("x", need_x), ("w", need_w)) if need], grads):
        assert got.shape == want[name].shape and _dev(got, want[name])[0] <= COARSE, name
    if need_x:
        assert torch.equal(grads[0], cw.winograd_conv3x3_input_grad(gy, conv.weight.detach(), d))
    if need_w:
        assert torch.equal(grads[-1], cw.winograd_conv3x3_weight_grad(x, gy, d))


def test_autograd_takes_any_layout_of_grad_y_and_differentiates_once(settings):
    cw = settings
    C, K, H, W, d = 64, 64, 10, 16, 1
    x, gy, w = _real_case(C, K, H, W, d)
    conv = _conv_for(w, d)
    xin = x.clone(memory_format=torch.preserve_format).requires_grad_(True)

    def grads(g):
        return torch.autograd.grad(cw.winograd_conv3x3_train(xin, conv, force=True), (xin, conv.weight), g)

    want = grads(gy)
    nchw = gy.contiguous()                                                     # NCHW memory
    assert not nchw.is_contiguous(memory_format=torch.channels_last)
    big = torch.randn(2, K + 2, H, W + 2, device=DEV).contiguous(memory_format=torch.channels_last)
    big[:, 1:K + 1, :, 1:W + 1] = gy
    sliced = big[:, 1:K + 1, :, 1:W + 1]                                       # a slice of a larger tensor, 4 bytes off 16
    assert not sliced.is_contiguous(memory_format=torch.channels_last) and sliced.data_ptr() % 16 != 0
    for g in (nchw, sliced):
        got = grads(g)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # through a loss, and no second backward through the graph
    y = cw.winograd_conv3x3_train(xin, conv, force=True)
    (gx,) = torch.autograd.grad((y * gy).sum(), xin, create_graph=True)
    assert torch.equal(gx, want[0])
    with pytest.raises(RuntimeError):
        gx.sum().backward()
    with pytest.raises(RuntimeError, match="do not take the kernel"):
        cw.winograd_conv3x3_train(xin[:, :, :, 1:], conv, force=True)          # not dense: nothing falls back silently


def test_both_caches_are_rebuilt_after_an_in_place_update(settings):
    cw = settings
    C, K, H, W, d = 64, 64, 9, 13, 1
    x, gy, w = _real_case(C, K, H, W, d)
    conv = _conv_for(w, d)
    opt = torch.optim.SGD(conv.parameters(), lr=0.05)
    xin = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
    counts = []
    for step in range(3):
        opt.zero_grad()
        before = cw.launch_count()
        y = cw.winograd_conv3x3_train(xin, conv, force=True)
        gx, gw = torch.autograd.grad(y, (xin, conv.weight), gy)
        counts.append(cw.launch_count() - before)
        w_now = conv.weight.detach().double()
        want_x = torch.nn.grad.conv2d_input(x.shape, w_now, gy.double(), 1, d, d)
        assert _dev(gx, want_x)[0] <= COARSE, step            # the data gradient of the CURRENT weights
        with torch.no_grad():
            assert _dev(y, F.conv2d(x.double(), w_now, None, 1, d, d))[0] <= COARSE, step
        if step < 2:
            conv.weight.grad = gw
            opt.step()
    assert counts == [5, 5, 5]                                                 # U, forward, Ut, dgrad, wgrad: every step rebuilds both
    before = cw.launch_count()
    torch.autograd.grad(cw.winograd_conv3x3_train(xin, conv, force=True), (xin, conv.weight), gy)
    assert cw.launch_count() == before + 3                                     # unchanged weights: neither transform


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
REPS = 3
SMALL = 64


class _TrainRoute:
    """Every 3x3 convolution of ``model`` that the training route can take switched on in TRAIN_FAMILIES, floors at 0, MIOpen's
    default solvers."""
    def __init__(self, cw, model):
        self.cw = cw
        self.convs = [m for m in model.modules() if type(m) is nn.Conv2d and m.kernel_size == (3, 3) and m.stride == (1, 1)
                      and m.in_channels % 64 == 0 and m.out_channels % 64 == 0 and m.padding == m.dilation and m.bias is None]
        self.table = {}
        for m in self.convs:
            self.table.setdefault((m.in_channels, m.out_channels), {})[m.dilation[0]] = cw.PIECES

    def __enter__(self):
        cw = self.cw
        self.prev = (cw.TRAIN_FAMILIES, cw.set_winograd_train_min_pixels(0), cw.set_winograd_min_pixels(0),
                     cw.set_winograd_narrow_min_pixels(0), torch.backends.cudnn.deterministic, cw.set_trunk_winograd_training(True))
        cw.TRAIN_FAMILIES = self.table
        torch.backends.cudnn.deterministic = False
        return self

    def __exit__(self, *exc):
        cw = self.cw
        cw.TRAIN_FAMILIES = self.prev[0]
        cw.set_winograd_train_min_pixels(self.prev[1])
        cw.set_winograd_min_pixels(self.prev[2])
        cw.set_winograd_narrow_min_pixels(self.prev[3])
        torch.backends.cudnn.deterministic = self.prev[4]
        cw.set_trunk_winograd_training(self.prev[5])


def _solver_runs(run):
    default = [run() for _ in range(REPS)]
    torch.backends.cudnn.deterministic = True
    try:
        return default, run()
    finally:
        torch.backends.cudnn.deterministic = False


def _assert_within(names, on, off, det, fp64):
    """on[r][i] against off[r][i] within 2 x (off[r][i] against det[i]), tensor by tensor, each side the largest of REPS
    repetitions: the rule of test_conv_winograd_gpu._assert_within (3 x fp32-vs-fp64 where the two solver choices agree).
    That rule compares max-abs and rms of tensors of thousands of elements, which are stable statistics; the deviation of a
    tensor of one or two elements (a head's bias) is a single draw on either side, and the ratio of two draws has no bound.
    So the tensors of fewer than SMALL elements (but a scalar loss, named "loss", which the rule is asked of by itself) are
    concatenated into one vector, "small tensors", before the rule is applied."""
    pool = [i for i, name in enumerate(names) if name != "loss" and on[0][i].numel() < SMALL]
    if pool:
        cat = lambda ts: torch.cat([ts[i].reshape(-1) for i in pool])            # noqa: E731
        keep = [i for i in range(len(names)) if i not in pool]
        regroup = lambda ts: [ts[i] for i in keep] + [cat(ts)]                   # noqa: E731
        names = [names[i] for i in keep] + [f"small tensors ({len(pool)})"]
        on, off, det, fp64_all = [regroup(t) for t in on], [regroup(t) for t in off], regroup(det), fp64
        fp64 = lambda: regroup(fp64_all())                                       # noqa: E731
    failed = []
    for i, name in enumerate(names):
        devs = [_dev(a[i], b[i].double()) for a, b in zip(on, off)]
        d_max, d_rms = max(v[0] for v in devs), max(v[1] for v in devs)
        bars = [_dev(o[i], det[i].double()) for o in off]
        b_max, b_rms, how = 2 * max(v[0] for v in bars), 2 * max(v[1] for v in bars), "2 x solver-vs-solver"
        if b_max == 0:
            f_max, f_rms = _dev(off[0][i], fp64()[i])
            b_max, b_rms, how = 3 * f_max, 3 * f_rms, "3 x fp32-vs-fp64"
        line = f"{name}: on vs off max {d_max:.3e} rms {d_rms:.3e} | bar ({how}) max {b_max:.3e} rms {b_rms:.3e}"
        print(line)
        if not (d_max <= b_max and d_rms <= b_rms):
            failed.append(line)
    assert not failed, "\n".join(failed)


def test_trunk_in_training_with_the_route_on_against_off(settings):
    cw = settings
    from mvdetr_amd.model import resnet_trunk
    torch.manual_seed(0)
    trunk = resnet_trunk(18).to(DEV).train()
    keys = list(trunk.state_dict())
    x = torch.randn(2, 3, 128, 192, generator=torch.Generator().manual_seed(5)).to(DEV).contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    params = [p for _, p in trunk.named_parameters()]
    names = ["input"] + [n for n, _ in trunk.named_parameters()]
    stats = {k: v.clone() for k, v in trunk.named_buffers()}

    def run(count=None):
        with torch.no_grad():
            for k, v in trunk.named_buffers():                                 # the same running statistics every time
                v.copy_(stats[k])
        before = cw.launch_count()
        out = trunk(x)
        fwd = cw.launch_count() - before
        grads = torch.autograd.grad(out.square().mean(), [x] + params)
        if count is not None:
            count.append((fwd, cw.launch_count() - before - fwd))
        return list(grads)

    with _TrainRoute(cw, trunk) as route:
        n = len(route.convs)
        assert n >= 12                                                         # layer1-4 of ResNet-18 but the strided ones
        run()                                                                  # (builds U and Ut)
        counts = []
        on = [run(counts) for _ in range(REPS)]
        assert counts == [(n, 2 * n)] * REPS, (n, counts)                      # a forward each; a dgrad and a wgrad each
        prev = cw.set_trunk_winograd_training(False)
        try:
            before = cw.launch_count()
            off, det = _solver_runs(run)
            assert cw.launch_count() == before
        finally:
            cw.set_trunk_winograd_training(prev)
        torch.backends.cudnn.deterministic = True                              # the caller asked for determinism: torch's
        before = cw.launch_count()
        run()
        assert cw.launch_count() == before
        torch.backends.cudnn.deterministic = False
        fp64 = []

        def double_grads():
            if not fp64:
                t64 = copy.deepcopy(trunk).double()
                x64 = x.detach().double().requires_grad_(True)
                fp64.extend(torch.autograd.grad(t64(x64).square().mean(), [x64] + list(t64.parameters())))
            return fp64
        _assert_within(names, on, off, det, double_grads)
    assert list(trunk.state_dict()) == keys
    before = cw.launch_count()                                                 # at the default floors this input keeps torch's
    run()
    assert cw.launch_count() == before


def test_the_environment_switch_keeps_torchs_convolutions_in_training():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import torch\n"
        "from mvdetr_amd.ops import conv_winograd as cw\n"
        "from mvdetr_amd.model import BasicBlock\n"
        "cw.set_winograd_train_min_pixels(0)\n"
        "cw.TRAIN_FAMILIES[(64, 64)] = {1: cw.PIECES}\n"
        "b = BasicBlock(64, 64).cuda().train()\n"
        "x = torch.randn(2, 64, 8, 8, device='cuda').contiguous(memory_format=torch.channels_last).requires_grad_(True)\n"
        "b(x).sum().backward()\n"
        "torch.cuda.synchronize()\n"
        "print('LAUNCHES', cw.launch_count(), cw.trunk_winograd_training_enabled())\n"
    ) % root
    # on: per convolution U, forward, Ut, dgrad, wgrad
    for value, want in (("0", "LAUNCHES 0 False"), ("1", "LAUNCHES 10 True")):
        env = dict(os.environ, MVDETR_TRUNK_WINOGRAD_TRAIN=value)
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert want in out.stdout, out.stdout + out.stderr


def test_one_train_step_of_the_mini_model_on_against_off(settings):
    cw = settings
    from mvdetr_amd import geometry
    from mvdetr_amd.model import build_model
    from mvdetr_amd.targets import synthetic_frame_targets
    from mvdetr_amd.train import MVDeTrCriterion, train_step
    g = geometry.MINI
    model0 = build_model("mini", seed=0, channels_last=True, dropout=0.0).to(DEV).train()
    keys = list(model0.state_dict())
    world_gt, imgs_gt = synthetic_frame_targets(g, 8, seed=0)
    world_gt, imgs_gt = ({k: v.to(DEV) for k, v in t.items()} for t in (world_gt, imgs_gt))
    imgs = torch.randn(1, g.num_cam, 3, *g.input_img_shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    M = torch.eye(3).repeat(1, g.num_cam, 1, 1)
    crit = MVDeTrCriterion()
    names = ["loss"] + [n for n, _ in model0.named_parameters()]
    # A step of plain SGD at rate 1: the updated parameters then differ between two runs by the gradients' own deviation.  At a
    # small rate the deviation of p - rate * g is below the spacing of p, both sides of the rule count a handful of one-ulp
    # flips, and their ratio says nothing about the convolutions.
    LR = 1.0

    def run():
        model = copy.deepcopy(model0)
        opt = torch.optim.SGD(model.parameters(), lr=LR)
        loss = train_step(model, crit, opt, imgs, M, world_gt, imgs_gt)
        return [loss] + [p.detach() for p in model.parameters()]

    with _TrainRoute(cw, model0) as route:
        assert route.convs
        before = cw.launch_count()
        on = [run() for _ in range(REPS)]
        assert cw.launch_count() > before and cw.last_kernel() in ("conv3x3_winograd_wgrad_f32", "conv3x3_winograd_f32")
        prev = cw.set_trunk_winograd_training(False)
        try:
            before = cw.launch_count()
            off, det = _solver_runs(run)
            assert cw.launch_count() == before
        finally:
            cw.set_trunk_winograd_training(prev)
        fp64 = []

        def double_step():
            if not fp64:
                model = copy.deepcopy(model0).cpu().double()                   # on the host: torch's ops throughout
                opt = torch.optim.SGD(model.parameters(), lr=LR)
                to64 = lambda t: {k: v.cpu().double() if v.is_floating_point() else v.cpu() for k, v in t.items()}    # noqa: E731
                loss = train_step(model, crit, opt, imgs.cpu().double(), M.double(), to64(world_gt), to64(imgs_gt))
                fp64.extend([loss.to(DEV)] + [p.detach().to(DEV) for p in model.parameters()])
            return fp64
        _assert_within(names, on, off, det, double_step)
    assert list(model0.state_dict()) == keys
