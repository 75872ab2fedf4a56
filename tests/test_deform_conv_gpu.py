"""Deformable convolution on the MI355X: the MFMA implicit-GEMM route and the generic kernels against the fp64 restatement
(tests/deform_conv_oracle.py), the route pinned by last_kernel, and the deform_conv model on the GPU vs the CPU.

Bars: per element, from the fp32 error model of tests/deform_conv_cases.py (forward, grad_input, grad_offset, grad_weight,
grad_bias; the large forward-only cases keep fp32_bar of tests/test_deform_conv.py, whose operands fit in memory there).
Taps within 1e-4 px of an integer coordinate or of the -1 / H edge are masked out of the offset-gradient comparison when
the offsets are random (fp32 rounding can flip the floor there); the dyadic cases compare every tap.

The geometry matrix of tests/deform_conv_cases.py runs forward and backward on dc_*_mfma (channel-last, and NCHW for a few)
and on dc_*_generic (the fp32 twins, and fp64 on every shape); among its MFMA cases are the launch structures C_out = 160
and 256 (blockIdx.y > 0), C = C_out = 160, an output of 24 pixels (dc_bwd_weight_mfma's single-range direct store),
C = 16 under stride 2 (dc_fwd_mfma<16>) and pixel tiles that straddle batch items.  Every check prints its largest
err / bar per tensor before it asserts (pytest -s)."""
import pytest
import torch
import torch.nn.functional as F

import deform_conv_cases as cases
from deform_conv_oracle import with_grads
from deform_conv_oracle import deform_conv2d as oracle
from deform_conv_cases import NONFINITE_IDS, check_against_oracle, check_nonfinite, matrix_reference, nonfinite_reference
from test_deform_conv import EPS32, fp32_bar

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _ops():
    from mvdetr_amd.ops import deform_conv
    return deform_conv


def _case(C, Co, H, W, seed, scale=None, model_like=False, B=1, k=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(Co, C, k, k, generator=g) / (C * k * k) ** 0.5
    b = torch.randn(Co, generator=g) * 0.1
    if model_like:                      # a random 1x1 conv of features + position embedding: ~1 px offsets
        from mvdetr_amd.world_feat import create_pos_embedding
        feat = x + create_pos_embedding((H, W), C // 2)
        wp = torch.randn(2 * k * k, C, 1, 1, generator=g) / C ** 0.5
        off = F.conv2d(feat, wp)
    else:
        off = (torch.rand(B, 2 * k * k, H, W, generator=g) - 0.5) * 2 * scale
    return x, off, w, b


def _forward_check(x, off, w, b, cl=True, want_kernel="dc_fwd_mfma", padding=1, stride=1, dilation=1):
    dc = _ops()
    xd = x.to(DEV)
    if cl:
        xd = xd.contiguous(memory_format=torch.channels_last)
    got = dc.deform_conv2d(xd, off.to(DEV), w.to(DEV), b.to(DEV), stride=stride, padding=padding, dilation=dilation)
    torch.cuda.synchronize()
    assert dc.last_kernel() == want_kernel
    want = oracle(x, off, w, b, stride, padding, dilation)
    err = (got.cpu().double() - want).abs()
    bar = fp32_bar(x, off, w, stride, padding, dilation)
    assert (err <= bar).all(), (err.max().item(), (err / bar).max().item())
    case = _case_of(x, off, w, stride, padding, dilation)
    if x.shape[1] * off.shape[1] * off.shape[0] * off.shape[2] * off.shape[3] <= 1 << 22:   # the per-element bar's operands fit
        bar = cases.bars(case, x, off, w, b, torch.zeros(got.shape))["out"]
        print(f"DCBAR {want_kernel} forward {tuple(x.shape)} out={(err / bar).max().item():.4f}")
        assert (err <= bar).all(), (err.max().item(), (err / bar).max().item())
    return got


def test_mini_forward_mfma_route():
    x, off, w, b = _case(32, 32, 24, 72, 1, model_like=True)
    _forward_check(x, off, w, b, cl=True)
    _forward_check(x, off, w, b, cl=False)          # NCHW: transposed to channel-last, then the same kernel


def test_odd_channels_take_the_generic_route():
    x, off, w, b = _case(5, 7, 13, 17, 2, scale=3.0)
    _forward_check(x, off, w, b, cl=True, want_kernel="dc_fwd_generic")
    _forward_check(x, off, w, b, cl=False, want_kernel="dc_fwd_generic")
    x, off, w, b = _case(48, 40, 13, 17, 3, scale=3.0)          # C_out % 32 != 0
    _forward_check(x, off, w, b, cl=True, want_kernel="dc_fwd_generic")
    # stride / dilation and two offset groups
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 6, 11, 9, generator=g)
    w = torch.randn(4, 6, 3, 3, generator=g)
    off = (torch.rand(2, 36, 5, 4, generator=g) - 0.5) * 4
    _forward_check(x, off, w, torch.zeros(4), cl=False, want_kernel="dc_fwd_generic", padding=1, stride=2, dilation=2)


def test_wildtrack_camera_model_like_offsets():
    x, off, w, b = _case(128, 128, 120, 360, 5, model_like=True)
    _forward_check(x, off, w, b)


def test_wildtrack_camera_large_offsets():
    x, off, w, b = _case(128, 128, 120, 360, 6, scale=20.0)
    _forward_check(x, off, w, b)


def test_c16_mfma_route_and_batch():
    x, off, w, b = _case(16, 64, 9, 31, 7, scale=2.0, B=3)
    _forward_check(x, off, w, b)


def test_zero_offsets_match_conv2d_on_the_device():
    dc = _ops()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 64, 20, 30, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(96, 64, 3, 3, generator=g) / 24).to(DEV)
    b = torch.randn(96, generator=g).to(DEV)
    got = dc.deform_conv2d(x, torch.zeros(2, 18, 20, 30, device=DEV), w, b, padding=1)
    assert dc.last_kernel() == "dc_fwd_mfma"
    want = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    bar = EPS32 * (64 * 9 + 8) * F.conv2d(x.double().abs(), w.double().abs(), None, padding=1) + 1e-6
    assert ((got.double() - want).abs() <= bar).all()


def _case_of(x, off, w, stride, padding, dilation):
    pair = lambda v: (v, v) if isinstance(v, int) else tuple(v)                                          # noqa: E731
    Co, C, kh, kw = w.shape
    return cases.Case("adhoc", kh, kw, pair(stride), pair(padding), pair(dilation), C, Co, x.shape[2], x.shape[3], x.shape[0],
                      off.shape[1] // (2 * kh * kw))


def _grad_check(x, off, w, b, cl, want_kernel, stride=1, padding=1, dilation=1):
    """All four gradients for a random grad_out of the output's shape, every element inside its bar."""
    case = _case_of(x, off, w, stride, padding, dilation)
    assert tuple(off.shape[2:]) == case.out_hw
    g = torch.Generator().manual_seed(11)
    gout = torch.randn(x.shape[0], w.shape[0], *case.out_hw, generator=g)
    got = _run(case, (x, off, w, b, gout), torch.float32, cl, want_kernel[len("dc_bwd_"):])
    want = with_grads(x, off, w, b, gout, **case.conf)
    mask = cases.smooth_mask(case, off)
    assert mask.float().mean().item() >= 0.99
    check_against_oracle(f"{want_kernel} {tuple(x.shape)}", got, want, cases.bars(case, x, off, w, b, gout), torch.float32,
                         cases.tap_mask_to_channels(mask))


def _run(case, inputs, dtype, cl, route):
    """Forward and backward on the device with both routes pinned; (out, grad_input, grad_offset, grad_weight, grad_bias)."""
    dc = _ops()
    x, off, w, b, gout = (t.to(dtype).to(DEV) for t in inputs)
    if cl:
        x = x.contiguous(memory_format=torch.channels_last)
    leaves = [t.detach().requires_grad_(True) for t in (x, off, w, b)]
    out = dc.deform_conv2d(*leaves, **case.conf)
    torch.cuda.synchronize()
    assert dc.last_kernel() == f"dc_fwd_{route}"
    out.backward(gout)
    torch.cuda.synchronize()
    assert dc.last_kernel() == f"dc_bwd_{route}"
    return (out.detach(),) + tuple(t.grad for t in leaves)


def _matrix_check(name, kind, dtype, cl, route):
    case = cases.by_name(name)
    inputs, want, bar = matrix_reference(name, kind)
    mask = cases.tap_mask_to_channels(cases.smooth_mask(case, inputs[1])) if kind == "random" else None
    got = _run(case, inputs, dtype, cl, route)
    check_against_oracle(f"{route} {'cl' if cl else 'nchw'} {kind} {name}", got, want, bar, dtype, mask)


@pytest.mark.parametrize("name", [c.name for c in cases.MFMA_CASES])
def test_matrix_mfma_route_channel_last(name):
    _matrix_check(name, "random", torch.float32, True, "mfma")


@pytest.mark.parametrize("name", ["k3_default", "k5x3_aniso", "k3_s2_rem_c16", "k3_d2_c160", "k3_s2_tiny"])
def test_matrix_mfma_route_nchw_input_is_transposed_first(name):
    _matrix_check(name, "random", torch.float32, False, "mfma")


@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "cl"])
@pytest.mark.parametrize("name", [c.name for c in cases.GENERIC_CASES])
def test_matrix_generic_route_fp32_twins(name, cl):
    _matrix_check(name, "random", torch.float32, cl, "generic")


@pytest.mark.parametrize("name,cl", [(c.name, i % 2 == 1) for i, c in enumerate(cases.MATRIX)],
                         ids=[f"{c.name}-{'cl' if i % 2 else 'nchw'}" for i, c in enumerate(cases.MATRIX)])
def test_matrix_generic_route_fp64(name, cl):
    """fp64 takes the generic kernels on every shape, the MFMA cases' included; the layout alternates over the matrix."""
    _matrix_check(name, "random", torch.float64, cl, "generic")


@pytest.mark.parametrize("name", [c.name for c in cases.DYADIC_CASES])
def test_dyadic_offsets_without_a_mask_on_both_routes(name):
    case = cases.by_name(name)
    on_integer, on_minus_one, on_far_edge = cases.on_grid(case, matrix_reference(name, "dyadic")[0][1])
    assert on_integer > 0 and on_minus_one > 0 and on_far_edge > 0
    _matrix_check(name, "dyadic", torch.float32, True, "generic" if "generic" in name else "mfma")


@pytest.mark.parametrize("name", NONFINITE_IDS)
def test_nonfinite_and_huge_offsets_sample_zero_on_both_routes(name):
    """NaN, +-inf and +-1e9 offsets: dc_foot forms no index before its `in` guard, so such a tap samples 0, the result is
    finite and equals the oracle's with the tap far outside, and the tap's offset gradient is 0."""
    case = cases.by_name(name)
    route = "generic" if "generic" in name else "mfma"
    got = _run(case, nonfinite_reference(name)[0], torch.float32, True, route)
    check_nonfinite(f"{route} nonfinite {name}", got, name, torch.float32)


def test_gradients_mfma_route():
    x, off, w, b = _case(128, 128, 18, 40, 12, model_like=True)
    _grad_check(x, off, w, b, cl=True, want_kernel="dc_bwd_mfma")
    x, off, w, b = _case(160, 64, 10, 21, 13, scale=4.0)          # two channel blocks (C > 128), C_in % 32 == 0
    _grad_check(x, off, w, b, cl=False, want_kernel="dc_bwd_mfma")
    x, off, w, b = _case(48, 32, 9, 14, 14, scale=4.0, B=2)       # C_in % 32 == 16, batch 2
    _grad_check(x, off, w, b, cl=True, want_kernel="dc_bwd_mfma")


def test_gradients_generic_route():
    x, off, w, b = _case(5, 7, 9, 11, 15, scale=3.0)
    _grad_check(x, off, w, b, cl=False, want_kernel="dc_bwd_generic")
    _grad_check(x, off, w, b, cl=True, want_kernel="dc_bwd_generic")


def test_device_fp64_gradcheck():
    dc = _ops()
    g = torch.Generator().manual_seed(16)
    x = torch.randn(1, 3, 5, 6, generator=g, dtype=torch.float64).to(DEV).requires_grad_(True)
    w = torch.randn(2, 3, 3, 3, generator=g, dtype=torch.float64).to(DEV).requires_grad_(True)
    b = torch.randn(2, generator=g, dtype=torch.float64).to(DEV).requires_grad_(True)
    frac = 0.2 + 0.6 * torch.rand(1, 18, 5, 6, generator=g, dtype=torch.float64)
    off = (torch.randint(-2, 2, (1, 18, 5, 6), generator=g).double() + frac).to(DEV).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, o, ww, bb: dc.deform_conv2d(a, o, ww, bb, padding=1), (x, off, w, b),
                                    eps=1e-6, atol=1e-6, nondet_tol=1e-12)


def test_channel_last_input_is_read_in_place_and_matches_nchw(monkeypatch):
    dc = _ops()
    x, off, w, b = (t.to(DEV) for t in _case(64, 64, 15, 22, 17, scale=2.0))
    calls = []
    real = dc._transpose
    monkeypatch.setattr(dc, "_transpose", lambda *a: calls.append(a) or real(*a))
    xc = x.contiguous(memory_format=torch.channels_last)
    a = dc.deform_conv2d(xc, off, w, b, padding=1)
    assert calls == [] and dc.last_kernel() == "dc_fwd_mfma"
    nchw = dc.deform_conv2d(x, off, w, b, padding=1)
    assert len(calls) == 1 and dc.last_kernel() == "dc_fwd_mfma"
    assert torch.equal(a, nchw)


def test_side_stream_and_inputs_unchanged():
    dc = _ops()
    x, off, w, b = (t.to(DEV) for t in _case(32, 64, 12, 20, 18, scale=2.0))
    x = x.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    keep = [t.detach().clone() for t in (x, off, w, b)]
    ref = dc.deform_conv2d(x, off, w, b, padding=1).detach()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch.cuda._sleep(2_000_000)                      # the side stream is busy: a launch on the default one would race
        out = dc.deform_conv2d(x, off, w, b, padding=1)
        out.sum().backward()
    s.synchronize()
    assert torch.equal(out.detach(), ref)
    for t, k in zip((x, off, w, b), keep):
        assert torch.equal(t.detach(), k)
    assert torch.isfinite(x.grad).all() and x.grad.abs().sum().item() > 0


def test_mini_deform_conv_model_gpu_matches_cpu():
    from mvdetr_amd import geometry
    from mvdetr_amd.model import build_model
    g = torch.Generator().manual_seed(3)
    imgs = torch.randn(1, 3, 3, *geometry.MINI.input_img_shape, generator=g)
    M = geometry.random_affine_mats(1, 3, geometry.MINI.input_img_shape, seed=2, translate=0.05, scale=(0.9, 1.1))
    cpu = build_model("mini", seed=0, world_feat_arch="deform_conv", channels_last=False).eval()
    gpu = build_model("mini", seed=0, world_feat_arch="deform_conv").to(DEV).eval()
    with torch.no_grad():
        feat = cpu.features(imgs)
        proj = cpu.frame_proj_mats(M)
        want = cpu.hot_path(feat, proj)
        got = gpu.hot_path(feat.to(DEV), proj.to(DEV))
        assert _ops().last_kernel() == "dc_fwd_mfma"
    err = (got.cpu() - want).abs().max().item()
    assert err <= 1e-4 * max(1.0, want.abs().max().item()), err
