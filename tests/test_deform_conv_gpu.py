"""Deformable convolution on the MI355X: the MFMA implicit-GEMM route and the generic kernels against the fp64 restatement
(tests/deform_conv_oracle.py), the route pinned by last_kernel, and the deform_conv model on the GPU vs the CPU.

Bars: forward per element from the fp32 error model of tests/test_deform_conv.py (fp32_bar).  Gradients per tensor:
2^-24 * (chain length + position term) * the largest bound of the same quantity with |.| operands, where taps within 1e-4 px
of an integer coordinate or of the -1 / H edge are masked out of the offset-gradient comparison (the derivative is one-sided
there)."""
import pytest
import torch
import torch.nn.functional as F

from deform_conv_oracle import positions, with_grads
from deform_conv_oracle import deform_conv2d as oracle
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


def _smooth_mask(off, k, H, W, tol=1e-4):
    """[B, T, Ho, Wo] True where the tap's y and x are more than tol px from an integer and from the -1 / H edges."""
    y, x = positions(off, k, k, 1, 1, 1)

    def ok(v, n):
        frac = v - torch.floor(v)
        return (frac > tol) & (frac < 1 - tol) & ((v + 1).abs() > tol) & ((v - n).abs() > tol)
    return ok(y, H) & ok(x, W)


def _grad_check(x, off, w, b, cl, want_kernel):
    dc = _ops()
    k = w.shape[-1]
    Co, C = w.shape[:2]
    H, W = x.shape[-2:]
    g = torch.Generator().manual_seed(11)
    gout = torch.randn(x.shape[0], Co, H, W, generator=g)
    xd = x.to(DEV)
    if cl:
        xd = xd.contiguous(memory_format=torch.channels_last)
    leaves = [t.detach().requires_grad_(True) for t in (xd, off.to(DEV), w.to(DEV), b.to(DEV))]
    dc.deform_conv2d(*leaves, padding=1).backward(gout.to(DEV))
    torch.cuda.synchronize()
    assert dc.last_kernel() == want_kernel
    _, gi, go, gw, gb = with_grads(x, off, w, b, gout, padding=1)
    # bounds with |.| operands: the same gradients of sum(|gout| * out(|x|, |w|)) are sums of non-negative terms
    _, bi, _, bw, _ = with_grads(x.abs(), off, w.abs(), b, gout.abs(), padding=1)
    reach = 2 * (H + W + 2 * float(off.abs().max()) + 2 * k)
    xmax = float(x.abs().max())
    gcol_abs = torch.einsum("okt,bohw->bkthw", w.double().abs().reshape(Co, C, k * k), gout.double().abs())
    # grad_input: a K = C_out chain per g_col, <= 4 k^2 corner contributions per element, each corner weight off by the
    # rounded position
    checks = [("input", leaves[0].grad, gi, (Co + 16) * bi.abs().max() + reach * 4 * k * k * gcol_abs.max()),
              ("weight", leaves[2].grad, gw, (H * W * x.shape[0] + 8) * bw.abs().max() + reach * xmax * float(gout.abs().sum())),
              ("bias", leaves[3].grad, gb, H * W * x.shape[0] * gout.abs().max())]
    # offset gradient: sum over C of g_col * d sample / d pos, |g_col| <= sum_o |w| |gout|, |d sample / d pos| <= 2 max|x|
    boff = 2 * xmax * gcol_abs.sum(1).max()
    mask = _smooth_mask(off, k, H, W)
    got_off = leaves[1].grad.cpu().double()
    for d in (0, 1):
        checks.append((f"offset[{d}]", got_off[:, d::2][mask], go[:, d::2][mask], (Co + C + 16 + reach) * boff))
    for name, got, want, bound in checks:
        err = (got.cpu().double() - want).abs().max().item()
        assert err <= EPS32 * float(bound), (name, err, EPS32 * float(bound))
        assert want.abs().max().item() > 0, name


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
