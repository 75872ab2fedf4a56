"""Deformable convolution (torchvision.ops.deform_conv2d v1) on the library's host path, the DeformConv2d module, the
DeformConvWorldFeat aggregator and MVDeTr(world_feat_arch="deform_conv") on CPU tensors.

fp32 bars follow the error of the fp32 arithmetic: a sum of K = C_in * kh * kw products accumulated in order errs by
about K * 2^-24 * sum|w * sample|; each bilinear sample adds a few roundings of its own (+8 below); the fp32 sampling
position y = (h * s - p + i * d) + dy is rounded once, 2^-24 * |y| px, which moves a sample by at most that times
|v_hi - v_lo| <= 2 max|x| per axis."""
import inspect
import math

import pytest
import torch
import torch.nn.functional as F

from deform_conv_oracle import deform_conv2d as oracle
from deform_conv_oracle import with_grads

EPS32 = 2.0 ** -24


def fp32_bar(x, off, w, stride, padding, dilation):
    """Per-element bound of |fp32 result - exact| (module docstring)."""
    Co, C, kh, kw = w.shape
    K = C * kh * kw
    S = oracle(x.abs(), off, w.abs(), None, stride, padding, dilation)
    H, W = x.shape[-2:]
    reach = H + W + 2 * float(off.abs().max()) + 2 * kh * max(dilation if isinstance(dilation, int) else max(dilation), 1)
    pos = 2 * reach * float(x.abs().max()) * w.double().abs().sum((1, 2, 3))[None, :, None, None]
    return EPS32 * ((K + 8) * S + pos)


def _lib_op():
    from mvdetr_amd.ops import deform_conv2d
    return deform_conv2d


def test_public_names_exist():
    from mvdetr_amd.ops import DeformConv2d, deform_conv2d  # noqa: F401
    from mvdetr_amd.world_feat import DeformConvWorldFeat  # noqa: F401


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("k,stride,padding,dilation,cin", [
    (1, 1, 0, 1, 3), (3, 1, 1, 1, 16), (3, 2, 1, 1, 32), (3, 1, 2, 2, 16), (5, 1, 2, 1, 3), (5, 2, 3, 2, 32), (3, (1, 2), (0, 1), (2, 1), 3),
])
def test_zero_offsets_are_conv2d(dtype, k, stride, padding, dilation, cin):
    """Known answer (a): zero offsets give F.conv2d, and so do the input, weight and bias gradients."""
    op = _lib_op()
    g = torch.Generator().manual_seed(cin * 7 + k)
    x = torch.randn(2, cin, 11, 13, generator=g, dtype=dtype)
    w = torch.randn(8, cin, k, k, generator=g, dtype=dtype) / math.sqrt(cin * k * k)
    b = torch.randn(8, generator=g, dtype=dtype)
    want = F.conv2d(x.double(), w.double(), b.double(), stride, padding, dilation)
    off = torch.zeros(2, 2 * k * k, *want.shape[-2:], dtype=dtype)
    xs, ws, bs = (t.clone().requires_grad_(True) for t in (x, w, b))
    got = op(xs, off, ws, bs, stride=stride, padding=padding, dilation=dilation)
    gout = torch.randn(got.shape, generator=g, dtype=dtype)
    got.backward(gout)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    F.conv2d(xr, wr, br, stride, padding, dilation).backward(gout.double())
    if dtype == torch.float64:
        tol = dict(atol=1e-12, rtol=1e-12)
        assert torch.allclose(got.double(), want, **tol)
    else:
        assert ((got.double() - want).abs() <= fp32_bar(x, off, w, stride, padding, dilation)).all()
        tol = dict(atol=2e-5, rtol=1e-5)
    assert torch.allclose(xs.grad.double(), xr.grad, **tol)
    assert torch.allclose(ws.grad.double(), wr.grad, **tol)
    assert torch.allclose(bs.grad.double(), br.grad, **tol)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("k,padding,dy,dx", [(3, 1, 2, -1), (3, 0, -3, 4), (1, 0, 1, 1), (5, 2, -2, 0)])
def test_integer_offset_is_an_index_shift(dtype, k, padding, dy, dx):
    """Known answer (b): the same integer offset at every pixel and tap is conv2d (padding 0) of the zero-padded input,
    sliced so that its pixel (0, 0) is input pixel (dy - p, dx - p) -- not conv2d of a shifted input with the original
    padding (a tap in the padding still samples the image when it lands inside)."""
    op = _lib_op()
    g = torch.Generator().manual_seed(k * 10 + dy)
    C, H, W = 3, 9, 10
    x = torch.randn(1, C, H, W, generator=g, dtype=dtype)
    w = torch.randn(4, C, k, k, generator=g, dtype=dtype)
    Ho, Wo = H + 2 * padding - k + 1, W + 2 * padding - k + 1
    off = torch.empty(1, 2 * k * k, Ho, Wo, dtype=dtype)
    off[:, 0::2], off[:, 1::2] = dy, dx
    P = 32
    big = F.pad(x.double(), (P, P, P, P))
    y0, x0 = dy - padding + P, dx - padding + P
    want = F.conv2d(big[..., y0:y0 + Ho + k - 1, x0:x0 + Wo + k - 1], w.double())
    got = op(x, off, w, padding=padding)
    assert got.shape == want.shape
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    assert (got.double() - want).abs().max().item() <= tol * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("cl", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_fractional_offsets_match_the_oracle(dtype, cl):
    """Random fractional offsets, many taps outside the image and straddling the -1 / H edges, NCHW and channel-last."""
    op = _lib_op()
    g = torch.Generator().manual_seed(5)
    C, H, W, Co = 16, 10, 12, 8
    x = torch.randn(2, C, H, W, generator=g, dtype=dtype)
    w = torch.randn(Co, C, 3, 3, generator=g, dtype=dtype) / 12
    b = torch.randn(Co, generator=g, dtype=dtype)
    off = (torch.rand(2, 18, H, W, generator=g, dtype=dtype) - 0.5) * 8
    off[:, :, 0, :] = -1.0 + 1e-3 * torch.rand(2, 18, W, generator=g, dtype=dtype)   # straddle the y = -1 edge
    if cl:
        x = x.contiguous(memory_format=torch.channels_last)
    got = op(x, off, w, b, padding=1)
    want = oracle(x, off, w, b, 1, 1, 1)
    err = (got.double() - want).abs()
    if dtype == torch.float64:
        assert err.max().item() < 1e-12
    else:
        assert (err <= fp32_bar(x, off, w, 1, 1, 1)).all(), err.max().item()


def test_offset_groups_match_the_oracle():
    op = _lib_op()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, 6, 7, 8, generator=g, dtype=torch.float64)
    w = torch.randn(5, 6, 3, 3, generator=g, dtype=torch.float64)
    off = (torch.rand(1, 3 * 18, 4, 4, generator=g, dtype=torch.float64) - 0.5) * 3
    got = op(x, off, w, None, stride=2, padding=1, dilation=1)
    assert (got - oracle(x, off, w, None, 2, 1, 1)).abs().max().item() < 1e-12


def test_gradients_match_the_oracle():
    op = _lib_op()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(1, 4, 6, 7, generator=g, dtype=torch.float64)
    w = torch.randn(3, 4, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(3, generator=g, dtype=torch.float64)
    off = (torch.rand(1, 36, 6, 7, generator=g, dtype=torch.float64) - 0.5) * 5        # 2 offset groups
    gout = torch.randn(1, 3, 6, 7, generator=g, dtype=torch.float64)
    leaves = [t.clone().requires_grad_(True) for t in (x, off, w, b)]
    op(*leaves, padding=1).backward(gout)
    want = with_grads(x, off, w, b, gout, padding=1)
    for got_t, want_t in zip(leaves, want[1:]):
        assert (got_t.grad - want_t).abs().max().item() < 1e-10


def test_host_gradcheck_all_four_gradients():
    op = _lib_op()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 3, 5, 6, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(2, 3, 3, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(2, generator=g, dtype=torch.float64).requires_grad_(True)
    # fractional parts kept away from 0 / 1 (the offset gradient is one-sided at integer coordinates)
    frac = 0.2 + 0.6 * torch.rand(1, 18, 5, 6, generator=g, dtype=torch.float64)
    off = (torch.randint(-2, 2, (1, 18, 5, 6), generator=g).double() + frac).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, o, ww, bb: op(a, o, ww, bb, padding=1), (x, off, w, b), eps=1e-6, atol=1e-6)


def test_module_signature_parameters_and_init():
    from mvdetr_amd.ops import DeformConv2d
    params = list(inspect.signature(DeformConv2d.__init__).parameters)
    assert params == ["self", "in_channels", "out_channels", "kernel_size", "stride", "padding", "dilation", "groups", "bias"]
    assert list(inspect.signature(DeformConv2d.forward).parameters) == ["self", "input", "offset", "mask"]
    from mvdetr_amd.ops import deform_conv2d
    assert list(inspect.signature(deform_conv2d).parameters) == [
        "input", "offset", "weight", "bias", "stride", "padding", "dilation", "mask"]
    torch.manual_seed(0)
    m = DeformConv2d(16, 32, 3, padding=1)
    assert m.weight.shape == (32, 16, 3, 3) and m.bias.shape == (32,)
    bound = 1 / math.sqrt(16 * 9)
    assert m.weight.abs().max().item() <= bound + 1e-7 and m.bias.abs().max().item() <= bound + 1e-7
    assert m.weight.std().item() > 0.4 * bound
    assert DeformConv2d(4, 4, (1, 3), bias=False).bias is None
    x = torch.randn(1, 16, 5, 6)
    out = m(x, torch.zeros(1, 18, 5, 6))
    assert torch.allclose(out, F.conv2d(x, m.weight, m.bias, padding=1), atol=1e-5)


def test_refusals():
    from mvdetr_amd.ops import DeformConv2d, deform_conv2d
    x, w = torch.randn(1, 4, 5, 5), torch.randn(2, 4, 3, 3)
    off = torch.zeros(1, 18, 3, 3)
    with pytest.raises(NotImplementedError):
        deform_conv2d(x, off, w, mask=torch.ones(1, 9, 3, 3))
    with pytest.raises(NotImplementedError):
        deform_conv2d(x, off, torch.randn(2, 2, 3, 3))
    with pytest.raises(NotImplementedError):
        DeformConv2d(4, 4, 3, groups=2)
    with pytest.raises(NotImplementedError):
        DeformConv2d(4, 4, 3)(x, torch.zeros(1, 18, 3, 3), mask=torch.ones(1, 9, 3, 3))
    with pytest.raises(RuntimeError, match="mvdetr_ops"):
        deform_conv2d(x.half(), off.half(), w.half())
    with pytest.raises(RuntimeError, match="mvdetr_ops"):
        deform_conv2d(x.bfloat16(), off.bfloat16(), w.bfloat16())
    with pytest.raises(RuntimeError):
        deform_conv2d(x, torch.zeros(1, 17, 3, 3), w)                    # not a multiple of 2 kh kw
    with pytest.raises(RuntimeError):
        deform_conv2d(x, torch.zeros(1, 18, 4, 4), w)                    # wrong output size
    with pytest.raises(RuntimeError):
        deform_conv2d(x, torch.zeros(1, 18, 3, 3), w.double())           # mixed dtypes


REFERENCE_KEYS = (
    # conv_world_feat.py:58-64: deform_pos[n] = Conv2d(base, 18, 1), deform_conv[n] = DeformConv2d(base, base, 3, padding=1),
    # merge_linear = Sequential(Conv2d(base * N, hidden, 1), ReLU), world_feat = Sequential(3 x (Conv2d, ReLU)); the position
    # embedding is a plain attribute (not in the state dict)
    [f"deform_pos.{n}.{p}" for n in range(3) for p in ("weight", "bias")]
    + [f"deform_conv.{n}.{p}" for n in range(3) for p in ("weight", "bias")]
    + ["merge_linear.0.weight", "merge_linear.0.bias"]
    + [f"world_feat.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")])


def test_deform_conv_world_feat_state_dict_matches_the_reference():
    from mvdetr_amd.world_feat import DeformConvWorldFeat
    m = DeformConvWorldFeat(3, (24, 72), 32, hidden_dim=16)
    sd = m.state_dict()
    assert sorted(sd) == sorted(REFERENCE_KEYS)
    assert sd["deform_pos.0.weight"].shape == (18, 32, 1, 1)
    assert sd["deform_conv.2.weight"].shape == (32, 32, 3, 3)
    assert sd["merge_linear.0.weight"].shape == (16, 96, 1, 1)
    assert sd["world_feat.4.weight"].shape == (16, 16, 3, 3)
    assert m.pos_embedding.shape == (1, 32, 24, 72)
    m.load_state_dict({k: torch.zeros_like(v) for k, v in sd.items()}, strict=True)


def test_deform_conv_world_feat_channel_last_input_gives_the_same_result():
    from mvdetr_amd.world_feat import DeformConvWorldFeat
    torch.manual_seed(1)
    m = DeformConvWorldFeat(2, (6, 10), 16, hidden_dim=16)
    x = torch.randn(2, 2, 16, 6, 10)
    with torch.no_grad():
        a = m(x)
        b = m(x.permute(0, 1, 3, 4, 2).contiguous())
    assert a.shape == (2, 16, 6, 10)
    assert (a - b).abs().max().item() < 1e-5


def test_mini_deform_conv_model_runs_forward_and_backward_on_the_cpu():
    from mvdetr_amd import geometry
    from mvdetr_amd.model import build_model
    model = build_model("mini", seed=0, world_feat_arch="deform_conv", channels_last=False)
    g = torch.Generator().manual_seed(3)
    imgs = torch.randn(1, 3, 3, *geometry.MINI.input_img_shape, generator=g)
    M = geometry.random_affine_mats(1, 3, geometry.MINI.input_img_shape, seed=2, translate=0.05, scale=(0.9, 1.1))
    (wh, wo), (ih, io, iw) = model(imgs, M)
    assert wh.shape == (1, 1, 24, 72) and wo.shape == (1, 2, 24, 72)
    assert torch.isfinite(wh).all() and torch.isfinite(wo).all()
    (wh.square().mean() + wo.square().mean() + ih.square().mean()).backward()
    for name in ("world_feat.deform_conv.0.weight", "world_feat.deform_conv.0.bias", "world_feat.deform_pos.1.weight",
                 "world_feat.merge_linear.0.weight", "base.0.weight"):
        grad = dict(model.named_parameters())[name].grad
        assert grad is not None and torch.isfinite(grad).all() and grad.abs().sum().item() > 0, name
