"""Deformable convolution (torchvision.ops.deform_conv2d v1) on the library's host path, the DeformConv2d module, the
DeformConvWorldFeat aggregator and MVDeTr(world_feat_arch="deform_conv") on CPU tensors.

fp32 bars follow the error of the fp32 arithmetic: a sum of K = C_in * kh * kw products accumulated in order errs by
about K * 2^-24 * sum|w * sample|; each bilinear sample adds a few roundings of its own (+8 below); the fp32 sampling
position y = (h * s - p + i * d) + dy is rounded once, 2^-24 * |y| px, which moves a sample by at most that times
|v_hi - v_lo| <= 2 max|x| per axis.

The geometry matrix (tests/deform_conv_cases.py: kernels 1x1 .. 5x5 and 5x3, strides with and without a remainder,
anisotropic stride / padding / dilation, padding 0 and beyond the kernel's reach, one and two offset groups) runs the host
path in fp64 (<= 1e-10 (1 + max|want|)) and in fp32 against that module's per-element bars, for the output and all four
gradients, with +-3 px random offsets, with dyadic offsets (multiples of 1/4: no mask, taps exactly on integers, on -1 and
on H) and with NaN / inf / 1e9 offsets.  Largest host fp32 err / bar over the matrix (NCHW and channel-last, random and
dyadic): out 0.44, grad_input 0.60, grad_offset 0.56, grad_weight 0.12, grad_bias 0.27.  Every mutant of that module
exceeds every bar it touches (test_mutants_exceed_every_bar_they_touch, over elements whose bar is not 0); the smallest
margins are out 5.7x (positions shifted, k3_d2_c160), grad_input 10x and grad_offset 13x (one grad_out element dropped,
k3_default), grad_weight 9.7x (positions shifted, k3_c128_18x40) and grad_bias 140x."""
import inspect
import math

import pytest
import torch
import torch.nn.functional as F

import deform_conv_cases as cases
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


# ---- the geometry matrix on the host path ---------------------------------------------------------------------------------

CASE_IDS = [c.name for c in cases.MATRIX]


def _typed(tensors, dtype, cl):
    x, *rest = (t.to(dtype) for t in tensors)
    return [x.contiguous(memory_format=torch.channels_last) if cl else x] + rest


@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "cl"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", CASE_IDS)
def test_matrix_host_path_matches_the_oracle(name, dtype, cl):
    """Output and all four gradients over the geometry matrix with +-3 px random offsets.  The offsets must exercise full,
    partial and empty footprints, and the mask of the offset-gradient comparison (taps within 1e-4 px of an integer or of
    the -1 / H edges, where fp32 rounding can flip the floor) must keep at least 99 % of the taps."""
    case = cases.by_name(name)
    inputs, want, bar = cases.matrix_reference(name, "random")
    full, partial, outside = cases.tap_classes(case, inputs[1])
    assert full.any() and partial.any() and outside.any(), (int(full.sum()), int(partial.sum()), int(outside.sum()))
    keep = cases.smooth_mask(case, inputs[1])
    assert keep.float().mean().item() >= 0.99
    got = cases.run(_lib_op(), *_typed(inputs, dtype, cl), case)
    cases.check_against_oracle(f"host {name}", got, want, bar, dtype, cases.tap_mask_to_channels(keep))


@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "cl"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", [c.name for c in cases.DYADIC_CASES])
def test_dyadic_offsets_match_the_oracle_without_a_mask(name, dtype, cl):
    """Offsets that are multiples of 1/4: every position is exact in fp32, so nothing is masked -- the one-sided derivative
    at integer coordinates and the zero sample exactly on y = -1 and y = H are compared as they are."""
    case = cases.by_name(name)
    inputs, want, bar = cases.matrix_reference(name, "dyadic")
    on_integer, on_minus_one, on_far_edge = cases.on_grid(case, inputs[1])
    assert on_integer > 0 and on_minus_one > 0 and on_far_edge > 0, (on_integer, on_minus_one, on_far_edge)
    got = cases.run(_lib_op(), *_typed(inputs, dtype, cl), case)
    cases.check_against_oracle(f"host dyadic {name}", got, want, bar, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", cases.NONFINITE_IDS)
def test_nonfinite_and_huge_offsets_sample_zero(name, dtype):
    """A tap whose offset is NaN, +-inf or +-1e9 samples 0: the result is the oracle's with that tap far outside, finite
    everywhere, with a zero offset gradient at the tap."""
    case = cases.by_name(name)
    inputs = cases.nonfinite_reference(name)[0]
    assert not torch.isfinite(inputs[1]).all() and (inputs[1].abs() == 1e9).any()
    got = cases.run(_lib_op(), *_typed(inputs, dtype, False), case)
    cases.check_nonfinite(f"host nonfinite {name}", got, name, dtype)


@pytest.mark.parametrize("name", CASE_IDS + [c.name for c in cases.BAR_ONLY_CASES])
def test_mutants_exceed_every_bar_they_touch(name):
    """The bars must catch a subtly wrong implementation: each mutant (cases.MUTANTS, made from the oracle alone) errs by
    more than the bar in at least one element of every tensor it touches."""
    case = cases.by_name(name)
    inputs, want, bar = cases.matrix_reference(name, "random")
    applied = 0
    for mutant, fn in cases.MUTANTS.items():
        wrong = fn(case, *inputs)
        if wrong is None:                                  # equal to the truth by construction on this geometry
            continue
        applied += 1
        r = cases.ratios([t if m is None else m for m, t in zip(wrong, want)], want, bar, positive_bar_only=True)
        for tensor in cases.MUTANT_TOUCHES[mutant]:
            assert r[tensor] > 1.0, f"mutant {mutant} passes the {tensor} bar on {name}: err / bar = {r[tensor]:.3f}"
    assert applied >= 6


def test_every_mutant_applies_somewhere():
    for mutant, fn in cases.MUTANTS.items():
        assert any(fn(c, *cases.matrix_reference(c.name, "random")[0]) is not None for c in cases.MATRIX if c.C <= 6), mutant


def test_matrix_holds_the_geometries_and_launch_structures_it_is_for():
    """The matrix is shared with the GPU tests: what they rely on being in it is pinned here."""
    m = cases.MFMA_CASES
    assert {(c.kh, c.kw) for c in m} >= {(1, 1), (1, 3), (3, 1), (2, 2), (5, 5), (5, 3), (3, 3)}
    assert all(c.offset_groups == 1 and c.C % 16 == 0 and c.C_out % 32 == 0 for c in m)                  # the MFMA route
    assert all(c.C % 2 == 1 or c.offset_groups == 2 for c in cases.GENERIC_CASES)
    assert [c._replace(name="", C=0, C_out=0, offset_groups=0) for c in m] == \
        [c._replace(name="", C=0, C_out=0, offset_groups=0) for c in cases.GENERIC_CASES]                  # twins: same geometry
    rem = lambda c, a: (c[8 + a] + 2 * c.padding[a] - c.dilation[a] * (c[1 + a] - 1) - 1) % c.stride[a]  # noqa: E731
    assert any(c.stride == (2, 2) and rem(c, 0) for c in m) and any(c.stride == (2, 2) and not rem(c, 0) and not rem(c, 1) for c in m)
    assert any(len({c.stride[0], c.stride[1]}) == 2 and c.padding[0] != c.padding[1] and c.dilation[0] != c.dilation[1] for c in m)
    assert any(c.dilation == (2, 2) for c in m) and any(c.padding == (0, 0) for c in m)
    assert any(c.padding[0] > c.dilation[0] * (c.kh - 1) for c in m)
    assert all(c.B >= 2 and (c.out_hw[0] * c.out_hw[1]) % 32 for c in m if c.name != "k3_s2_tiny")
    assert {c.C_out for c in m} >= {160, 256} and any(c.C == 160 and c.C_out == 160 for c in m)
    assert any(c.B * c.out_hw[0] * c.out_hw[1] <= 32 for c in m)                                         # one 32-pixel chunk
    assert any(c.C == 16 and c.stride != (1, 1) for c in m)                                              # dc_fwd_mfma<16>
    assert any(c.out_hw != (c.H, c.W) for c in m)
