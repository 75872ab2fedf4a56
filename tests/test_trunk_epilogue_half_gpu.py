"""The trunk's 16-bit fused epilogues on the GPU (mvdetr_amd/csrc/trunk_epilogue.hip: bn_act_half, bn_relu_maxpool_half).

The op-level oracle is the fp64 formula on the SAME, already rounded 16-bit inputs, upcast; the bar is the 16-bit house bar
(helpers.assert_rounded_once: half an ulp of the storage type on every element plus a floor, and the correctly rounded
value on >= 99 % of them) with the floor MEASURED in the test: twice the max-abs deviation from fp64 of torch's own fp32
chain on the upcast inputs -- the fp32 test's bar.  No element is excluded.  The RMS error of the fused result and of
torch's own 16-bit chain (which rounds after every op) against fp64 are printed (run with -s).

The pool is compared with max_pool2d of the 16-bit bn_act output as raw 16-bit words: rounding to nearest is monotone, so
the max of the fp32 values, rounded, IS the max of the rounded values.

The model-level bar is the project's bar for "the HIP path's error is not above the torch composition's"
(test_half_inference_gpu.test_encoder_error_is_not_above_the_torch_compositions): per output, RMS(fused - fp32 model) <=
1.25 x RMS(unfused - fp32 model), the fp32 model holding the same rounded parameters."""
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from helpers import assert_rounded_once, ulp_of
from test_half_inference_gpu import DTYPES
from test_trunk_epilogue_gpu import _bn, _bn64, _cl, _torch_bn, _trunk_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = {"none": "bn", "identity": "bn_add", "downsample_bn": "bn_bn_add"}


@pytest.fixture(scope="module")
def te():
    from mvdetr_amd.ops import trunk_epilogue
    assert trunk_epilogue.trunk_fusion_enabled()
    return trunk_epilogue


@pytest.fixture
def deterministic_convs():
    """"torch's result bit for bit" is only defined with the deterministic convolution solvers (see the fp32 test)."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


def _raw(t):
    return t.view(torch.int16)


def _rms(a, ref64):
    return (a.double() - ref64).square().mean().sqrt().item()


def _to16(trunk, dtype):
    """What MVDeTr.to_inference does to a trunk: convolutions in 16 bits, BatchNorm left in fp32."""
    for m in trunk.modules():
        if isinstance(m, nn.Conv2d):
            m.to(dtype)
    return trunk


def _chains(x, r, bn, bn_r, relu):
    """-> fp64 oracle, torch's fp32 chain on the upcast inputs, torch's own 16-bit chain (a rounding after every op)."""
    want, c32, c16 = _bn64(bn, x), _torch_bn(bn, x.float()), _torch_bn(bn, x)
    if r is not None:
        want = want + (_bn64(bn_r, r) if bn_r is not None else r.double())
        c32 = c32 + (_torch_bn(bn_r, r.float()) if bn_r is not None else r.float())
        c16 = c16 + (_torch_bn(bn_r, r) if bn_r is not None else r)
    if relu:
        want, c32, c16 = torch.relu(want), torch.relu(c32), torch.relu(c16)
    return want, c32, c16


# ---- 1. bn_act parity ----------------------------------------------------------------------------------------------------
# (shape, what it exercises): C/8 lanes across, 256/(C/8) rows per block and step, two rows per lane in flight
SHAPES = [
    (1, 64, 7, 5),          # tiled; 35 rows, odd: the row that travels alone after the pairs
    (2, 64, 45, 79),        # tiled
    (3, 128, 1, 1),         # tiled; fewer rows than one block holds
    (1, 2048, 6, 9),        # tiled; 256 lanes across
    (1, 4096, 3, 5),        # tiled; the second blockIdx.y chunk
    (1, 2048, 65, 65),      # tiled; 4,225 rows: past the 2,048-block grid cap, the grid-stride loop turns over
    (2, 48, 9, 7),          # the flat "any" route (C/8 = 6)
    (1, 8, 33, 3),          # tiled; C/8 = 1
]
# (affine, relu, inplace): the three cover relu on / off, in place / out of place and a BatchNorm without gamma / beta
COMBOS = [(True, True, True), (True, False, False), (False, True, False)]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("mode", ["none", "identity", "downsample_bn"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bn_act_half_is_the_fp64_formula_rounded_once(te, shape, mode, dtype):
    torch.manual_seed(shape[1] + shape[2])
    x = _cl((torch.randn(shape, device=DEV) * 2).to(dtype))
    r = None if mode == "none" else _cl((torch.randn(shape, device=DEV) * 2).to(dtype))
    r_keep = None if r is None else r.clone(memory_format=torch.preserve_format)
    for affine, relu, inplace in COMBOS:
        bn = _bn(shape[1], 1, affine)
        bn_r = _bn(shape[1], 2, affine) if mode == "downsample_bn" else None
        want, c32, c16 = _chains(x, r, bn, bn_r, relu)
        floor = 2 * (c32.double() - want).abs().max().item()
        xin = x.clone(memory_format=torch.preserve_format) if inplace else x
        assert te.fused_bn_act_half_available(xin, bn, r, bn_r) and not te.fused_bn_act_available(xin, bn, r, bn_r)
        before = te.launch_count()
        got = te.bn_act_half(xin, bn, r, bn_r, relu=relu, inplace=inplace)
        assert te.launch_count() == before + 1
        assert te.last_kernel() == NAMES[mode] + ("_relu" if relu else "") + "_half"
        assert (got is xin) == inplace and got.is_contiguous(memory_format=torch.channels_last)
        rms_f, rms_t = _rms(got, want), _rms(c16, want)
        print(f"bn_act_half {dtype} {shape} {mode} affine={affine} relu={relu} inplace={inplace}: floor {floor:.3e}; RMS vs fp64: "
              f"fused {rms_f:.4e}, torch's 16-bit chain {rms_t:.4e} (ratio {rms_f / rms_t:.3f})")
        assert_rounded_once(got, want.cpu(), dtype, floor)
        if not inplace:
            assert torch.equal(_raw(xin), _raw(x))
        if r is not None:
            assert torch.equal(_raw(r), _raw(r_keep))                  # (the residual is read only)


# ---- 2. non-finite values and overflow -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("mode", ["none", "identity", "downsample_bn"])
def test_bn_act_half_non_finite_and_overflow(te, mode, dtype):
    torch.manual_seed(11)
    shape = (1, 64, 5, 7)
    x = (torch.randn(shape, device=DEV) * 2).to(dtype)
    r = (torch.randn(shape, device=DEV) * 2).to(dtype)
    x[0, 3, 1, 2], x[0, 4, 0, 0], x[0, 5, 4, 6] = float("nan"), float("inf"), float("-inf")
    r[0, 8, 2, 2], r[0, 9, 3, 3], r[0, 10, 0, 6] = float("nan"), float("inf"), float("-inf")
    # finite inputs whose result leaves float16's range (gamma / sqrt(var + eps) > 0.28 with these vectors): x alone, the
    # residual alone, and two halves that only overflow together
    x[0, 20, 1, 1], r[0, 21, 2, 3] = 60000.0, 60000.0
    x[0, 22, 3, 4], r[0, 22, 3, 4] = 40000.0, 40000.0
    x[0, 23, 0, 5] = -60000.0
    x, r = _cl(x), _cl(r)
    if mode == "none":
        r = None
    bn = _bn(64, 3)
    with torch.no_grad():
        bn.weight[20], bn.running_var[20] = 1.5, 0.25                     # scale 3 in channel 20: 60,000 becomes 180,000
    bn_r = _bn(64, 6) if mode == "downsample_bn" else None
    for relu in (True, False):
        want, c32, _ = _chains(x, r, bn, bn_r, relu)
        got = te.bn_act_half(x, bn, r, bn_r, relu=relu)
        want16 = want.to(dtype)
        odd = ~got.isfinite() | ~want16.isfinite()
        assert torch.equal(got.isnan(), want16.isnan()) and got.isnan().any()
        assert torch.equal(got[odd & ~got.isnan()], want16[odd & ~got.isnan()])      # +-inf where, and only where, fp64 rounds to it
        assert got.isinf().any() and (relu or (got == float("-inf")).any())
        if dtype == torch.float16:
            inputs_finite = x.isfinite() if r is None else x.isfinite() & r.isfinite()
            assert (got.isinf() & inputs_finite).any()                                # an overflow, not a passed-on inf
        if relu:
            assert got[0, 5, 4, 6] == 0 and got[0, 23, 0, 5] == 0
        ok = ~odd
        floor = 2 * (c32.double() - want)[ok].abs().max().item()
        assert_rounded_once(got[ok], want[ok].cpu(), dtype, floor)


# ---- 3. the stem's pool ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(1, 64, 7, 5), (3, 128, 1, 1), (1, 2048, 6, 9), (1, 64, 2, 640), (2, 64, 45, 79)],
                         ids=lambda s: "x".join(map(str, s)))
def test_bn_relu_maxpool_half_is_the_pool_of_bn_act_half_bit_for_bit(te, shape, dtype):
    torch.manual_seed(shape[2])
    bn = _bn(shape[1], 4)
    x = (torch.randn(shape, device=DEV) * 2).to(dtype)
    N, C, H, W = shape
    x[:, 9] = -x[:, 9].abs() - 10                                         # a channel negative everywhere: every window is relu's 0
    x[0, 1, 0, 0], x[-1, 2, H - 1, W - 1], x[0, 3, H // 2, W // 2] = float("nan"), float("inf"), float("-inf")
    x[0, 5, H - 1, 0], x[0, 6, 0, W - 1], x[0, 7, H // 2, 0] = float("nan"), float("nan"), float("inf")
    x = _cl(x)
    assert te.fused_bn_relu_maxpool_half_available(x, bn, nn.ReLU(), nn.MaxPool2d(3, 2, 1))
    assert not te.fused_bn_relu_maxpool_available(x, bn, nn.ReLU(), nn.MaxPool2d(3, 2, 1))
    before = te.launch_count()
    got = te.bn_relu_maxpool_half(x, bn)
    assert te.last_kernel() == "bn_relu_maxpool_half" and te.launch_count() == before + 1
    want = F.max_pool2d(te.bn_act_half(x, bn, relu=True), 3, 2, 1)
    assert got.dtype == dtype and got.shape == want.shape == (N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert want.isnan().any() and want.isinf().any() and (want[:, 9] == 0).all()
    assert torch.equal(_raw(got), _raw(_cl(want)))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_96_channel_stem_keeps_torchs_three_ops(te, dtype, deterministic_convs):
    """C / 8 = 12 does not tile the pool's block: the predicate refuses, and ResNetTrunk runs BatchNorm, ReLU and MaxPool2d."""
    from mvdetr_amd.model import ResNetTrunk
    torch.manual_seed(3)
    stem = _to16(ResNetTrunk(nn.Conv2d(3, 96, 7, 2, 3, bias=False), nn.BatchNorm2d(96), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2, 1)), dtype)
    stem = stem.to(DEV).eval()
    img = _cl(torch.randn(1, 3, 32, 32, device=DEV).to(dtype))
    with torch.no_grad():
        mid = stem[0](img)
        assert not te.fused_bn_relu_maxpool_half_available(mid, stem[1], stem[2], stem[3])
        assert te.fused_bn_act_half_available(mid, stem[1])               # (bn_act's flat route would take 96 channels)
        before = te.launch_count()
        got = stem(img)
        assert te.launch_count() == before
        assert torch.equal(_raw(got), _raw(stem[3](stem[2](stem[1](stem[0](img))))))


# ---- 4. never written ------------------------------------------------------------------------------------------------------
def _trunk16(depth, dtype, seed=0):
    from mvdetr_amd.model import resnet_trunk
    torch.manual_seed(seed)
    trunk = resnet_trunk(depth)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in trunk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    return _to16(trunk, dtype).to(DEV).eval()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("depth", [18, 50])
def test_the_block_input_and_the_callers_tensor_are_never_written(te, depth, dtype):
    """BasicBlocks (layer2's first has a downsample branch) and Bottlenecks (layer1's first has one)."""
    trunk = _trunk16(depth, dtype, 1)
    per_block = 2 if depth == 18 else 3
    x = _cl(torch.randn(1, 3, 64, 64, device=DEV).to(dtype))
    x_keep = x.clone(memory_format=torch.preserve_format)
    with torch.no_grad():
        mid = trunk[3](trunk[2](trunk[1](trunk[0](x))))
        seen_downsample = 0
        for layer in (trunk[4], trunk[5]):
            for b in layer:
                seen_downsample += b.downsample is not None
                keep = mid.clone(memory_format=torch.preserve_format)
                before = te.launch_count()
                out = b(mid)
                assert te.launch_count() == before + per_block and out.data_ptr() != mid.data_ptr()
                assert te.last_kernel() == ("bn_bn_add_relu_half" if b.downsample is not None else "bn_add_relu_half")
                assert torch.equal(_raw(mid), _raw(keep))
                mid = out
        assert seen_downsample >= 1
    assert torch.equal(_raw(x), _raw(x_keep))


# ---- 5. predicates ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_half_predicates(te, dtype):
    bn = _bn(64, 5)
    x = _cl(torch.randn(1, 64, 8, 8, device=DEV).to(dtype))
    other = _cl(torch.randn(1, 64, 8, 8, device=DEV).to(dtype))
    relu, pool = nn.ReLU(), nn.MaxPool2d(3, 2, 1)
    assert te.fused_bn_act_half_available(x, bn) and te.fused_bn_act_half_available(x, bn, other)
    assert te.fused_bn_act_half_available(x, bn, other, _bn(64, 6)) and te.fused_bn_relu_maxpool_half_available(x, bn, relu, pool)
    # a BatchNorm cast to 16 bits (model.half()): torch's ops
    bn16 = copy.deepcopy(bn).to(dtype)
    assert not te.fused_bn_act_half_available(x, bn16) and not te.fused_bn_relu_maxpool_half_available(x, bn16, relu, pool)
    assert not te.fused_bn_act_half_available(x, bn, other, bn16)
    # mixed dtypes
    wrong = torch.bfloat16 if dtype == torch.float16 else torch.float16
    assert not te.fused_bn_act_half_available(x, bn, other.to(wrong)) and not te.fused_bn_act_half_available(x, bn, other.float())
    # C = 12: a multiple of 4 (the fp32 kernels' rule), not of 8
    x12 = _cl(torch.randn(1, 12, 8, 8, device=DEV).to(dtype))
    assert not te.fused_bn_act_half_available(x12, _bn(12, 5))
    assert te.fused_bn_act_available(x12.float(), _bn(12, 5))
    assert not te.fused_bn_act_half_available(x.contiguous(), bn)                                 # NCHW
    assert not te.fused_bn_act_half_available(x[..., ::2], bn)                                    # a strided view
    assert not te.fused_bn_act_half_available(x, bn, x)                                           # the residual is the output
    base = torch.randn(1, 8 * 8 + 8, 64, device=DEV).to(dtype)                                    # two dense NHWC tensors, overlapping storage
    a, b = base[:, :64].view(1, 8, 8, 64).permute(0, 3, 1, 2), base[:, 8:].view(1, 8, 8, 64).permute(0, 3, 1, 2)
    assert a.is_contiguous(memory_format=torch.channels_last) and not te.fused_bn_act_half_available(a, bn, b)
    assert not te.fused_bn_act_half_available(b, bn, a) and te.fused_bn_act_half_available(a, bn, x)
    assert not te.fused_bn_act_half_available(x, copy.deepcopy(bn).train())                       # train mode
    assert not te.fused_bn_relu_maxpool_half_available(x, copy.deepcopy(bn).train(), relu, pool)
    with torch.enable_grad():                                                                     # grad required
        assert te.fused_bn_act_half_available(x, bn)
        assert not te.fused_bn_act_half_available(x, copy.deepcopy(bn).requires_grad_(True))
        assert not te.fused_bn_act_half_available(x.clone(memory_format=torch.preserve_format).requires_grad_(True), bn)
        assert not te.fused_bn_act_half_available(x, bn, other.clone(memory_format=torch.preserve_format).requires_grad_(True))
    prev = te.set_trunk_fusion(False)                                                             # the switch
    try:
        assert not te.fused_bn_act_half_available(x, bn) and not te.fused_bn_relu_maxpool_half_available(x, bn, relu, pool)
        with pytest.raises(RuntimeError, match="fused kernel"):
            te.bn_act_half(x, bn)
    finally:
        te.set_trunk_fusion(prev)
    with pytest.raises(RuntimeError, match="fused kernel"):                                       # the ops raise, nothing falls back
        te.bn_act_half(x, bn16)
    with pytest.raises(RuntimeError, match="fused kernel"):
        te.bn_relu_maxpool_half(x12, _bn(12, 5))
    assert not te.fused_bn_act_available(x, bn) and not te.fused_bn_relu_maxpool_available(x, bn, relu, pool)   # fp32 surface: as it was


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case", ["grad", "switch"])
def test_half_fallbacks_run_torchs_ops_bit_for_bit(te, case, dtype, deterministic_convs):
    trunk = _trunk16(18, dtype, 2)
    x = _cl(torch.randn(2, 3, 64, 96, device=DEV).to(dtype))
    ref_trunk = copy.deepcopy(trunk)
    prev = te.set_trunk_fusion(case != "switch")
    try:
        with (torch.enable_grad() if case == "grad" else torch.no_grad()):      # grad: eval mode, parameters require grad
            before = te.launch_count()
            got = trunk(x)
            assert te.launch_count() == before, te.last_kernel()
            want = _trunk_reference(ref_trunk, x)
    finally:
        te.set_trunk_fusion(prev)
    assert got.dtype == dtype and torch.equal(_raw(got), _raw(want))


# ---- 6. trunk and model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("depth,img,launches", [(18, (2, 3, 64, 96), 17), (50, (1, 3, 64, 64), 1 + 3 * 16)])
def test_16_bit_trunks_take_the_fused_kernels(te, depth, img, launches, dtype):
    """The stem + 2 per BasicBlock x 8, or + 3 per Bottleneck x (3 + 4 + 6 + 3)."""
    trunk = _trunk16(depth, dtype, 0)
    x = _cl(torch.randn(img, device=DEV).to(dtype))
    with torch.no_grad():
        before = te.launch_count()
        got = trunk(x)
        assert te.launch_count() == before + launches
        assert te.last_kernel() == "bn_add_relu_half"
        prev = te.set_trunk_fusion(False)
        try:
            want = trunk(x)
            assert te.launch_count() == before + launches
        finally:
            te.set_trunk_fusion(prev)
    assert got.dtype == dtype and got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
    assert torch.isfinite(want).all() and torch.isfinite(got).all()
    # two 16-bit evaluations of the same trunk: a few ulps of the output's scale apart (information; the bar is the model's)
    scale = want.float().abs().max().item()
    print(f"resnet{depth} {dtype}: fused vs unfused max {(got.float() - want.float()).abs().max().item():.3e} at scale {scale:.3e} "
          f"(ulp {ulp_of(dtype):.1e})")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_mini_model_fused_error_is_not_above_unfused(te, dtype):
    from mvdetr_amd import geometry
    from mvdetr_amd.model import build_model

    def perturbed():
        m = build_model("mini", seed=0, bottleneck_dim=128).eval()
        with torch.no_grad():
            for layer in m.world_feat.encoder.layers:
                layer.self_attn.sampling_offsets.weight.normal_(0, 0.02, generator=torch.Generator().manual_seed(4))
                layer.self_attn.attention_weights.weight.normal_(0, 0.05, generator=torch.Generator().manual_seed(5))
        return m.to(DEV)

    model = perturbed().to_inference(dtype)
    ref = perturbed()                                                         # fp32, holding the same ROUNDED parameters
    ref.load_state_dict(model.state_dict())
    for name in ("pos_embedding", "coord_map"):
        if model.world_feat._buffers.get(name) is not None:
            ref.world_feat._buffers[name] = model.world_feat._buffers[name].float()
    assert all(p.dtype == torch.float32 for p in ref.parameters())
    imgs = torch.randn(1, 3, 3, *geometry.MINI.input_img_shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    imgs = imgs.to(dtype).float()                                             # (both models see the same, rounded frame)
    M = geometry.random_affine_mats(1, 3, geometry.MINI.input_img_shape, seed=2, translate=0.05, scale=(0.9, 1.1))
    flat = lambda o: [o[0][0], o[0][1], o[1][0], o[1][1], o[1][2]]          # noqa: E731
    with torch.no_grad():
        want = flat(ref(imgs, M))
        before = te.launch_count()
        fused = flat(model(imgs, M))
        assert te.launch_count() > before and te.last_kernel().endswith("_half")
        prev = te.set_trunk_fusion(False)
        try:
            before = te.launch_count()
            plain = flat(model(imgs, M))
            assert te.launch_count() == before
        finally:
            te.set_trunk_fusion(prev)
    for name, f, p, w in zip(("world_heatmap", "world_offset", "img_heatmap", "img_offset", "img_wh"), fused, plain, want):
        assert f.dtype == p.dtype == dtype and w.dtype == torch.float32 and f.shape == w.shape
        assert torch.isfinite(f).all() and torch.isfinite(p).all()
        rms_f, rms_p = _rms(f, w.double()), _rms(p, w.double())
        print(f"{name} ({dtype}): RMS vs the fp32 model: fused {rms_f:.4e}, unfused {rms_p:.4e} (ratio {rms_f / rms_p:.3f}); "
              f"output RMS {w.double().square().mean().sqrt().item():.3e}")
        assert rms_f <= 1.25 * rms_p, (name, rms_f, rms_p)
    det = model.detect(imgs, M, cls_thres=0.05)
    assert te.last_kernel().endswith("_half")
    assert det[0].dtype == torch.float32 and det[0].shape[-1] == 2 and torch.isfinite(det[0]).all()
