"""The trunk's fused inference epilogues on the GPU (mvdetr_amd/csrc/trunk_epilogue.hip).

Bars are measured, not chosen: the op-level bar is twice the deviation from fp64 of torch's own unfused fp32 chain
(F.batch_norm eval -> + -> relu) on the same input; the model-level bar is twice the deviation between the unfused
channel-last model and the unfused NCHW model on the same frame (two orderings of the same fp32 arithmetic that
tests/test_frame_gpu.py already treats as one result).  Every measured pair is printed (run with -s to see them).

NaN results are compared as "NaN in the same places and torch.equal everywhere else": torch.equal itself is False for
any tensor holding a NaN, also against itself."""
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def te():
    from mvdetr_amd.ops import trunk_epilogue
    assert trunk_epilogue.trunk_fusion_enabled()
    return trunk_epilogue


@pytest.fixture
def deterministic_convs():
    """MIOpen's default 3x3 fp32 convolutions are not bit-reproducible from one call to the next on this GPU (the same
    module on the same input twice: 1.5e-5 apart after the trunk), so "torch's result bit for bit" is only defined with
    its deterministic solvers; the epilogues under test are deterministic either way."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _bn(C, seed, affine=True, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(C, affine=affine)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.5)
        bn.running_var.copy_(torch.rand(C, generator=g) * 2 + 0.25)
        if affine:
            bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
    return bn.to(DEV, dtype).eval().requires_grad_(False)      # (frozen: the tests below call the ops with autograd on)


def _bn64(bn, x):
    """The BatchNorm formula in fp64 from the module's fp32 vectors."""
    v = [t.double().view(1, -1, 1, 1) for t in (bn.running_mean, bn.running_var)]
    y = (x.double() - v[0]) / torch.sqrt(v[1] + bn.eps)
    if bn.weight is not None:
        y = y * bn.weight.double().view(1, -1, 1, 1) + bn.bias.double().view(1, -1, 1, 1)
    return y


def _torch_bn(bn, x):
    return F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)


def _same(got, want):
    nan = want.isnan()
    return got.shape == want.shape and torch.equal(got.isnan(), nan) and torch.equal(got.masked_fill(nan, 0), want.masked_fill(nan, 0))


# the trunk's activation shapes at 2 views (the passes are per element) and two whose row count is not a multiple of the
# block's tile (C = 64: 16 rows per block and step; C = 2048: two 256-group chunks per row); 96 takes the untiled kernel
SHAPES = [(2, 64, 180, 320), (2, 128, 90, 160), (2, 256, 90, 160), (2, 512, 90, 160), (2, 2048, 23, 41), (2, 64, 45, 79),
          (1, 96, 37, 53)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", ["none", "identity", "downsample_bn"])
def test_bn_act_within_twice_torchs_own_deviation_from_fp64(te, shape, mode):
    torch.manual_seed(shape[1] + shape[2])
    x = _cl(torch.randn(shape, device=DEV) * 2)
    r = None if mode == "none" else _cl(torch.randn(shape, device=DEV) * 2)
    r_keep = None if r is None else r.clone(memory_format=torch.preserve_format)
    for affine in (True, False):
        bn = _bn(shape[1], 1, affine)
        bn_r = _bn(shape[1], 2, affine) if mode == "downsample_bn" else None
        for relu in (True, False):
            want = _bn64(bn, x)
            chain = _torch_bn(bn, x)
            if r is not None:
                want = want + (_bn64(bn_r, r) if bn_r is not None else r.double())
                chain = chain + (_torch_bn(bn_r, r) if bn_r is not None else r)
            if relu:
                want, chain = torch.relu(want), torch.relu(chain)
            e_t = (chain.double() - want).abs()
            t_max, t_rms = e_t.max().item(), e_t.square().mean().sqrt().item()
            for inplace in (False, True):
                xin = x.clone(memory_format=torch.preserve_format) if inplace else x
                before = te.launch_count()
                got = te.bn_act(xin, bn, r, bn_r, relu=relu, inplace=inplace)
                assert te.launch_count() == before + 1
                assert te.last_kernel() == {"none": "bn", "identity": "bn_add", "downsample_bn": "bn_bn_add"}[mode] + ("_relu" if relu else "")
                assert (got.data_ptr() == xin.data_ptr()) == inplace and got.is_contiguous(memory_format=torch.channels_last)
                e = (got.double() - want).abs()
                f_max, f_rms = e.max().item(), e.square().mean().sqrt().item()
                print(f"bn_act {shape} {mode} affine={affine} relu={relu} inplace={inplace}: fused max {f_max:.3e} rms {f_rms:.3e} | "
                      f"torch chain max {t_max:.3e} rms {t_rms:.3e}")
                assert f_max <= 2 * t_max and f_rms <= 2 * t_rms
                if not inplace:
                    assert torch.equal(xin, x)
            if r is not None:
                assert torch.equal(r, r_keep)                      # (the residual is read only)


def test_bn_act_propagates_nan_and_inf_like_torch(te):
    bn = _bn(64, 3)
    x = _cl(torch.randn(1, 64, 5, 7, device=DEV))
    x[0, 3, 1, 2], x[0, 4, 0, 0], x[0, 5, 4, 6] = float("nan"), float("inf"), float("-inf")
    got = te.bn_act(x, bn, relu=True)
    want = torch.relu(_torch_bn(bn, x))
    assert got[0, 3, 1, 2].isnan() and got[0, 4, 0, 0] == float("inf") and got[0, 5, 4, 6] == 0
    assert torch.equal(got.isnan(), want.isnan()) and torch.equal(got.isinf(), want.isinf())
    # the residual modes: NaN / inf arriving through x and through the residual
    r = _cl(torch.randn(1, 64, 5, 7, device=DEV))
    r[0, 8, 2, 2], r[0, 9, 3, 3], r[0, 10, 0, 6] = float("nan"), float("inf"), float("-inf")
    for bn_r in (None, _bn(64, 6)):
        got = te.bn_act(x, bn, r, bn_r, relu=True)
        want = torch.relu(_torch_bn(bn, x) + (r if bn_r is None else _torch_bn(bn_r, r)))
        assert got[0, 3, 1, 2].isnan() and got[0, 8, 2, 2].isnan() and got[0, 9, 3, 3] == float("inf") and got[0, 10, 0, 6] == 0
        assert got[0, 4, 0, 0] == float("inf") and got[0, 5, 4, 6] == 0
        assert torch.equal(got.isnan(), want.isnan()) and torch.equal(got.isinf(), want.isinf())
        ok = want.isfinite()
        assert (got[ok] - want[ok]).abs().max().item() < 1e-4


@pytest.mark.parametrize("shape", [(2, 64, 360, 640), (2, 64, 45, 79), (1, 64, 7, 5), (3, 128, 1, 1), (1, 2048, 6, 9), (1, 64, 2, 640)],
                         ids=lambda s: "x".join(map(str, s)))
def test_bn_relu_maxpool_is_the_pool_of_bn_act_bit_for_bit(te, shape):
    torch.manual_seed(shape[2])
    bn = _bn(shape[1], 4)
    x = _cl(torch.randn(shape, device=DEV) * 2)
    N, C, H, W = shape
    x[0, 1, 0, 0], x[-1, 2, H - 1, W - 1], x[0, 3, H // 2, W // 2] = float("nan"), float("inf"), float("-inf")
    x[0, 5, H - 1, 0], x[0, 6, 0, W - 1], x[0, 7, H // 2, 0] = float("nan"), float("nan"), float("inf")
    before = te.launch_count()
    got = te.bn_relu_maxpool(x, bn)
    assert te.last_kernel() == "bn_relu_maxpool" and te.launch_count() == before + 1
    want = F.max_pool2d(te.bn_act(x, bn, relu=True), 3, 2, 1)
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert want.isnan().any() and want.isinf().any()
    assert _same(got, want)
    # and torch's own three modules agree to rounding (BatchNorm in another arithmetic order)
    ref = F.max_pool2d(torch.relu(_torch_bn(bn, x)), 3, 2, 1)
    ok = ref.isfinite()
    assert torch.equal(ok, got.isfinite()) and (got[ok] - ref[ok]).abs().max().item() < 1e-4


def _block_reference(b, x):
    identity = x if b.downsample is None else b.downsample(x)
    out = b.relu(b.bn1(b.conv1(x)))
    if hasattr(b, "conv3"):
        out = b.relu(b.bn2(b.conv2(out)))
        out = b.bn3(b.conv3(out))
    else:
        out = b.bn2(b.conv2(out))
    return b.relu(out + identity)


def _trunk_reference(trunk, x):
    for i, m in enumerate(trunk):
        if i < 4:
            x = m(x)
        else:
            for b in m:
                x = _block_reference(b, x)
    return x


def _small_trunk(seed=0):
    from mvdetr_amd.model import resnet_trunk
    torch.manual_seed(seed)
    trunk = resnet_trunk(18)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in trunk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    return trunk.to(DEV).eval()


def test_eval_trunk_takes_the_fused_kernels_and_agrees_with_torchs_ops(te, deterministic_convs):
    trunk = _small_trunk()
    x = _cl(torch.randn(2, 3, 64, 96, device=DEV))
    with torch.no_grad():
        before = te.launch_count()
        got = trunk(x)
        assert te.launch_count() == before + 17                   # the stem + 2 per BasicBlock x 8 blocks
        assert te.last_kernel() == "bn_add_relu"
        prev = te.set_trunk_fusion(False)
        try:
            want = trunk(x)
            assert te.launch_count() == before + 17
        finally:
            te.set_trunk_fusion(prev)
        assert torch.equal(want, _trunk_reference(trunk, x))
    assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
    # the two differ by one fp32 rounding or so per epilogue (6e-8 relative), carried through 17 convolutions of unit
    # gain: 1e-6 of the output's scale is expected; the measured bars are in the model-level tests below
    assert (got - want).abs().max().item() < 1e-4 * max(1.0, want.abs().max().item())


def test_resnet50_trunk_takes_the_fused_kernels(te):
    from mvdetr_amd.model import resnet_trunk
    torch.manual_seed(2)
    trunk = resnet_trunk(50).to(DEV).eval()
    x = _cl(torch.randn(1, 3, 64, 64, device=DEV))
    with torch.no_grad():
        before = te.launch_count()
        got = trunk(x)
        assert te.launch_count() == before + 1 + 3 * 16           # the stem + 3 per Bottleneck x (3 + 4 + 6 + 3)
        assert te.last_kernel() == "bn_add_relu"
        prev = te.set_trunk_fusion(False)
        try:
            want = trunk(x)
        finally:
            te.set_trunk_fusion(prev)
    assert (got - want).abs().max().item() < 1e-4 * max(1.0, want.abs().max().item())


def test_the_block_input_and_the_callers_tensor_are_never_written(te):
    trunk = _small_trunk(1)
    x = _cl(torch.randn(1, 3, 64, 64, device=DEV))
    with torch.no_grad():
        mid = trunk[3](trunk[2](trunk[1](trunk[0](x))))
        for layer in (trunk[4], trunk[5]):
            for b in layer:
                keep = mid.clone(memory_format=torch.preserve_format)
                before = te.launch_count()
                out = b(mid)
                assert te.launch_count() == before + 2 and out.data_ptr() != mid.data_ptr()
                assert torch.equal(mid, keep)
                mid = out


@pytest.mark.parametrize("case", ["train", "grad", "fp64", "nchw", "switch"])
def test_fallbacks_run_torchs_ops_bit_for_bit(te, case, deterministic_convs):
    trunk = _small_trunk(2)
    x = _cl(torch.randn(2, 3, 64, 96, device=DEV))
    ctx = torch.no_grad()
    if case == "train":
        trunk.train()
    elif case == "grad":
        ctx = torch.enable_grad()                                   # eval mode, parameters require grad
    elif case == "fp64":
        trunk, x = trunk.double(), x.double()
    elif case == "nchw":
        x = x.contiguous()
    ref_trunk = copy.deepcopy(trunk)
    prev = te.set_trunk_fusion(case != "switch")
    try:
        with ctx:
            before = te.launch_count()
            got = trunk(x)
            assert te.launch_count() == before, te.last_kernel()
            want = _trunk_reference(ref_trunk, x)
    finally:
        te.set_trunk_fusion(prev)
    assert torch.equal(got, want)
    if case == "grad":
        got.square().mean().backward()
        assert trunk[0].weight.grad is not None and trunk[0].weight.grad.abs().sum() > 0
    if case == "train":
        for (k, a), b in zip(trunk.state_dict().items(), ref_trunk.state_dict().values()):
            assert torch.equal(a, b), k


def test_fallback_predicates(te, deterministic_convs):
    bn = _bn(64, 5)
    x = _cl(torch.randn(1, 64, 8, 8, device=DEV))
    relu, pool = nn.ReLU(), nn.MaxPool2d(3, 2, 1)
    assert te.fused_bn_act_available(x, bn) and te.fused_bn_relu_maxpool_available(x, bn, relu, pool)
    for other in (nn.MaxPool2d(2, 2), nn.MaxPool2d(3, 2, 1, ceil_mode=True), nn.MaxPool2d(3, 2, 0), nn.MaxPool2d(3, 1, 1),
                  nn.MaxPool2d(3, 2, 1, dilation=2), nn.MaxPool2d(3, 2, 1, return_indices=True), nn.AvgPool2d(3, 2, 1)):
        assert not te.fused_bn_relu_maxpool_available(x, bn, relu, other)
    assert not te.fused_bn_relu_maxpool_available(x, bn, nn.LeakyReLU(), pool)
    assert not te.fused_bn_act_available(x.contiguous(), bn)                                 # NCHW
    assert not te.fused_bn_act_available(x[..., ::2], bn)                                    # a strided view
    assert not te.fused_bn_act_available(x.double(), bn) and not te.fused_bn_act_available(x.half(), bn)
    assert not te.fused_bn_act_available(x, copy.deepcopy(bn).train())
    assert not te.fused_bn_act_available(x, nn.BatchNorm2d(64, track_running_stats=False).to(DEV).eval())
    assert not te.fused_bn_act_available(x, bn, x)                                           # the residual is the output
    base = torch.randn(1, 8 * 8 + 8, 64, device=DEV)                                         # two dense NHWC tensors, overlapping storage
    a, b = base[:, :64].view(1, 8, 8, 64).permute(0, 3, 1, 2), base[:, 8:].view(1, 8, 8, 64).permute(0, 3, 1, 2)
    assert a.is_contiguous(memory_format=torch.channels_last) and not te.fused_bn_act_available(a, bn, b)
    assert not te.fused_bn_act_available(b, bn, a) and te.fused_bn_act_available(a, bn, x)
    assert not te.fused_bn_act_available(x, bn, _cl(torch.randn(1, 64, 8, 4, device=DEV)))
    with torch.enable_grad():
        assert te.fused_bn_act_available(x, bn)                                              # nothing requires grad
        assert not te.fused_bn_act_available(x, copy.deepcopy(bn).requires_grad_(True))      # gamma / beta require grad
        assert not te.fused_bn_act_available(x.clone(memory_format=torch.preserve_format).requires_grad_(True), bn)
    # a non-contiguous identity branch: the block's tail is torch's three ops
    from mvdetr_amd import model as mm
    out = _cl(torch.randn(1, 64, 8, 8, device=DEV))
    ident = _cl(torch.randn(1, 64, 8, 16, device=DEV))[..., ::2]
    assert not ident.is_contiguous() and not ident.is_contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        before = te.launch_count()
        got = mm._bn_add_relu(out.clone(memory_format=torch.preserve_format), bn, ident, None, nn.ReLU(inplace=True))
        assert te.launch_count() == before and torch.equal(got, torch.relu(bn(out) + ident))
    # a stem with another pool keeps torch's three passes
    from mvdetr_amd.model import ResNetTrunk
    stem = ResNetTrunk(nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True), nn.MaxPool2d(2, 2)).to(DEV).eval()
    img = _cl(torch.randn(1, 3, 32, 32, device=DEV))
    with torch.no_grad():
        before = te.launch_count()
        got = stem(img)
        assert te.launch_count() == before
        assert torch.equal(got, stem[3](stem[2](stem[1](stem[0](img)))))


def _devs(a, b):
    d = (a.double() - b.double()).abs()
    return d.max().item(), d.square().mean().sqrt().item()


def _frame_ab(te, model, other, imgs, M):
    """All five outputs: fused against unfused (same process, same model), with the bar 2 x the deviation between the
    unfused channel-last and the unfused NCHW model."""
    flat = lambda o: [o[0][0], o[0][1], o[1][0], o[1][1], o[1][2]]          # noqa: E731
    with torch.no_grad():
        before = te.launch_count()
        fused = flat(model(imgs, M))
        assert te.launch_count() > before
        prev = te.set_trunk_fusion(False)
        try:
            before = te.launch_count()
            plain = flat(model(imgs, M))
            nchw = flat(other(imgs, M))
            assert te.launch_count() == before
        finally:
            te.set_trunk_fusion(prev)
    for name, f, p, n in zip(("world_heatmap", "world_offset", "img_heatmap", "img_offset", "img_wh"), fused, plain, nchw):
        (f_max, f_rms), (b_max, b_rms) = _devs(f, p), _devs(p, n)
        print(f"{name}: fused vs unfused max {f_max:.3e} rms {f_rms:.3e} | unfused channel-last vs unfused NCHW max {b_max:.3e} rms {b_rms:.3e}")
        assert f.shape == p.shape and p.abs().max().item() > 0
        assert f_max <= 2 * b_max and f_rms <= 2 * b_rms, name


def test_mini_model_fused_against_unfused(te):
    from mvdetr_amd import geometry
    from mvdetr_amd.model import build_model
    model = build_model("mini", seed=0).eval()
    with torch.no_grad():
        for layer in model.world_feat.encoder.layers:
            layer.self_attn.sampling_offsets.weight.normal_(0, 0.02)
            layer.self_attn.attention_weights.weight.normal_(0, 0.05)
    model = model.to(DEV)
    other = build_model("mini", seed=0, channels_last=False).eval().to(DEV)
    other.load_state_dict(model.state_dict())
    imgs = torch.randn(1, 3, 3, *geometry.MINI.input_img_shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    M = geometry.random_affine_mats(1, 3, geometry.MINI.input_img_shape, seed=2, translate=0.05, scale=(0.9, 1.1))
    _frame_ab(te, model, other, imgs, M)


def test_full_size_wildtrack_frame_fused_against_unfused(te):
    """The benchmark's seeded model and input (bench.py: build_model('wildtrack', seed=0), perturb_sampling, the frame
    of generator seed 1000, identity augmentation)."""
    import bench
    from mvdetr_amd import geometry
    from mvdetr_amd.model import build_model
    geom = geometry.GEOMETRIES["wildtrack"]
    model = build_model("wildtrack", seed=0)
    bench.perturb_sampling(model, 1.0)
    model = model.to(DEV).eval()
    other = build_model("wildtrack", seed=0, channels_last=False).eval().to(DEV)
    other.load_state_dict(model.state_dict())
    imgs = torch.randn(1, geom.num_cam, 3, *geom.input_img_shape, generator=torch.Generator().manual_seed(1000)).to(DEV)
    M = torch.eye(3).repeat(1, geom.num_cam, 1, 1)
    _frame_ab(te, model, other, imgs, M)
