"""BatchNorm, residual and ReLU in the Winograd convolution's output store (mvdetr_amd/csrc/conv_winograd.hip, MODE 1-3).

The fused store applies bn_act_cl's expressions (csrc/bn_epilogue.h, one text for both kernels) to the value a lane is
about to store, so every comparison here is torch.equal against the two-launch form: the plain kernel, then bn_act in
place on its output.  Kernel level over every geometry edge, mode and the null gamma / beta; memory safety by NaN guards
around y and the residual; the refusals; then BasicBlock, Bottleneck and the ResNet-18 trunk with the switch on against
off, with the launch counts of both sides."""
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 1024                                      # floats of NaN on either side of y and of the residual

GEOMETRIES = [(3, 5, 7), (2, 4, 4), (1, 1, 1), (1, 2, 130), (64, 2, 2)]       # N, H, W
MODES = ["bn", "bn_add", "bn_bn_add"]


@pytest.fixture(scope="module")
def cw():
    from mvdetr_amd.ops import conv_winograd
    return conv_winograd


@pytest.fixture(scope="module")
def te():
    from mvdetr_amd.ops import trunk_epilogue
    return trunk_epilogue


def _bn(K, g, affine=True):
    bn = nn.BatchNorm2d(K, affine=affine)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(K, generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(K, generator=g) + 0.5)
        if affine:
            bn.weight.copy_(torch.randn(K, generator=g))                      # both signs
            bn.bias.copy_(torch.randn(K, generator=g) * 0.3)
    return bn.to(DEV).eval()


def _guarded(t):
    """A channel-last copy of t [N, K, H, W] inside a NaN-filled allocation: (the view, the whole buffer)."""
    N, K, H, W = t.shape
    buf = torch.full((t.numel() + 2 * PAD,), float("nan"), device=DEV)
    view = buf[PAD:PAD + t.numel()].view(N, H, W, K).permute(0, 3, 1, 2)
    view.copy_(t)
    assert view.is_contiguous(memory_format=torch.channels_last) and view.data_ptr() % 16 == 0
    return view, buf


def _case(N, C, K, H, W, d, mode, affine=True, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + N + 3 * C + 5 * K + 7 * H + 11 * W + 13 * d + len(mode))
    conv = nn.Conv2d(C, K, 3, 1, d, d, bias=False)
    with torch.no_grad():
        conv.weight.normal_(0, (2.0 / (C * 9)) ** 0.5, generator=g)
    x = torch.randn(N, C, H, W, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)     # mixed signs
    bn = _bn(K, g, affine)
    residual = residual_bn = res_buf = None
    if mode != "bn":
        residual, res_buf = _guarded(torch.randn(N, K, H, W, generator=g))
    if mode == "bn_bn_add":
        residual_bn = _bn(K, g)
    return conv.to(DEV).eval(), x, bn, residual, residual_bn, res_buf


def _vectors(*bns):
    return [v.detach().clone() for bn in bns if bn is not None
            for v in (bn.running_mean, bn.running_var, bn.weight, bn.bias) if v is not None]


def _fused_raw(cw, te, x, conv, bn, residual, residual_bn, relu):
    """The C entry on a y inside a NaN-filled buffer: (y as an NCHW-shaped view, the buffer, the return code)."""
    from mvdetr_amd import _lib
    N, C, H, W = x.shape
    K = conv.out_channels
    U = cw._transformed_weights(conv.weight)
    buf = torch.full((N * H * W * K + 2 * PAD,), float("nan"), device=DEV)
    y = buf[PAD:PAD + N * H * W * K]
    code = _lib.lib().mvdetr_conv3x3_winograd_bn_act_f32(
        x.data_ptr(), U.data_ptr(), y.data_ptr(), N, H, W, C, K, conv.dilation[0], *te._bn_args(bn),
        0 if residual is None else residual.data_ptr(), *te._bn_args(residual_bn), int(relu), _lib.current_stream_ptr(x.device))
    return y.view(N, H, W, K).permute(0, 3, 1, 2), buf, code


def _two_launch(cw, te, x, conv, bn, residual, residual_bn, relu):
    return te.bn_act(cw.winograd_conv3x3(x, conv, force=True), bn, residual, residual_bn, relu=relu, inplace=True)


def _check(cw, te, N, C, K, H, W, d, mode, relu, affine=True):
    conv, x, bn, residual, residual_bn, res_buf = _case(N, C, K, H, W, d, mode, affine)
    x_keep = x.clone(memory_format=torch.preserve_format)
    res_keep = None if res_buf is None else res_buf.clone()
    vec_keep = _vectors(bn, residual_bn)
    with torch.no_grad():
        want = _two_launch(cw, te, x, conv, bn, residual, residual_bn, relu)
        before, passes = cw.launch_count(), te.launch_count()
        got = cw.winograd_conv3x3_bn_act(x, conv, bn, residual, residual_bn, relu=relu, force=True)
        assert cw.launch_count() == before + 1 and te.launch_count() == passes
        assert cw.last_kernel() == "conv3x3_winograd_f32" and cw.last_epilogue() == mode + ("_relu" if relu else "")
        padded, buf, code = _fused_raw(cw, te, x, conv, bn, residual, residual_bn, relu)
    assert code == 0
    assert got.shape == want.shape == (N, K, H, W) and got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got, want) and torch.equal(padded, want)
    assert not torch.isnan(want).any()
    if relu:
        assert (want == 0).any() and (want > 0).any() and not (want < 0).any()     # ReLU cut something
    else:
        assert (want < 0).any() and (want > 0).any()
    # nothing outside y is stored, every element of y is; the inputs are bit-unchanged
    assert torch.isnan(buf[:PAD]).all() and torch.isnan(buf[-PAD:]).all() and not torch.isnan(buf[PAD:-PAD]).any()
    assert torch.equal(x, x_keep)
    if res_buf is not None:
        assert torch.equal(res_buf[PAD:-PAD], res_keep[PAD:-PAD])
        assert torch.isnan(res_buf[:PAD]).all() and torch.isnan(res_buf[-PAD:]).all()
    assert all(torch.equal(a, b) for a, b in zip(_vectors(bn, residual_bn), vec_keep))


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", [1, 2, 4])
@pytest.mark.parametrize("N,H,W", GEOMETRIES)
def test_fused_store_is_the_two_launch_form(cw, te, N, H, W, d, mode, relu):
    """C 24 -> K 128: three chunks, two channel blocks."""
    _check(cw, te, N, 24, 128, H, W, d, mode, relu)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d", [1, 2, 4])
@pytest.mark.parametrize("N,H,W", GEOMETRIES)
def test_fused_store_one_chunk_one_channel_block(cw, te, N, H, W, d, mode):
    """C 8 -> K 64: one chunk, one channel block; ReLU on and off alternate over the grid."""
    _check(cw, te, N, 8, 64, H, W, d, mode, relu=(N + d + len(mode)) % 2 == 0)


@pytest.mark.parametrize("C,K", [(8, 128), (24, 64)])
@pytest.mark.parametrize("mode", MODES)
def test_fused_store_null_gamma_and_beta(cw, te, C, K, mode):
    """affine=False: the BatchNorm has no weight and no bias, the entry gets null pointers (gamma 1, beta 0)."""
    _check(cw, te, 3, C, K, 5, 7, 2, mode, relu=True, affine=False)


@pytest.mark.parametrize("mode", ["bn_add", "bn_bn_add"])
@pytest.mark.parametrize("relu", [True, False])
def test_nan_comes_out_where_the_two_launch_form_has_it(cw, te, mode, relu):
    conv, x, bn, residual, residual_bn, _ = _case(3, 24, 128, 5, 7, 2, mode)
    x[1, 5, 2, 3] = float("nan")
    residual[2, 70, 4, 6] = float("nan")
    with torch.no_grad():
        want = _two_launch(cw, te, x, conv, bn, residual, residual_bn, relu)
        got = cw.winograd_conv3x3_bn_act(x, conv, bn, residual, residual_bn, relu=relu, force=True)
    nan = torch.isnan(want)
    # x's NaN reaches every channel of the pixels whose window holds it (and of their 2x2 tiles), the residual's one element
    assert nan[2, 70, 4, 6] and nan[1, :, 2, 3].all() and nan[2].sum().item() == 1 and not nan[0].any()
    assert 128 * 9 <= nan[1].sum().item() < nan[1].numel()
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got.nan_to_num(nan=-7.0), want.nan_to_num(nan=-7.0))


def test_refusals(cw, te):
    from mvdetr_amd import _lib
    lib, st = _lib.lib(), _lib.current_stream_ptr(torch.device(DEV))
    N, H, W, C, K = 1, 4, 4, 64, 64
    x, U, vec = (torch.zeros(1 << 16, device=DEV) for _ in range(3))
    ybuf = torch.full((1 << 16,), float("nan"), device=DEV)
    var = torch.ones(K, device=DEV)
    size = N * H * W * K

    def call(y, res, res_mean=None, res_var=None, mean=vec, var_=var):
        ptr = lambda t: None if t is None else t.data_ptr()                   # noqa: E731
        return lib.mvdetr_conv3x3_winograd_bn_act_f32(x.data_ptr(), U.data_ptr(), ptr(y), N, H, W, C, K, 1, ptr(mean), ptr(var_),
                                                      None, None, 1e-5, ptr(res), ptr(res_mean), ptr(res_var), None, None,
                                                      1e-5, 1, st)
    before = cw.launch_count()
    y = ybuf[:size]
    # a residual whose bytes meet y's: the same tensor, the last 16 bytes of y, the first 16 bytes behind the residual's start
    assert call(y, y) == 1
    assert call(y, ybuf[size - 4:]) == 1
    assert call(ybuf[size - 4:], y) == 1
    # a residual BatchNorm without a residual, a BatchNorm without its statistics
    assert call(y, None, vec, var) == 1
    assert call(y, ybuf[size:], mean=None) == 1
    assert call(y, ybuf[size:], var_=None) == 1
    assert call(y, ybuf[size:], vec, None) == 1
    # the convolution's own refusals stand
    assert call(None, None) == 1
    assert call(ybuf[1:], None) == 801
    assert call(y, ybuf[size + 1:]) == 801                                    # a residual that is not 16-byte aligned
    assert cw.launch_count() == before
    torch.cuda.synchronize()
    assert torch.isnan(ybuf).all()
    # adjacent ranges are fine
    assert call(y, ybuf[size:]) == 0 and cw.launch_count() == before + 1 and cw.last_epilogue() == "bn_add_relu"
    # the plain entry reports no epilogue
    assert lib.mvdetr_conv3x3_winograd_f32(x.data_ptr(), U.data_ptr(), y.data_ptr(), N, H, W, C, K, 1, st) == 0
    assert cw.last_epilogue() == "none" and cw.last_kernel() == "conv3x3_winograd_f32"
    torch.cuda.synchronize()


def test_the_wrapper_raises_where_the_predicate_is_false(cw, te):
    conv, x, bn, residual, _, _ = _case(2, 24, 128, 4, 4, 1, "bn_add")
    with torch.no_grad():
        assert not cw.winograd_conv3x3_bn_act_available(x, conv, bn, residual)     # (24, 128) is in no family
        with pytest.raises(RuntimeError):
            cw.winograd_conv3x3_bn_act(x, conv, bn, residual)
        with pytest.raises(RuntimeError):                                      # forced, but the residual has the wrong shape
            cw.winograd_conv3x3_bn_act(x, conv, bn, residual[:1], force=True)
        with pytest.raises(RuntimeError):                                      # forced, a BatchNorm in training mode
            cw.winograd_conv3x3_bn_act(x, conv, nn.BatchNorm2d(128).to(DEV), force=True)
        with pytest.raises(RuntimeError):                                      # forced, 16-bit activations
            cw.winograd_conv3x3_bn_act(x.half(), conv, bn, force=True)


# ---- block and trunk level ----------------------------------------------------------------------------------------------------

class _Floor:
    """The pixel floor lowered for a model on small images, MIOpen's deterministic solvers off (the kernel's condition)."""
    def __init__(self, cw, pixels=0):
        self.cw, self.pixels = cw, pixels

    def __enter__(self):
        self.prev = self.cw.set_winograd_min_pixels(self.pixels)
        self.det = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = False

    def __exit__(self, *exc):
        torch.backends.cudnn.deterministic = self.det
        self.cw.set_winograd_min_pixels(self.prev)


def _randomise_bn(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    return module.to(DEV).eval()


def _off(cw, run):
    prev = cw.set_winograd_epilogue(False)
    try:
        return run()
    finally:
        cw.set_winograd_epilogue(prev)


class _TorchConvs:
    """MIOpen's default solvers are not reproducible from one call to the next (measured here: the block's 1x1 downsample
    convolution differs from itself by 3e-7 - 5e-7, the trunk's stem + layer1/2 by more), and cudnn.deterministic cannot be
    asked for: the Winograd kernel then stands back.  So that switch-on against switch-off can still be held to torch.equal,
    the convolutions that torch runs are taken out of the comparison: record() keeps what each of them was given and
    returned during one forward, replay() ASSERTS during another that each is given the same bits again and hands back the
    recorded result.  Whatever the fused store did differently would show as a different input further down or a different
    output."""
    def __init__(self, module):
        self.convs = [m for m in module.modules() if type(m) is nn.Conv2d]
        self.tape, self.at, self.hooks = [], 0, []

    def _recorded(self, m, args, out):
        self.tape.append((m, args[0].clone(memory_format=torch.preserve_format), out.clone(memory_format=torch.preserve_format)))

    def _replayed(self, m, args, out):
        want, x, y = self.tape[self.at]
        self.at += 1
        assert m is want and torch.equal(args[0], x), f"torch convolution {self.at - 1} of the forward got other input bits"
        return y.clone(memory_format=torch.preserve_format)

    def _run(self, hook, run):
        self.hooks = [m.register_forward_hook(hook) for m in self.convs]
        try:
            return run()
        finally:
            for h in self.hooks:
                h.remove()

    def record(self, run):
        self.tape, self.at = [], 0
        return self._run(self._recorded, run)

    def replay(self, run):
        self.at = 0
        out = self._run(self._replayed, run)
        assert self.at == len(self.tape)
        return out


def _input(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).relu_().to(DEV).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("downsample", [False, True])
def test_basic_block_switch_on_against_off(cw, te, downsample):
    """BasicBlock(256, 256): both convolutions are in the (256, 256) d 1 family.  torch runs nothing in the block without a
    downsample; with one, its 1x1 convolution (_TorchConvs: one call on the tape)."""
    from mvdetr_amd.model import BasicBlock
    assert 1 in cw.FAMILIES[(256, 256)]
    torch.manual_seed(3)
    ds = nn.Sequential(nn.Conv2d(256, 256, 1, bias=False), nn.BatchNorm2d(256)) if downsample else None
    block = _randomise_bn(BasicBlock(256, 256, downsample=ds), 3)
    keys = list(block.state_dict())
    x = _input((2, 256, 8, 12), 3)
    x_keep = x.clone(memory_format=torch.preserve_format)
    with torch.no_grad(), _Floor(cw):
        block(x)                                                              # (builds the transformed weights)
        convs = _TorchConvs(block)
        before, passes = cw.launch_count(), te.launch_count()
        on = convs.record(lambda: block(x))
        assert len(convs.tape) == int(downsample)
        assert cw.launch_count() == before + 2 and te.launch_count() == passes     # no pass of its own
        assert cw.last_kernel() == "conv3x3_winograd_f32"
        assert cw.last_epilogue() == ("bn_bn_add_relu" if downsample else "bn_add_relu")
        before, passes = cw.launch_count(), te.launch_count()
        off = _off(cw, lambda: convs.replay(lambda: block(x)))
        assert cw.launch_count() == before + 2 and te.launch_count() == passes + 2 and cw.last_epilogue() == "none"
        # trunk fusion off: the epilogues are torch's ops, the fused store is not taken
        prev = te.set_trunk_fusion(False)
        try:
            before, passes = cw.launch_count(), te.launch_count()
            plain = block(x)
            assert cw.launch_count() == before + 2 and te.launch_count() == passes and cw.last_epilogue() == "none"
        finally:
            te.set_trunk_fusion(prev)
    assert torch.equal(on, off) and on.abs().max().item() > 0 and (on == 0).any()
    assert torch.allclose(plain, on, rtol=1e-4, atol=1e-4)
    assert torch.equal(x, x_keep) and list(block.state_dict()) == keys


@pytest.mark.parametrize("inplanes,planes,d,shape", [(1024, 256, 2, (2, 1024, 8, 12)), (2048, 512, 4, (1, 2048, 6, 10))])
def test_bottleneck_switch_on_against_off(cw, te, inplanes, planes, d, shape):
    """Bottleneck.conv2 with bn2 + ReLU in its store, at the shapes of test_conv_winograd_gpu.py's Bottleneck test.  The 1x1
    convolutions are torch's on both sides (_TorchConvs)."""
    from mvdetr_amd.model import Bottleneck
    assert d in cw.FAMILIES[(planes, planes)]
    torch.manual_seed(planes)
    block = _randomise_bn(Bottleneck(inplanes, planes, dilation=d), planes)
    x = _input(shape, planes)
    with torch.no_grad(), _Floor(cw):
        block(x)
        convs = _TorchConvs(block)
        before, passes = cw.launch_count(), te.launch_count()
        on = convs.record(lambda: block(x))
        assert len(convs.tape) == 2                                           # conv1 and conv3
        assert cw.launch_count() == before + 1 and te.launch_count() == passes + 2     # bn1 and bn3 keep their passes
        assert cw.last_epilogue() == "bn_relu"
        before, passes = cw.launch_count(), te.launch_count()
        off = _off(cw, lambda: convs.replay(lambda: block(x)))
        assert cw.launch_count() == before + 1 and te.launch_count() == passes + 3 and cw.last_epilogue() == "none"
        # conv2 + bn2 + ReLU alone, on the same input: bit for bit
        mid = te.bn_act(block.conv1(x), block.bn1, relu=True, inplace=True)
        fused = cw.winograd_conv3x3_bn_act(mid, block.conv2, block.bn2, relu=True)
        two = te.bn_act(cw.winograd_conv3x3(mid, block.conv2), block.bn2, relu=True, inplace=True)
    assert torch.equal(fused, two) and (fused == 0).any() and (fused > 0).any()
    assert torch.equal(on, off)


@pytest.fixture(scope="module")
def trunk():
    from mvdetr_amd.model import resnet_trunk
    torch.manual_seed(0)
    return _randomise_bn(resnet_trunk(18), 0)


def test_trunk_switch_on_against_off(cw, te, trunk):
    """resnet_trunk(18) on 2 x 3 x 256 x 384.  With the family table as it stands the eight layer3/4 convolutions take the
    kernel: with the switch on their epilogues ride in the store and 9 passes remain (the stem's and layer1/2's eight),
    with it off 17.  torch's twelve convolutions are on the tape of _TorchConvs."""
    assert cw.FAMILIES == {(128, 256): (1,), (256, 256): (1, 2), (256, 512): (2,), (512, 512): (1, 4)}
    keys = list(trunk.state_dict())
    x = torch.randn(2, 3, 256, 384, generator=torch.Generator().manual_seed(5)).to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), _Floor(cw):
        trunk(x)
        convs = _TorchConvs(trunk)
        before, passes = cw.launch_count(), te.launch_count()
        on = convs.record(lambda: trunk(x))
        assert len(convs.tape) == 12                                          # the stem, 8 in layer1/2, 3 downsample convolutions
        assert cw.launch_count() == before + 8 and te.launch_count() == passes + 9
        assert cw.last_kernel() == "conv3x3_winograd_f32" and cw.last_epilogue() == "bn_add_relu"
        before, passes = cw.launch_count(), te.launch_count()
        off = _off(cw, lambda: convs.replay(lambda: trunk(x)))
        assert cw.launch_count() == before + 8 and te.launch_count() == passes + 17
        prev = te.set_trunk_fusion(False)
        try:
            before, passes = cw.launch_count(), te.launch_count()
            plain = trunk(x)
            assert cw.launch_count() == before + 8 and te.launch_count() == passes and cw.last_epilogue() == "none"
        finally:
            te.set_trunk_fusion(prev)
    assert on.shape == off.shape and on.abs().max().item() > 0
    assert torch.equal(on, off)
    assert torch.allclose(plain, on, rtol=1e-3, atol=1e-3)
    assert list(trunk.state_dict()) == keys
