"""The fp32 Winograd F(2x2,3x3) MFMA convolution on the GPU (mvdetr_amd/csrc/conv_winograd.hip).

Op level: every case against F.conv2d in fp64 on the same inputs (post-ReLU N(0,1) activations, kaiming weights, as in
the trunk).  The bar is measured, not chosen: r = (the kernel's deviation from fp64) / (the deviation from fp64 of
torch's own fp32 convolution with cudnn.deterministic = True), for max-abs and for rms, and the assertion is 1.5 x the
worst r measured over all cases on an MI355X: 19.76 (max-abs; C 256, K 192, 5 x 7, dilation 2) and 18.74
(rms; C 256, K 192, 5 x 7, dilation 4).  Every r is printed (run with -s).  The ratios are this large, against about 3 at
the trunk's own sizes, because of the denominator: on images this small torch's deterministic fp32 convolution is within
half an ulp of the correctly rounded result (1.2e-7 on outputs of magnitude 4), while F(2x2,3x3) in float32 carries
about 5 ulp whatever the size (1.2e-6 to 2.5e-6 here).  That this is the arithmetic and not a wrong constant or edge tile is
what test_kernel_is_the_float32_algorithm checks: the kernel against a float32 emulation of the algorithm on the CPU
(conv_winograd_oracle.emulate_f32), at dilations 1, 2 and 4, odd and even extents, one chunk and odd chunk counts, post-ReLU
and mixed-sign activations, within 4 ulp of the largest output.  Measured on an MI355X over its eight cases: worst deviation
0.00 ulp, smallest share of identical elements 1.0000 -- the kernel reproduces the emulation bit for bit.
test_conv_winograd_exact_gpu.py holds it to fp64 with no tolerance on integer data over every geometry edge.

The weight transform on the device (test_weight_transform_on_the_device) against numpy's G g G^T: exact on integer weights;
on kaiming weights within one float32 rounding, identical in 1.000000 of the elements (bar: 0.999) at all three (C, K).

Model level: the trunk and the mini model with the Winograd convolutions on against off (their own switch), with the bar
2 x the deviation of the model from itself under two MIOpen solver choices (cudnn.deterministic True / False), measured in
the same test (each side: the largest of three repetitions, MIOpen's default solvers not being reproducible call to call);
where that is 0, 3 x the model's fp32-vs-fp64 deviation instead.  Measured on an MI355X, single repetitions: trunk max
4.6e-5 - 5.0e-5 / rms 4.8e-6 against bars of 5.8e-5 - 6.7e-5 / 7.2e-6; mini model's image heads 3.5e-6 - 4.3e-6 against
5.6e-6 - 6.9e-6."""
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import conv_winograd_oracle as oracle
from conv_winograd_oracle import emulate_f32
from test_conv_winograd import _numpy_weights

pytestmark = pytest.mark.gpu

DEV = "cuda"
R_WORST_MAX, R_WORST_RMS = 19.76, 18.74          # measured (see the docstring); the bars are 1.5 x these
PAD = 1024                                      # floats of NaN on either side of y


@pytest.fixture(scope="module")
def cw():
    from mvdetr_amd.ops import conv_winograd
    return conv_winograd


def _case(C, K, H, W, d, seed=0, relu=True):
    g = torch.Generator().manual_seed(1000 * seed + C + 3 * K + 7 * H + 11 * W + 13 * d)
    conv = nn.Conv2d(C, K, 3, 1, d, d, bias=False)
    with torch.no_grad():
        conv.weight.normal_(0, (2.0 / (K * 9)) ** 0.5, generator=g)            # kaiming_normal_(fan_out, relu)
    x = torch.randn(2, C, H, W, generator=g)
    if relu:
        x.relu_()
    return conv.to(DEV).eval(), x.to(DEV).contiguous(memory_format=torch.channels_last)


def _raw_call(cw, x, conv):
    """The C entry on a y that sits inside a larger NaN-filled buffer: (y as NCHW-shaped view, the whole buffer)."""
    from mvdetr_amd import _lib
    N, C, H, W = x.shape
    K, d = conv.out_channels, conv.dilation[0]
    U = cw._transformed_weights(conv.weight)
    buf = torch.full((N * H * W * K + 2 * PAD,), float("nan"), device=x.device)
    y = buf[PAD:PAD + N * H * W * K]
    code = _lib.lib().mvdetr_conv3x3_winograd_f32(x.data_ptr(), U.data_ptr(), y.data_ptr(), N, H, W, C, K, d,
                                                  _lib.current_stream_ptr(x.device))
    assert code == 0
    return y.view(N, H, W, K).permute(0, 3, 1, 2), buf


def _dev(a, want):
    e = (a.double() - want).abs()
    return e.max().item(), e.square().mean().sqrt().item()


@pytest.mark.parametrize("d", [1, 2, 4])
@pytest.mark.parametrize("H,W", [(10, 16), (9, 13), (5, 7), (18, 17)])
@pytest.mark.parametrize("C,K", [(64, 64), (128, 64), (64, 128), (256, 192)])
def test_against_fp64_with_the_measured_bar(cw, C, K, H, W, d):
    conv, x = _case(C, K, H, W, d)
    x_keep, w_keep = x.clone(memory_format=torch.preserve_format), conv.weight.detach().clone()
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        with torch.no_grad():
            want = F.conv2d(x.double(), conv.weight.double(), None, 1, d, d)
            torch_max, torch_rms = _dev(conv(x), want)
            cw._transformed_weights(conv.weight)                              # (the weight transform is a launch of its own)
            before = cw.launch_count()
            got = cw.winograd_conv3x3(x, conv, force=True)
            assert cw.launch_count() == before + 1 and cw.last_kernel() == "conv3x3_winograd_f32"
            again = cw.winograd_conv3x3(x, conv, force=True)
            padded, buf = _raw_call(cw, x, conv)
    finally:
        torch.backends.cudnn.deterministic = prev
    assert got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got, again) and torch.equal(got, padded)               # bit-identical call to call
    assert torch.equal(x, x_keep) and torch.equal(conv.weight, w_keep)        # inputs are never written
    assert torch.isnan(buf[:PAD]).all() and torch.isnan(buf[-PAD:]).all()     # nothing outside y is stored
    assert not torch.isnan(buf[PAD:-PAD]).any()                               # and every element of y is
    got_max, got_rms = _dev(got, want)
    r_max, r_rms = got_max / torch_max, got_rms / torch_rms
    print(f"C {C} K {K} {H}x{W} d {d}: winograd max {got_max:.3e} rms {got_rms:.3e} | torch max {torch_max:.3e} rms {torch_rms:.3e} "
          f"| r max {r_max:.2f} rms {r_rms:.2f}")
    assert torch_max > 0 and want.abs().max().item() > 1
    assert r_max <= 1.5 * R_WORST_MAX and r_rms <= 1.5 * R_WORST_RMS


@pytest.mark.parametrize("C,K,H,W,d,relu", [
    (64, 64, 10, 16, 1, True), (256, 192, 10, 16, 1, True),
    (24, 64, 9, 13, 1, True), (64, 64, 9, 13, 2, True), (64, 128, 5, 7, 4, True), (256, 192, 18, 17, 2, True), (8, 64, 3, 2, 4, True),
    (64, 64, 9, 13, 2, False),                                                # activations of both signs
])
def test_kernel_is_the_float32_algorithm(cw, C, K, H, W, d, relu):
    """The MFMA sums are k-ordered fmaf chains and every other step is a float add, so the kernel should reproduce a float32
    emulation of F(2x2,3x3) in the same order of operations (conv_winograd_oracle.emulate_f32: any dilation, odd extents).
    Bar: 4 ulp of the largest output -- the emulated fmaf rounds twice (fp64, then float), which can move the last bit of a
    partial sum, and an output is a signed sum of nine of them."""
    import numpy as np
    conv, x = _case(C, K, H, W, d, relu=relu)
    with torch.no_grad():
        got = cw.winograd_conv3x3(x, conv, force=True).cpu().numpy()
    emu = emulate_f32(x.cpu().numpy(), conv.weight.detach().cpu().numpy(), d)
    diff = np.abs(got.astype(np.float64) - emu).max()
    ulp = np.spacing(np.float32(np.abs(emu).max()))
    print(f"C {C} K {K} {H}x{W} d {d} relu {relu}: kernel vs float32 emulation max {diff:.3e} = {diff / ulp:.2f} ulp of the largest "
          f"output, identical elements {(got == emu).mean():.4f}")
    assert got.shape == emu.shape and np.abs(emu).max() > 0
    assert diff <= 4 * ulp


def test_refusals_of_the_c_entry(cw):
    from mvdetr_amd import _lib
    lib, st = _lib.lib(), _lib.current_stream_ptr(torch.device(DEV))
    x, U, y = (torch.zeros(1 << 16, device=DEV) for _ in range(3))
    ok = (x.data_ptr(), U.data_ptr(), y.data_ptr(), 1, 4, 4, 64, 64, 1, st)
    before = cw.launch_count()
    for i, bad in ((6, 60), (7, 96), (8, 3), (8, 0), (0, x.data_ptr() + 4), (1, U.data_ptr() + 8), (2, y.data_ptr() + 4)):
        args = list(ok)
        args[i] = bad
        assert lib.mvdetr_conv3x3_winograd_f32(*args) == 801, (i, bad)
    assert lib.mvdetr_conv3x3_winograd_f32(*ok[:2], ok[0], *ok[3:]) == 1                      # y is x
    assert lib.mvdetr_winograd_weights_f32(x.data_ptr(), 60, 64, U.data_ptr(), st) == 801
    assert lib.mvdetr_winograd_weights_f32(x.data_ptr(), 64, 32, U.data_ptr(), st) == 801
    # edges that launch nothing: an empty batch is done, a negative one and null pointers are invalid
    y.fill_(float("nan"))
    args = list(ok)
    args[3] = 0
    assert lib.mvdetr_conv3x3_winograd_f32(*args) == 0
    args[3] = -1
    assert lib.mvdetr_conv3x3_winograd_f32(*args) == 1
    for i in range(3):
        args = list(ok)
        args[i] = None
        assert lib.mvdetr_conv3x3_winograd_f32(*args) == 1, i
    assert lib.mvdetr_winograd_weights_f32(None, 64, 64, U.data_ptr(), st) == 1
    assert lib.mvdetr_winograd_weights_f32(x.data_ptr(), 64, 64, None, st) == 1
    # the 32-bit span guard, (256 + 2 H W) * max(C, K) < 2^30, just above the limit: the shape is checked here before the
    # call, since these buffers are far too small for a launch (test_conv_winograd.py asks the predicate about both sides)
    for C, K, H, W in ((64, 64, 2896, 2897), (128, 64, 2048, 2048), (64, 128, 2048, 2048)):
        assert (256 + 2 * H * (W - 1)) * max(C, K) < 1 << 30 <= (256 + 2 * H * W) * max(C, K)
        args = list(ok)
        args[4:8] = H, W, C, K
        assert lib.mvdetr_conv3x3_winograd_f32(*args) == 801, (C, K, H, W)
    assert cw.launch_count() == before
    torch.cuda.synchronize()
    assert torch.isnan(y).all()                                               # and nothing was written by any of them


@pytest.mark.parametrize("C,K", [(8, 64), (24, 128), (256, 192)])
def test_weight_transform_on_the_device(cw, C, K):
    """winograd_weights_f32 against numpy's G g G^T.  Integer multiples of 4: exact.  Kaiming weights: both sides are an fp64
    evaluation rounded once, so they differ by at most one float32 rounding, and only where the differently ordered fp64 sums
    fall on different sides of a rounding boundary -- the bar is one spacing of |U| (+ 2^-50 max|w| for the fp64 sums
    themselves, which matters where U is 0 or tiny), and at least 99.9 % of the elements are identical."""
    import numpy as np
    from mvdetr_amd import _lib
    lib, st = _lib.lib(), _lib.current_stream_ptr(torch.device(DEV))
    g = torch.Generator().manual_seed(C + 3 * K)
    cases = (("integer", (4 * torch.randint(-2, 3, (K, C, 3, 3), generator=g)).float()),
             ("kaiming", torch.randn(K, C, 3, 3, generator=g) * (2.0 / (K * 9)) ** 0.5))
    for name, w in cases:
        wd = w.to(DEV)
        buf = torch.full((16 * C * K + 2 * PAD,), float("nan"), device=DEV)
        before = cw.launch_count()
        assert lib.mvdetr_winograd_weights_f32(wd.data_ptr(), C, K, buf[PAD:-PAD].data_ptr(), st) == 0
        assert cw.launch_count() == before + 1 and cw.last_kernel() == "winograd_weights_f32"
        host = buf.cpu()
        assert torch.isnan(host[:PAD]).all() and torch.isnan(host[-PAD:]).all() and not torch.isnan(host[PAD:-PAD]).any()
        assert torch.equal(wd.cpu(), w)
        got, ref = host[PAD:-PAD].view(16, C, K).numpy(), _numpy_weights(w)
        share = (got == ref).mean()
        print(f"C {C} K {K} {name}: U identical to numpy's in {share:.6f} of the elements")
        if name == "integer":
            assert np.array_equal(got, ref) and np.array_equal(ref, np.round(ref)) and np.abs(ref).max() >= 8
        else:
            diff = np.abs(got.astype(np.float64) - ref.astype(np.float64))
            assert (diff <= np.spacing(np.abs(ref)).astype(np.float64) + 2.0 ** -50 * w.abs().max().item()).all(), diff.max()
            assert share >= 0.999


def test_channels_last_weight_tensor(cw):
    """A non-dense (channels-last) weight goes through the real transform: the same U and the same output, bit for bit, as its
    dense twin."""
    conv, x = _case(64, 64, 9, 13, 2)
    twin = copy.deepcopy(conv).to(memory_format=torch.channels_last)
    assert conv.weight.is_contiguous() and not twin.weight.is_contiguous()
    assert twin.weight.is_contiguous(memory_format=torch.channels_last) and torch.equal(twin.weight, conv.weight)
    with torch.no_grad():
        before = cw.launch_count()
        U, Ut = cw._transformed_weights(conv.weight), cw._transformed_weights(twin.weight)
        assert cw.launch_count() == before + 2 and U is not Ut and torch.equal(U, Ut)
        y, yt = cw.winograd_conv3x3(x, conv, force=True), cw.winograd_conv3x3(x, twin, force=True)
    assert torch.equal(y, yt) and y.abs().max().item() > 1


def test_cache_with_the_real_kernel(cw):
    """The cache of transformed weights behind winograd_conv3x3(), on integer cases (so every comparison is exact): after each
    way of changing the weights the output is the convolution with the NEW weights, at the price of one transform."""
    N, C, K, H, W, d = 2, 24, 64, 5, 9, 2
    x, w0 = oracle.integer_case(N, C, K, H, W, d, seed=0)
    w1, w2 = (oracle.integer_case(N, C, K, H, W, d, seed=s)[1] for s in (1, 2))
    assert not torch.equal(w0, w1) and not torch.equal(w1, w2)
    conv = nn.Conv2d(C, K, 3, 1, d, d, bias=False)
    with torch.no_grad():
        conv.weight.copy_(w0)
    conv = conv.to(DEV).eval()
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)

    def run(w, launches):
        before = cw.launch_count()
        with torch.no_grad():
            got = cw.winograd_conv3x3(xd, conv, force=True).cpu()
        want = oracle.direct_fp64(x, w, d)
        oracle.check_sanity(want, C)
        assert torch.equal(got.double(), want), oracle.first_mismatch(got, want, d)
        assert cw.launch_count() == before + launches

    run(w0, 2)                                                                 # the transform and the convolution
    run(w0, 1)                                                                 # an unchanged weight: no transform
    with torch.no_grad():
        conv.weight.copy_(w1.to(DEV))
    run(w1, 2)
    run(w1, 1)
    conv.load_state_dict({"weight": w2})
    run(w2, 2)
    run(w2, 1)
    conv.double().float()                                                      # new storage behind the same Parameter
    run(w2, 2)
    run(w2, 1)


@pytest.mark.parametrize("inplanes,planes,d,shape", [(1024, 256, 2, (2, 1024, 8, 12)), (2048, 512, 4, (1, 2048, 6, 10))])
def test_bottleneck_with_winograd_against_torchs_convolution(cw, inplanes, planes, d, shape):
    """Bottleneck.conv2 goes through model._conv3x3 at the shapes the family table holds for it ((256, 256) d 2, (512, 512) d 4):
    on against off within the bar of the trunk test, one Winograd launch per forward when on, none when off or under
    cudnn.deterministic."""
    from mvdetr_amd.model import Bottleneck
    assert d in cw.FAMILIES[(planes, planes)]
    torch.manual_seed(planes)
    block = Bottleneck(inplanes, planes, dilation=d)
    g = torch.Generator().manual_seed(planes)
    with torch.no_grad():
        for m in block.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    block = block.to(DEV).eval()
    keys = list(block.state_dict())
    x = torch.randn(*shape, generator=g).relu_().to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), _Floor(cw):
        block(x)                                                              # (builds the transformed weights)
        before = cw.launch_count()
        on = [block(x) for _ in range(REPS)]
        assert cw.launch_count() == before + REPS and cw.last_kernel() == "conv3x3_winograd_f32"
        prev = cw.set_trunk_winograd(False)
        try:
            before = cw.launch_count()
            off, det = _solver_runs(lambda: block(x))
            assert cw.launch_count() == before
        finally:
            cw.set_trunk_winograd(prev)
        torch.backends.cudnn.deterministic = True                             # (_Floor restores it)
        before = cw.launch_count()
        block(x)
        assert cw.launch_count() == before                                    # the switch is on, the caller asked for determinism
        torch.backends.cudnn.deterministic = False
        _assert_within(f"Bottleneck({inplanes}, {planes}, dilation={d})", on, off, det,
                       lambda: copy.deepcopy(block).double()(x.double()))
    assert list(block.state_dict()) == keys


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


class _Floor:
    """The pixel floor lowered for a model on small images, MIOpen's default solvers."""
    def __init__(self, cw, pixels=0):
        self.cw, self.pixels = cw, pixels

    def __enter__(self):
        self.prev = self.cw.set_winograd_min_pixels(self.pixels)
        self.det = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = False

    def __exit__(self, *exc):
        torch.backends.cudnn.deterministic = self.det
        self.cw.set_winograd_min_pixels(self.prev)


REPS = 3


def _solver_runs(run):
    """run() REPS times with torch's convolutions under MIOpen's default solvers, and once under the deterministic ones."""
    default = [run() for _ in range(REPS)]
    torch.backends.cudnn.deterministic = True
    try:
        return default, run()
    finally:
        torch.backends.cudnn.deterministic = False


def _worst(pairs):
    devs = [_dev(a, b.double()) for a, b in pairs]
    return max(d[0] for d in devs), max(d[1] for d in devs)


def _assert_within(name, on, off, det, fp64):
    """on[i] against off[i] within 2 x (off[i] against det).  MIOpen's default solvers are not reproducible from one call to
    the next, which moves both sides of the comparison, so each side is the largest of REPS repetitions."""
    d_max, d_rms = _worst(zip(on, off))
    b_max, b_rms = _worst((o, det) for o in off)
    how = "2 x solver-vs-solver"
    if b_max == 0:
        b_max, b_rms = _dev(off[0], fp64())
        b_max, b_rms, how = 1.5 * b_max, 1.5 * b_rms, "3 x fp32-vs-fp64"
    print(f"{name}: winograd on vs off max {d_max:.3e} rms {d_rms:.3e} | bar ({how}) max {2 * b_max:.3e} rms {2 * b_rms:.3e}")
    assert on[0].shape == off[0].shape and off[0].abs().max().item() > 0
    assert d_max <= 2 * b_max and d_rms <= 2 * b_rms, name


def test_trunk_with_winograd_against_torchs_convolutions(cw):
    assert cw.FAMILIES, "no convolution family is switched on"
    trunk = _small_trunk()
    keys = list(trunk.state_dict())
    x = torch.randn(2, 3, 256, 384, generator=torch.Generator().manual_seed(5)).to(DEV).contiguous(memory_format=torch.channels_last)     # 2 x 32 x 48 = 3,072 pixels
    n_convs = sum(1 for m in trunk.modules() if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3)
                  and m.dilation[0] in cw.FAMILIES.get((m.in_channels, m.out_channels), ()))
    assert n_convs > 0
    with torch.no_grad(), _Floor(cw):
        trunk(x)                                                              # (builds the transformed weights)
        before = cw.launch_count()
        on = [trunk(x) for _ in range(REPS)]
        assert cw.launch_count() == before + REPS * n_convs and cw.last_kernel() == "conv3x3_winograd_f32"
        prev = cw.set_trunk_winograd(False)
        try:
            before = cw.launch_count()
            off, det = _solver_runs(lambda: trunk(x))
            assert cw.launch_count() == before
        finally:
            cw.set_trunk_winograd(prev)
        _assert_within("trunk", on, off, det, lambda: copy.deepcopy(trunk).double()(x.double()))
    assert list(trunk.state_dict()) == keys
    # at the default floor this input keeps torch's convolutions
    with torch.no_grad():
        before = cw.launch_count()
        trunk(x)
        assert cw.launch_count() == before


def test_mini_model_with_winograd_against_torchs_convolutions(cw):
    from mvdetr_amd import geometry
    from mvdetr_amd.model import build_model
    model = build_model("mini", seed=0).eval()
    with torch.no_grad():
        for layer in model.world_feat.encoder.layers:
            layer.self_attn.sampling_offsets.weight.normal_(0, 0.02)
            layer.self_attn.attention_weights.weight.normal_(0, 0.05)
    model = model.to(DEV)
    keys = list(model.state_dict())
    imgs = torch.randn(1, 3, 3, *geometry.MINI.input_img_shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    M = geometry.random_affine_mats(1, 3, geometry.MINI.input_img_shape, seed=2, translate=0.05, scale=(0.9, 1.1))
    flat = lambda o: [o[0][0], o[0][1], o[1][0], o[1][1], o[1][2]]          # noqa: E731
    with torch.no_grad(), _Floor(cw):
        before = cw.launch_count()
        on = [flat(model(imgs, M)) for _ in range(REPS)]
        assert cw.launch_count() > before
        prev = cw.set_trunk_winograd(False)
        try:
            before = cw.launch_count()
            off, det = _solver_runs(lambda: flat(model(imgs, M)))
            assert cw.launch_count() == before
        finally:
            cw.set_trunk_winograd(prev)
        fp64 = []

        def double_outputs(i):
            if not fp64:
                fp64.extend(flat(copy.deepcopy(model).double()(imgs.double(), M.double())))
            return fp64[i]
        for i, name in enumerate(("world_heatmap", "world_offset", "img_heatmap", "img_offset", "img_wh")):
            _assert_within(name, [o[i] for o in on], [o[i] for o in off], det[i], lambda i=i: double_outputs(i))
    assert list(model.state_dict()) == keys


def test_the_environment_switch_keeps_torchs_convolutions(cw):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import torch\n"
        "from torch import nn\n"
        "from mvdetr_amd.ops import conv_winograd as cw\n"
        "from mvdetr_amd.model import BasicBlock\n"
        "cw.set_winograd_min_pixels(0)\n"
        "cw.FAMILIES[(64, 64)] = (1,)\n"
        "b = BasicBlock(64, 64).cuda().eval()\n"
        "x = torch.randn(1, 64, 8, 8, device='cuda').contiguous(memory_format=torch.channels_last)\n"
        "with torch.no_grad():\n"
        "    b(x)\n"
        "torch.cuda.synchronize()\n"
        "print('LAUNCHES', cw.launch_count(), cw.trunk_winograd_enabled())\n"
    ) % root
    for value, want in (("0", "LAUNCHES 0 False"), ("1", "LAUNCHES 4 True")):    # two weight transforms + two convolutions
        env = dict(os.environ, MVDETR_TRUNK_WINOGRAD=value)
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
        assert want in out.stdout, out.stdout + out.stderr
