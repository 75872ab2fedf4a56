"""dc_fwd_mfma_half (csrc/deform_conv_half.hip) on the MI355X: ops.deform_conv2d, ops.DeformConv2d, the ``deform_conv``
aggregator and the converted model in float16 / bfloat16.

The kernel's bar, on EVERY element:  |out - ref| <= u |ref| + bars(...)["out"],  u = 2^-11 (fp16) / 2^-8 (bf16) -- one
rounding on the way out of what the fp32 kernel may compute (tests/deform_conv_cases.py's committed error model) -- with
ref = the fp64 oracle on the inputs rounded to the dtype; and out == rn16(ref) on >= 99 % of the elements, pooled per dtype
over the cases of a test.  tests/test_deform_conv_half.py shows on the CPU that this bar passes the two-term column and
refuses the column rounded to 16 bits once."""
import copy
import importlib

import pytest
import torch
import torch.nn.functional as F

import deform_conv_cases as cases
import deform_conv_half_cases as hc
from helpers import smooth_features

pytestmark = pytest.mark.gpu

ROUTE = "dc_fwd_mfma_half"
FP32_ROUTES = ("dc_fwd_mfma", "dc_fwd_generic")
IDS = ["f16", "bf16"]
TWO = ["k3_default", "k5x3_aniso"]


@pytest.fixture
def D():
    return importlib.import_module("mvdetr_amd.ops.deform_conv")


def device_inputs(name, dtype, kind="random", layout="cl"):
    (x, off, w, b), _, _ = hc.rounded_reference(name, dtype, kind)
    x = x.cuda()
    if layout == "cl":
        x = x.contiguous(memory_format=torch.channels_last)
    return x, off.cuda(), w.cuda(), None if b is None else b.cuda()


def run(D, name, dtype, kind="random", layout="cl"):
    args = device_inputs(name, dtype, kind, layout)            # (the cached reference takes the oracle's gradients: not under no_grad)
    with torch.no_grad():
        out = D.deform_conv2d(*args, **cases.by_name(name).conf)
    return out, D.last_kernel()


class Pool:
    """Checks the bar case by case (printing the figure first) and the pooled share of correctly rounded outputs at the end."""

    def __init__(self, dtype):
        self.dtype, self.eq, self.n = dtype, 0, 0

    def check(self, label, out, name, kind="random"):
        _, ref, bar = hc.rounded_reference(name, self.dtype, kind)
        r, e, m = hc.bar_ratio_and_equal(out, ref, bar, self.dtype)
        print(f"DCBAR {label} {name}/{kind} {self.dtype} out={r:.4f} rounded-equal {e}/{m}")
        assert r <= 1.0, (label, name, kind, r)
        self.eq, self.n = self.eq + e, self.n + m

    def done(self):
        print(f"DCBAR pooled {self.dtype} rounded-equal share {self.eq / self.n:.4f} of {self.n}")
        assert self.eq >= 0.99 * self.n, (self.eq, self.n)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_kernel_against_the_fp64_oracle(D, dtype):
    """All 12 MFMA cases, channel-last, random +-3 px offsets: blockIdx.y > 0 (C_out 160, 256), KC = 16 (C = 16, 48), a
    24-pixel output, pixel tiles across batch items, stride / dilation / padding remainders."""
    pool = Pool(dtype)
    for case in cases.MFMA_CASES:
        out, route = run(D, case.name, dtype)
        assert route == ROUTE, (case.name, route)
        pool.check(ROUTE, out, case.name)
    pool.done()


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_dyadic_offsets_nchw_inputs_and_the_generic_twins(D, dtype):
    """Taps exactly on integers, on -1 and on H / W (dyadic offsets: exact in either dtype); an NCHW input is copied to
    channel-last and gives the kernel's bits; the odd-channel / two-group twins run an fp32 route on the upcast."""
    pool = Pool(dtype)
    for case in cases.DYADIC_CASES:
        (_, off, _, _), _, _ = hc.rounded_reference(case.name, dtype, "dyadic")
        assert min(cases.on_grid(case, off.float())) > 0, case.name
        out, route = run(D, case.name, dtype, "dyadic")
        assert (route == ROUTE) == (case in cases.MFMA_CASES) and (route == ROUTE or route in FP32_ROUTES), (case.name, route)
        pool.check(route, out, case.name, "dyadic")
    for name in TWO:
        want, _ = run(D, name, dtype)
        out, route = run(D, name, dtype, layout="nchw")
        assert route == ROUTE and torch.equal(out, want), name
        pool.check(ROUTE + "/nchw", out, name)
        twin = next(c.name for c in cases.GENERIC_CASES if c.name.startswith(name))
        out, route = run(D, twin, dtype)
        assert route in FP32_ROUTES, (twin, route)
        pool.check(route, out, twin)
    pool.done()


@pytest.mark.parametrize("name", TWO)
@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_nonfinite_and_far_offsets_sample_zero(D, dtype, name):
    out, route = run(D, name, dtype, "nonfinite")
    moved, _ = run(D, name, dtype, "nonfinite_moved")
    assert route == ROUTE and torch.isfinite(out).all() and torch.equal(out, moved)
    pool = Pool(dtype)
    pool.check(ROUTE, out, name, "nonfinite")
    pool.done()


def test_float16_small_values(D):
    """x and bias x 2^-4: the column's lo terms (and some hi terms) are subnormal float16; same bar, same 99 %."""
    pool = Pool(torch.float16)
    for name in hc.SMALL_CASES:
        out, route = run(D, name, torch.float16, "random_small")
        assert route == ROUTE
        pool.check(ROUTE, out, name, "random_small")
    pool.done()


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_no_bias_relu_slices_and_reproducibility(D, dtype):
    name = "k3_default"
    case = cases.by_name(name)
    pool = Pool(dtype)
    out, route = run(D, name, dtype, "nobias")
    assert route == ROUTE
    pool.check(ROUTE, out, name, "nobias")
    want, _ = run(D, name, dtype)
    again, _ = run(D, name, dtype)
    assert torch.equal(want.view(torch.int16), again.view(torch.int16))                   # two runs: the same bits
    pool.check(ROUTE, want, name)
    pool.done()
    # the module: ReLU in the store, written into a channel slice of a larger tensor (batch stride 3 C_out H W, B = 2)
    x, off, w, b = device_inputs(name, dtype)
    m = D.DeformConv2d(case.C, case.C_out, (case.kh, case.kw), **case.conf).cuda().to(dtype).eval()
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
        assert torch.equal(m(x, off), want) and D.last_kernel() == ROUTE
        key = m._half_weight_cache[0]
        m(x, off)
        assert m._half_weight_cache[0] == key                                            # cached in eval mode ...
        m.weight.mul_(1.0)
        m(x, off)
        assert m._half_weight_cache[0] != key                                            # ... until the weight is written
        Co = case.C_out
        big = torch.full((case.B, 3 * Co, *case.out_hw), -7.0, dtype=dtype, device="cuda")
        D.last_kernel()
        m.forward_relu_into(x, off, big[:, Co:2 * Co])
        assert D.last_kernel() == ROUTE
    assert (want < 0).any() and torch.equal(big[:, Co:2 * Co], F.relu(want))
    assert (big[:, :Co] == -7).all() and (big[:, 2 * Co:] == -7).all()


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_what_the_kernel_does_not_take(D, dtype, monkeypatch):
    name = "k3_default"
    case = cases.by_name(name)
    x, off, w, b = device_inputs(name, dtype)
    pool = Pool(dtype)
    # a channel-last view whose data pointer is 2 bytes off 16-byte alignment: the fp32 route on the upcast
    flat = torch.zeros(x.numel() + 8, dtype=dtype, device="cuda")
    view = flat[1:1 + x.numel()].view(case.B, case.H, case.W, case.C).permute(0, 3, 1, 2)
    view.copy_(x)
    assert view.data_ptr() % 16 == 2 and view.is_contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        out = D.deform_conv2d(view, off, w, b, **case.conf)
    assert D.last_kernel() in FP32_ROUTES
    pool.check("misaligned/" + D.last_kernel(), out, name)
    # forward only
    with torch.enable_grad(), pytest.raises(RuntimeError, match="forward-only"):
        D.deform_conv2d(x, off, w.clone().requires_grad_(True), b, **case.conf)
    with torch.no_grad():
        D.deform_conv2d(x, off, w.clone().requires_grad_(True), b, **case.conf)
    assert D.last_kernel() == ROUTE
    # the knob, read per call
    monkeypatch.setenv("MVDETR_DEFORM_CONV_HALF", "0")
    with torch.no_grad():
        out = D.deform_conv2d(x, off, w, b, **case.conf)
    assert D.last_kernel() in FP32_ROUTES
    pool.check("knob/" + D.last_kernel(), out, name)
    pool.done()


def _model(dtype):
    """The mini geometry with a 128-channel bottleneck: the channel count of the Wildtrack model."""
    from mvdetr_amd.model import build_model
    return build_model("mini", seed=0, world_feat_arch="deform_conv", bottleneck_dim=128).cuda().to_inference(dtype)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_deform_conv_world_feat_in_16_bits(D, dtype, monkeypatch):
    """DeformConvWorldFeat on channel-last 16-bit input: RMS error against its own fp32 twin (the rounded parameters and
    input, upcast) of the kernel route and of the MVDETR_DEFORM_CONV_HALF=0 route (fp32 kernels on the upcast, rounded once).
    Bar: kernel <= 1.25 x upcast route -- the quarter is allowance for one seed's luck over ~10^4 elements
    (test_encoder_error_is_not_above_the_torch_compositions).  And the fused slices are the cat-of-ReLU composition's bits."""
    model = _model(dtype)
    wf = model.world_feat
    H, W = model.Rworld_shape
    x = smooth_features(model.num_cam, 128, H, W, seed=9).to(dtype).cuda().permute(0, 2, 3, 1).contiguous()[None]   # [1, N, H, W, C]
    ref_wf = copy.deepcopy(wf).float()
    with torch.no_grad():
        want = ref_wf(x.float()).cpu()
        assert D.last_kernel() == "dc_fwd_mfma"
        # the slices the kernel's store writes against the cat-of-ReLU composition on the very tensors each camera's
        # deformable convolution was given (the offset convolution and what follows the cat are torch's)
        seen, given = [], []
        hook = wf.merge_linear.register_forward_pre_hook(lambda mod, args: seen.append(args[0]))
        for dc in wf.deform_conv:
            def recording(input, offset, out, dc=dc, inner=dc.forward_relu_into):
                given.append((dc, input, offset))
                return inner(input, offset, out)
            monkeypatch.setattr(dc, "forward_relu_into", recording)
        hip = wf(x)
        hook.remove()
        assert D.last_kernel() == ROUTE and len(seen) == 1 and len(given) == model.num_cam
        comp = torch.cat([F.relu(dc(input, offset)) for dc, input, offset in given], 1)
        assert D.last_kernel() == ROUTE and seen[0].shape == comp.shape
        assert torch.equal(seen[0], comp) and (comp == 0).any() and (comp > 0).any()
        monkeypatch.setenv("MVDETR_DEFORM_CONV_HALF", "0")
        up = wf(x)
        assert D.last_kernel() in FP32_ROUTES
    assert hip.dtype == up.dtype == dtype and hip.shape == want.shape
    rms_hip = (hip.float().cpu() - want).pow(2).mean().sqrt().item()
    rms_up = (up.float().cpu() - want).pow(2).mean().sqrt().item()
    print(f"deform_conv aggregator RMS error vs fp32 ({dtype}): kernel {rms_hip:.3e}, upcast route {rms_up:.3e}, "
          f"output RMS {want.pow(2).mean().sqrt().item():.3e} over {want.numel()} elements")
    assert rms_hip <= 1.25 * rms_up, (rms_hip, rms_up)


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=IDS)
def test_deform_conv_model_forward_and_detect_in_16_bits(D, dtype):
    from mvdetr_amd.ops import warp
    model = _model(dtype)
    imgs = torch.rand(1, model.num_cam, 3, *model.geom.img_shape, generator=torch.Generator().manual_seed(2)).cuda()
    M = torch.eye(3).repeat(1, model.num_cam, 1, 1)
    with torch.no_grad():
        (hm, off), (ihm, ioff, iwh) = model(imgs, M)
    assert warp.last_kernel() == "warp_fwd_cl_half" and D.last_kernel() == ROUTE
    H, W = model.Rworld_shape
    assert hm.shape == (1, 1, H, W) and off.shape == (1, 2, H, W)
    for t_ in (hm, off, ihm, ioff, iwh):
        assert t_.dtype == dtype and torch.isfinite(t_).all()
    det = model.detect(imgs, M, cls_thres=0.05)
    assert type(det).__name__ == "Detections"
    assert det[0].dtype == torch.float32 and det[0].shape[0] == 1 and det[0].shape[-1] == 2
    assert det[1].dtype == torch.float32 and torch.isfinite(det[0]).all() and int(det[3][0]) >= 0
