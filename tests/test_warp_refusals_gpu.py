"""What the warp's C ABI refuses, and what it accepts without launching anything (csrc/warp_route.h decides; tests/test_warp_route.py
pins the whole table on the CPU).  Here the library itself is called, with tensors of a few hundred elements whose shapes are
the ones the calls state: the return codes (0, 1 = hipErrorInvalidValue, 801 = hipErrorNotSupported), that
mvdetr_warp_last_kernel() is left alone by a refused or empty call, and that a backward without destination pixels really
zeroes grad_src.  Every call returns before any kernel launch, except the zero-fill's memset and the one small forward that
gives mvdetr_warp_last_kernel() a known value first."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

N, C, h, w, H, W = 1, 8, 5, 6, 7, 9
INVALID, NOT_SUPPORTED = 1, 801


@pytest.fixture(scope="module")
def lib():
    from mvdetr_amd import _lib
    return _lib


class Case:
    """Tensors of one dtype at the shapes above, the entries bound to the current stream, and `odd`: a channel count inside the
    tensors that leaves a partial 16-byte chunk per pixel (6 floats, 3 doubles)."""

    def __init__(self, _lib, dtype):
        dev = torch.device("cuda:0")
        self._lib, self.lib, self.dtype = _lib, _lib.lib(), dtype
        self.half = dtype in (torch.float16, torch.bfloat16)
        self.sfx = _lib.suffix(dtype, half_ok=True)
        self.odd = 3 if dtype == torch.float64 else 6
        self.stream = _lib.current_stream_ptr(dev)
        self.src = torch.randn(N * C * h * w + 4, device=dev).to(dtype)           # (+ 4: room for a misaligned view)
        self.dst = torch.empty(N * C * H * W + 4, device=dev, dtype=dtype)
        self.M = torch.eye(3, device=dev, dtype=torch.float32 if self.half else dtype).repeat(N, 1, 1).contiguous()
        assert self.src.data_ptr() % 16 == 0 and self.dst.data_ptr() % 16 == 0

    def call(self, name, a, M, o, *, n=N, c=C, sh=h, sw=w, dh=H, dw=W, layout=0):
        return getattr(self.lib, f"mvdetr_warp_perspective_{name}_{self.sfx}")(self.stream, a, M, n, c, sh, sw, dh, dw, layout, o)

    def forward(self, **kw):
        return self.call("forward", kw.pop("a", self.src.data_ptr()), kw.pop("M", self.M.data_ptr()), kw.pop("o", self.dst.data_ptr()), **kw)

    def backward(self, **kw):
        return self.call("backward", kw.pop("a", self.dst.data_ptr()), kw.pop("M", self.M.data_ptr()), kw.pop("o", self.src.data_ptr()), **kw)

    def last(self):
        return self.lib.mvdetr_warp_last_kernel().decode()


def _case(lib, dtype):
    c = Case(lib, dtype)
    assert c.forward() == 0                                                       # one real launch: a known last kernel
    torch.cuda.synchronize()
    assert c.last() == ("warp_fwd_half" if c.half else "warp_fwd<NCHW>")
    return c


_name = lambda d: str(d).split(".")[-1]


@pytest.fixture(scope="module", params=[torch.float32, torch.float64, torch.float16, torch.bfloat16], ids=_name)
def case(lib, request):
    """Every forward entry."""
    return _case(lib, request.param)


@pytest.fixture(scope="module", params=[torch.float32, torch.float64], ids=_name)
def fcase(lib, request):
    """The types that have a backward and a not_supported answer."""
    return _case(lib, request.param)


def _unchanged(case, rc, want):
    assert rc == want
    assert case.last() == ("warp_fwd_half" if case.half else "warp_fwd<NCHW>")


@pytest.mark.parametrize("kw", [dict(n=-1), dict(c=-1), dict(dh=-1), dict(dw=-1), dict(sh=0), dict(sw=0), dict(sh=-1), dict(layout=8),
                                dict(layout=8, dh=0), dict(a=None), dict(M=None), dict(o=None)], ids=str)
def test_forward_invalid_value(case, kw):
    _unchanged(case, case.forward(**kw), INVALID)


@pytest.mark.parametrize("kw", [dict(n=0), dict(c=0), dict(dh=0), dict(dw=0), dict(dh=0, a=None, M=None, o=None),
                                dict(c=0, layout=3)], ids=str)
def test_forward_empty(case, kw):
    _unchanged(case, case.forward(**kw), 0)


def test_forward_channel_last_refusals(fcase):
    """A channel-last source wants whole 16-byte chunks per pixel and 16-byte aligned tensors; an NCHW destination is served
    for fp32 only.  The 16-bit entry refuses none of it: warp_fwd_half takes those calls (tests/test_half_edges_gpu.py)."""
    case = fcase
    es = case.src.element_size()
    for layout in (2, 3):
        _unchanged(case, case.forward(layout=layout, c=case.odd), NOT_SUPPORTED)  # 24 bytes per pixel
        _unchanged(case, case.forward(layout=layout, a=case.src.data_ptr() + es), NOT_SUPPORTED)
        _unchanged(case, case.forward(layout=layout, o=case.dst.data_ptr() + es), NOT_SUPPORTED)
    if case.dtype == torch.float64:
        _unchanged(case, case.forward(layout=2), NOT_SUPPORTED)
    _unchanged(case, case.forward(layout=3, c=case.odd, a=None), INVALID)         # the pointers come first


def test_backward_refusals_and_empty_calls(fcase):
    case = fcase
    es = case.src.element_size()
    for kw in (dict(n=-1), dict(sh=0), dict(layout=8), dict(a=None), dict(M=None), dict(o=None), dict(dh=0, o=None), dict(c=0, layout=8)):
        _unchanged(case, case.backward(**kw), INVALID)
    for kw in (dict(c=0), dict(n=0), dict(c=0, a=None, M=None, o=None), dict(n=0, dh=0, layout=3, c=6)):
        _unchanged(case, case.backward(**kw), 0)                                  # an empty grad_src: nothing to do
    for kw in (dict(layout=2), dict(layout=6), dict(layout=3, c=case.odd), dict(layout=3, a=case.dst.data_ptr() + es),
               dict(layout=3, o=case.src.data_ptr() + es)):
        _unchanged(case, case.backward(**kw), NOT_SUPPORTED)


@pytest.mark.parametrize("kw", [dict(dh=0), dict(dw=0), dict(dh=0, layout=1), dict(dh=0, layout=3), dict(dw=0, layout=3, c=6, a=None, M=None)],
                         ids=str)
def test_backward_without_destination_pixels_zeroes_grad_src(fcase, kw):
    case = fcase
    c = kw.get("c", C)
    grad_src = torch.full((N * C * h * w,), float("nan"), device="cuda:0", dtype=case.dtype)
    _unchanged(case, case.backward(o=grad_src.data_ptr(), **kw), 0)
    torch.cuda.synchronize()
    assert torch.equal(grad_src[:N * c * h * w], torch.zeros_like(grad_src[:N * c * h * w]))
    assert torch.isnan(grad_src[N * c * h * w:]).all()                            # and nothing beyond what the call states


def test_plan_entries(fcase):
    case = fcase
    lib, es = case.lib, case.src.element_size()
    sfx = case.sfx
    nbytes = lib.mvdetr_warp_backward_plan_bytes(N, C, h, w, H, W, es)
    # [1026 counters | 2 scans of 40 bytes per 2 x 2 block of the 5 x 6 source | the block list | 1024 pixel-list segments]
    assert nbytes == 4112 + 9 * 80 + 48 + 4096
    for args in ((0, C, h, w, H, W, es), (N, 0, h, w, H, W, es), (N, C, 0, w, H, W, es), (N, C, h, -1, H, W, es), (N, C, h, w, 0, W, es),
                 (N, C, h, w, H, 0, es), (N, C, h, w, H, W, 2), (N, C, h, w, H, W, 16), (N, case.odd, h, w, H, W, es)):
        assert lib.mvdetr_warp_backward_plan_bytes(*args) == 0, args
    plan = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda:0")
    build = getattr(lib, f"mvdetr_warp_backward_plan_{sfx}")
    planned = getattr(lib, f"mvdetr_warp_perspective_backward_planned_{sfx}")
    M, g, o, p = case.M.data_ptr(), case.dst.data_ptr(), case.src.data_ptr(), plan.data_ptr()
    _unchanged(case, build(case.stream, None, N, C, h, w, H, W, p), INVALID)
    _unchanged(case, build(case.stream, M, N, C, h, w, H, W, None), INVALID)
    _unchanged(case, build(case.stream, M, N, C, h, w, H, W, p + 8), INVALID)                      # a misaligned plan
    _unchanged(case, build(case.stream, M, 0, C, h, w, H, W, p + 8), INVALID)                      # the pointers come first
    _unchanged(case, build(case.stream, M, 0, C, h, w, H, W, p), NOT_SUPPORTED)
    _unchanged(case, build(case.stream, M, N, case.odd, h, w, H, W, p), NOT_SUPPORTED)
    for layout in (0, 1, 2, 4, 8):
        _unchanged(case, planned(case.stream, g, M, p, N, C, h, w, H, W, layout, o), INVALID)
    for bad in ((None, M, p, o), (g, None, p, o), (g, M, None, o), (g, M, p, None)):
        _unchanged(case, planned(case.stream, bad[0], bad[1], bad[2], N, C, h, w, H, W, 3, bad[3]), INVALID)
    _unchanged(case, planned(case.stream, g, M, p, 0, C, h, w, H, W, 3, o), NOT_SUPPORTED)
    _unchanged(case, planned(case.stream, g, M, p, N, case.odd, h, w, H, W, 3, o), NOT_SUPPORTED)
    _unchanged(case, planned(case.stream, g + es, M, p, N, C, h, w, H, W, 3, o), NOT_SUPPORTED)
    _unchanged(case, planned(case.stream, g, M, p, N, C, h, w, H, W, 7, o + es), NOT_SUPPORTED)
    # MVDETR_WARP_BWD_IMPL=scatter switches the two-step gradient off (the knob is read on every call)
    os.environ["MVDETR_WARP_BWD_IMPL"] = "scatter"
    try:
        assert lib.mvdetr_warp_backward_plan_bytes(N, C, h, w, H, W, es) == 0
        _unchanged(case, build(case.stream, M, N, C, h, w, H, W, p), NOT_SUPPORTED)
        _unchanged(case, planned(case.stream, g, M, p, N, C, h, w, H, W, 3, o), NOT_SUPPORTED)
    finally:
        del os.environ["MVDETR_WARP_BWD_IMPL"]
    assert lib.mvdetr_warp_backward_plan_bytes(N, C, h, w, H, W, es) == nbytes
    torch.cuda.synchronize()
