"""The fused peak extraction on the device (csrc/peak_detect.hip): every case of tests/peak_detect_oracle.py against the oracle
and against the host path, the route each case took (candidate list in LDS, or in the workspace when a map has more candidates
than mvdetr_peak_detect_lds_capacity), run-to-run identity, layouts, launch counts, no host synchronise, and
MVDeTr.detect_views in fp32 and after to_inference(bfloat16).  No child processes.

Bars (peak_detect_oracle.py): cells, counts, positions, sizes, boxes and the zero tail bit-exact; scores to 1e-6 (fp32) /
1e-14 (fp64)."""
import importlib

import pytest
import torch

import peak_detect_oracle as P
from mvdetr_amd.ops import PeakDetections, peak_detect

peak_mod = importlib.import_module("mvdetr_amd.ops.peak_detect")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CACHE = {}


def _to(t):
    return None if t is None else t.to(DEV)


def _result(name):
    """The case on the device, run once -> (tensors on the CPU, route name)."""
    if name not in _CACHE:
        hm, off, wh, kw = P.make_case(name)
        det = peak_detect(_to(hm), _to(off), _to(wh), **kw)
        route = peak_mod.last_kernel()
        _CACHE[name] = (PeakDetections(*[None if t is None else t.cpu() for t in det]), route)
    return _CACHE[name]


@pytest.mark.parametrize("name", P.CASES)
def test_device_against_the_oracle_and_its_route(name):
    det, route = _result(name)
    hm, _, _, _ = P.make_case(name)
    P.assert_matches(det, name, hm)
    cap = peak_mod.lds_capacity(hm.dtype)
    most = max(w["count"] for w in P.expected(name))
    if name in P.WORKSPACE_ROUTE:
        assert 72 * 96 > cap and most > cap
    assert route == "peak_compact+peak_select" + ("_global" if most > cap else ""), (route, most, cap)


@pytest.mark.parametrize("name", P.CASES)
def test_device_equals_host_path(name):
    hm, off, wh, kw = P.make_case(name)
    host = peak_detect(hm, off, wh, **kw)
    det, _ = _result(name)
    for field, a, b in zip(det._fields, det, host):
        if field == "score":
            assert float((a - b).abs().max()) <= P.SCORE_TOL[hm.dtype]
        else:
            assert (a is None and b is None) or torch.equal(a, b), field


def test_two_runs_are_bitwise_identical_and_layouts_agree():
    for name in ("threshold", "constant_100"):                             # the LDS list and the workspace list
        hm, off, wh, kw = [_to(t) if torch.is_tensor(t) else t for t in P.make_case(name)]
        first = peak_detect(hm, off, wh, **kw)
        torch.randn(1 << 20, device=DEV).sum()                             # other work on the device in between
        second = peak_detect(hm, off, wh, **kw)
        cl = lambda t: t.contiguous(memory_format=torch.channels_last)     # noqa: E731
        assert cl(off).stride() != off.stride()
        B, _, H, W = hm.shape
        wide = torch.zeros(B, 3, H, 2 * W + 3, device=DEV)
        wide[:, 1:2, :, 2:2 * W + 2:2] = hm
        sliced = wide[:, 1:2, :, 2:2 * W + 2:2]
        assert not sliced.is_contiguous()
        for other in (second, peak_detect(cl(hm), cl(off), cl(wh), **kw), peak_detect(sliced, cl(off), wh, **kw)):
            assert all(torch.equal(a, b) for a, b in zip(first, other)), name


def test_peak_detect_launches_twice_and_does_not_synchronise():
    hm, off, wh, kw = [_to(t) if torch.is_tensor(t) else t for t in P.make_case("corners_and_edges")]
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)         # noqa: E731
    hm, off, wh = cl(hm), cl(off), cl(wh)
    peak_detect(hm, off, wh, **kw)                                          # library load
    torch.cuda.synchronize()
    n0 = peak_mod.launch_count()
    peak_detect(hm, off, wh, **kw)
    n1 = peak_mod.launch_count()
    peak_detect(hm, None, None, **kw)
    assert n1 - n0 == 2 and peak_mod.launch_count() - n1 == 2
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this build of torch has no torch.cuda.set_sync_debug_mode")
    try:
        torch.cuda.set_sync_debug_mode("error")
    except NotImplementedError as e:                                       # nothing else may drop the assertion
        pytest.skip(f"this build of torch does not implement torch.cuda.set_sync_debug_mode: {e}")
    try:
        det = peak_detect(hm, off, wh, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    P.assert_matches(det, "corners_and_edges", hm)


@pytest.mark.parametrize("half", [False, True])
def test_detect_views_matches_peak_detect_on_the_same_forward(half):
    """The maps come from a forward hook on the very forward detect_views runs (two forwards of one model need not agree to the
    last bit on the device); a to_inference model's 16-bit maps are upcast to float32, as detect_views upcasts them."""
    from mvdetr_amd import geometry
    from mvdetr_amd.model import build_model
    from mvdetr_amd.ops import bev_detect
    geom = geometry.MINI
    model = build_model("mini", seed=0, bottleneck_dim=128).to(DEV).eval()   # 16-channel heads, as the Wildtrack model's
    if half:
        model.to_inference(torch.bfloat16)
    g = torch.Generator().manual_seed(100)
    B, N = 2, geom.num_cam
    imgs = torch.randn(B, N, 3, *geom.input_img_shape, generator=g).to(DEV)
    M = geometry.random_affine_mats(B, N, geom.input_img_shape, seed=0, translate=0.05, scale=(0.9, 1.1))
    kw = dict(cls_thres=0.0, dist_thres=6, indexing=geom.indexing, max_det=64)
    seen = []
    hook = model.register_forward_hook(lambda module, args, out: seen.append(out))
    try:
        det, views = model.detect_views(imgs, M, view_top_k=20, **kw)
    finally:
        hook.remove()
    assert len(seen) == 1
    (whm, woff), (hm, off, wh) = seen[0]
    assert hm.dtype == (torch.bfloat16 if half else torch.float32)
    want_det = bev_detect(whm.float(), woff.float(), world_reduce=geom.world_reduce, **kw)
    assert all(torch.equal(a, b) for a, b in zip(det, want_det))
    want = peak_detect(hm.float(), off.float(), wh.float(), top_k=20, scale=geom.img_reduce)
    assert views.xy.shape == (B, N, 20, 2) and views.box.shape == (B, N, 20, 4) and views.count.shape == (B, N)
    assert views.xy.dtype == torch.float32 and views.count.device.type == "cuda" and int(views.count.min()) >= 1
    for a, b in zip(views, want):
        assert torch.equal(a.reshape(b.shape), b)
