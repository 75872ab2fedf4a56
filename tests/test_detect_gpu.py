"""The fused detection extraction on the device (csrc/detect.hip): the cases of tests/test_detect.py and the reference's 72
golden NMS cases against tests/detect_oracle.py on both routes (candidate list in LDS, the default where it fits; in the
workspace, MVDETR_DETECT_ROUTE=global -- the library reads the variable once, so that route runs in a child process: this
file as a script, `python test_detect_gpu.py <out.pt>`), equality with the host path, run-to-run identity, no host
synchronise, launch counts, and MVDeTr.detect against the reference's loop on the same forward's outputs.

Bars (detect_oracle.py): cells, counts and positions bit-exact; scores to 1e-6 (fp32) / 1e-14 (fp64)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]

import detect_oracle as D  # noqa: E402
from mvdetr_amd.ops import bev_detect, distance_nms  # noqa: E402
from mvdetr_amd.ops import detect as detect_mod  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUTES = ["default", "global"]


def _nms_cases():
    from conftest import load_golden
    from test_detect import nms_cases
    return nms_cases(load_golden("post.npz"))


def _run_all():
    """Every case on the device under this process's environment -> {name: tensors on the CPU}."""
    res = {}
    for name in D.CASES:
        hm, off, kw = D.make_case(name)
        det = bev_detect(hm.to(DEV), None if off is None else off.to(DEV), **D.call_kw(kw))
        res[name] = [t.cpu() for t in det]
        res["kernel:" + name] = detect_mod.last_kernel()
    nms = []
    for pts, sc, thres, topk, *_ in _nms_cases():
        keep, count = distance_nms(pts.to(DEV), sc.to(DEV), thres, topk)
        nms.append((keep.cpu(), count.cpu()))
    res["nms"] = nms
    res["kernel:nms"] = detect_mod.last_kernel()
    return res


_CACHE = {}


def _results(route):
    if route not in _CACHE:
        if route == "default":
            assert os.environ.get("MVDETR_DETECT_ROUTE", "") != "global"
            _CACHE[route] = _run_all()
        else:
            with tempfile.TemporaryDirectory() as tmp:
                out = os.path.join(tmp, "out.pt")
                subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, MVDETR_DETECT_ROUTE="global"),
                               check=True, timeout=300)
                _CACHE[route] = torch.load(out)
    return _CACHE[route]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", D.CASES)
def test_bev_detect_against_the_reference_chain(name, route):
    res = _results(route)
    hm, _, _ = D.make_case(name)
    D.assert_matches(detect_mod.Detections(*res[name]), name, hm)
    assert res["kernel:" + name] == ("detect_compact+detect_nms" + ("_global" if route == "global" else ""))


@pytest.mark.parametrize("route", ROUTES)
def test_distance_nms_on_the_reference_goldens(route):
    res = _results(route)
    cases = _nms_cases()
    assert len(cases) == len(res["nms"]) == 72
    for i, ((_, _, _, _, keep, count, _), (got_keep, got_count)) in enumerate(zip(cases, res["nms"])):
        assert int(got_count) == count and got_keep.dtype == torch.long and got_keep.tolist() == keep, i
    assert res["kernel:nms"] == ("distance_nms" + ("_global" if route == "global" else ""))


@pytest.mark.parametrize("name", D.CASES)
def test_device_equals_host_path(name):
    hm, off, kw = D.make_case(name)
    host = bev_detect(hm, off, **D.call_kw(kw))
    xy, score, cell, count = _results("default")[name]
    assert torch.equal(count, host.count) and torch.equal(cell, host.cell) and torch.equal(xy, host.xy)
    assert float((score - host.score).abs().max()) <= D.SCORE_TOL[hm.dtype]


def test_two_runs_are_bitwise_identical_and_layouts_agree():
    hm, off, kw = D.make_case("all_above")
    hm, off = hm.to(DEV), off.to(DEV)
    first = bev_detect(hm, off, **D.call_kw(kw))
    torch.randn(1 << 20, device=DEV).sum()                                             # other work on the device in between
    second = bev_detect(hm, off, **D.call_kw(kw))
    cl = bev_detect(hm.contiguous(memory_format=torch.channels_last), off.contiguous(memory_format=torch.channels_last),
                    **D.call_kw(kw))
    wide = torch.zeros(2, 3, 24, 83, device=DEV)
    wide[:, 1:2, :, 2:82:2] = hm
    sliced = bev_detect(wide[:, 1:2, :, 2:82:2], off, **D.call_kw(kw))
    for other in (second, cl, sliced):
        assert all(torch.equal(a, b) for a, b in zip(first, other))
    pts, sc = torch.randn(5000, 2, device=DEV) * 300, torch.rand(5000, device=DEV)      # beyond the LDS list: the workspace route
    a, b = distance_nms(pts, sc, 20, float("inf")), distance_nms(pts, sc, 20, float("inf"))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int(a[1]) > 1000
    host = distance_nms(pts.cpu(), sc.cpu(), 20, float("inf"))
    assert torch.equal(a[0].cpu(), host[0]) and int(a[1]) == int(host[1])


def test_bev_detect_does_not_synchronise_and_launches_twice():
    hm, off, kw = D.make_case("one_frame_empty")
    hm, off = hm.to(DEV).contiguous(memory_format=torch.channels_last), off.to(DEV).contiguous(memory_format=torch.channels_last)
    bev_detect(hm, off, **D.call_kw(kw))                                                # library load
    torch.cuda.synchronize()
    n0 = detect_mod.launch_count()
    bev_detect(hm, off, **D.call_kw(kw))
    n1 = detect_mod.launch_count()
    distance_nms(off[0, :, 0].t().contiguous(), hm[0, 0, 0].contiguous(), 20, 50)
    assert 1 <= n1 - n0 <= 2 and detect_mod.launch_count() - n1 == 1
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this build of torch has no torch.cuda.set_sync_debug_mode")
    try:
        torch.cuda.set_sync_debug_mode("error")
    except NotImplementedError as e:                                                   # nothing else may drop the assertion
        pytest.skip(f"this build of torch does not implement torch.cuda.set_sync_debug_mode: {e}")
    try:
        det = bev_detect(hm, off, **D.call_kw(kw))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    D.assert_matches(det, "one_frame_empty", hm)


def model_detect_matches_loop(device):
    """MVDeTr.detect on the mini model against detections_from_heatmap on the same forward's outputs copied to the CPU: a
    forward hook hands over the maps of the forward that detect itself runs (two forwards of one model on the same input need
    not agree to the last bit on the device, and a position is compared bit for bit).  A seeded random model's logits sit far
    below 0.4, so the threshold is put halfway between the 40th and 41st highest score of a forward run beforehand; a seed
    whose copied maps have candidate scores closer than 2e-6 to each other (the devices' sigmoids differ by up to 1e-6) or
    within 1e-5 of the threshold is passed over, the comparison is never relaxed."""
    from mvdetr_amd import geometry
    from mvdetr_amd.model import build_model
    from mvdetr_amd.utils import detections_from_heatmap
    geom = geometry.MINI
    for seed in range(5):
        model = build_model("mini", seed=seed, channels_last=device != "cpu").to(device).eval()
        g = torch.Generator().manual_seed(100 + seed)
        imgs = torch.randn(2, geom.num_cam, 3, *geom.input_img_shape, generator=g).to(device)
        M = geometry.random_affine_mats(2, geom.num_cam, geom.input_img_shape, seed=seed, translate=0.05, scale=(0.9, 1.1))
        with torch.no_grad():
            (hm, off), _ = model(imgs, M)
        s = torch.sigmoid(hm.cpu()).flatten().sort(descending=True)[0]
        thres = float((s[39].double() + s[40].double()) / 2)
        kw = dict(cls_thres=thres, dist_thres=6, indexing=geom.indexing)
        seen = []
        hook = model.register_forward_hook(lambda module, args, out: seen.append(out[0]))
        try:
            det = model.detect(imgs, M, **kw)
        finally:
            hook.remove()
        assert len(seen) == 1
        hm, off = seen[0]
        s = torch.sigmoid(hm.cpu()).flatten().sort(descending=True)[0].double()
        cand, rest = s[s > thres], s[s <= thres]
        if (len(cand) < 5 or float(cand[-1] - thres) < 1e-5 or float(thres - rest[0]) < 1e-5
                or float((cand[:-1] - cand[1:]).min()) < 2e-6):
            continue
        assert det.count.device.type == torch.device(device).type and int(det.count.sum()) > 4
        want = detections_from_heatmap(hm.cpu(), off.cpu(), [7, 9], world_reduce=geom.world_reduce, **kw)
        rows = [torch.cat([torch.full((int(c), 1), float(f)), det.xy[b, :int(c)].cpu()], 1) for b, (c, f) in enumerate(zip(det.count.cpu(), [7, 9]))]
        assert torch.equal(torch.cat(rows), want)
        return
    raise AssertionError("no seed gave separated scores")


def test_model_detect_matches_the_reference_loop_on_the_same_outputs():
    model_detect_matches_loop(DEV)


if __name__ == "__main__":
    torch.save(_run_all(), sys.argv[1])
