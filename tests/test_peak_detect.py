"""Per-view detections on the CPU: utils.ctdet_decode against the reference's own goldens (tests/golden/ctdet.npz), the fused
peak extraction's host path (csrc/host_path.cpp) against tests/peak_detect_oracle.py on every case, ctdet_decode_fused against
ctdet_decode, the refusals, non-finite logits, and MVDeTr.detect_views.  tests/test_peak_detect_gpu.py runs the same cases on
the kernels.  Bars (peak_detect_oracle.py): cells, counts, positions, sizes, boxes and the zero tail bit-exact; scores to 1e-6
(fp32) / 1e-14 (fp64)."""
import numpy as np
import pytest
import torch

import peak_detect_oracle as P
from conftest import load_golden
from mvdetr_amd import _lib
from mvdetr_amd.ops import PeakDetections, peak_detect
from mvdetr_amd.utils import ctdet_decode, ctdet_decode_fused


@pytest.fixture(scope="module")
def gold():
    return load_golden("ctdet.npz")


def golden_cases(gold):
    for i in range(int(gold["ctdet_cases"])):
        t = lambda k: torch.from_numpy(gold[f"ctdet_{i}_{k}"]) if f"ctdet_{i}_{k}" in gold else None  # noqa: E731
        yield i, t("heatmap"), t("offset"), t("wh"), int(gold[f"ctdet_{i}_top_K"]), t("out")


def test_ctdet_decode_equals_the_reference_on_its_goldens(gold):
    seen = set()
    for i, hm, off, wh, top_K, want in golden_cases(gold):
        got = ctdet_decode(hm, off, wh, top_K=top_K)
        assert got.shape == want.shape == (hm.shape[0], top_K, 3 if wh is None else 5) and got.dtype == want.dtype
        pos = want[..., -1] > 0
        # positions and sizes are gathers and one add: the same bits.  The score is torch's own sigmoid, whose vectorised
        # kernel may differ in the last place between instruction sets: the project's bar for a sigmoid (1e-6 in fp32).
        assert torch.equal(got[pos][:, :-1], want[pos][:, :-1]), i
        assert float((got[..., -1] - want[..., -1]).abs().max()) <= P.SCORE_TOL[torch.float32], i
        assert torch.equal(got[..., -1] > 0, pos), i                        # and zero scores past the last candidate
        seen.add((hm.shape[1], int(pos.sum(1).min()), off is None, wh is None))
    assert {(1, 100, False, False), (1, 100, True, True), (1, 31, False, False), (1, 31, True, True), (2, 100, False, False)} <= seen
    assert {(1, 100, True, False), (1, 100, False, True)} <= seen


def test_ctdet_decode_refuses_the_id_branch():
    with pytest.raises(NotImplementedError):
        ctdet_decode(torch.zeros(1, 1, 4, 4), id=torch.zeros(1, 3, 4, 4), top_K=4)


@pytest.mark.parametrize("name", P.CASES)
def test_host_path_against_the_oracle(name):
    hm, off, wh, kw = P.make_case(name)
    P.assert_matches(peak_detect(hm, off, wh, **kw), name, hm)


def test_cases_are_what_they_say():
    lib = _lib.lib()
    assert [w["count"] for w in P.expected("corners_and_edges")][:2] == [8, 1]
    assert sorted(P.expected("corners_and_edges")[0]["cell"].tolist()) == sorted([0, 6, 28, 34, 3, 14, 20, 31])
    flat = set(P.expected("plateau")[0]["cell"][:20].tolist())
    assert flat == {r * 12 + c for r in range(2, 6) for c in range(3, 8)}
    assert P.expected("plateau")[1]["cell"][0] == 3 * 12 + 4
    assert not {2 * 12 + 3, 2 * 12 + 4, 2 * 12 + 5, 3 * 12 + 3, 4 * 12 + 4} & set(P.expected("plateau")[1]["cell"].tolist())
    c, W = P.RUN, 48
    seam = P.expected("seam")
    assert {c - 1, c} <= set(seam[0]["cell"].tolist())
    assert {c, c - W, c - 6, c - 6 + W} <= set(seam[1]["cell"].tolist())
    assert {c - 1, c + 3} <= set(seam[2]["cell"].tolist()) and not {c + W, c + 2 - W} & set(seam[2]["cell"].tolist())
    for name in P.WORKSPACE_ROUTE:
        hm, _, _, kw = P.make_case(name)
        cells = hm.shape[2] * hm.shape[3]
        assert cells == 72 * 96 > lib.mvdetr_peak_detect_lds_capacity(hm.element_size())
        for w in P.expected(name):
            assert w["count"] == cells and w["cell"].tolist() == list(range(cells - 1, cells - 1 - kw["top_k"], -1))
    for name in ("top_9", "top_50"):                                       # of the three equal scores on the cut, the highest cell
        (w,), k = P.expected(name), int(name[4:])
        hm = P.make_case(name)[0].view(-1)
        tied = torch.nonzero(hm == (256 - k) / 32).view(-1).tolist()
        assert len(tied) == 3 and w["cell"][-1] == max(tied) and w["count"] > k + 20


def test_fused_decode_equals_ctdet_decode_below_count(gold):
    ran = 0
    for i, hm, off, wh, top_K, _ in golden_cases(gold):
        if hm.shape[1] != 1:
            with pytest.raises(RuntimeError, match="one channel"):
                ctdet_decode_fused(hm, off, wh, top_K=top_K)
            continue
        want, got = ctdet_decode(hm, off, wh, top_K=top_K), ctdet_decode_fused(hm, off, wh, top_K=top_K)
        count = peak_detect(hm, off, wh, top_k=top_K).count
        assert got.shape == want.shape and got.dtype == want.dtype
        for b in range(hm.shape[0]):
            m = min(int(count[b]), top_K)
            assert m in (31, 100)
            # positions, sizes: the same bits; scores: torch's vectorised sigmoid against 1 / (1 + exp(-x))
            assert torch.equal(got[b, :m, :-1], want[b, :m, :-1]), i
            assert float((got[b, :m, -1] - want[b, :m, -1]).abs().max()) <= P.SCORE_TOL[torch.float32], i
            assert not got[b, m:].any()
        ran += 1
    assert ran >= 6


def test_layouts_give_the_same_answer():
    hm, off, wh, kw = P.make_case("threshold")
    want = peak_detect(hm, off, wh, **kw)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)  # noqa: E731
    assert cl(off).stride() != off.stride()
    wide = torch.zeros(2, 3, 24, 83)
    wide[:, 1:2, :, 2:82:2] = hm
    sliced = wide[:, 1:2, :, 2:82:2]
    assert not sliced.is_contiguous()
    for got in (peak_detect(cl(hm), cl(off), cl(wh), **kw), peak_detect(sliced, cl(off), wh, **kw)):
        assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_misuse_raises():
    hm, off, wh, _ = P.make_case("corners_and_edges")
    bad = [lambda: peak_detect(hm[:, 0], off, wh),                          # rank
           lambda: peak_detect(hm, off[:, :1], wh),                         # shapes
           lambda: peak_detect(hm, off, wh[..., :-1]),
           lambda: peak_detect(hm, off[:2], wh),
           lambda: peak_detect(torch.cat([hm, hm], 1), off, wh),            # more than one heat-map channel
           lambda: peak_detect(hm, off.double(), wh),                       # mixed dtype
           lambda: peak_detect(hm, off, wh.double()),
           lambda: peak_detect(hm.half(), off.half(), wh.half()),           # 16-bit
           lambda: peak_detect(hm.bfloat16(), None, None),
           lambda: peak_detect(hm, off, wh, top_k=0),
           lambda: peak_detect(hm, off, wh, top_k=1025),
           lambda: peak_detect(hm[:0], off[:0], wh[:0]),                    # empty
           lambda: peak_detect(hm[..., :0], off[..., :0], wh[..., :0])]
    for call in bad:
        with pytest.raises(RuntimeError):
            call()
    if torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="share device"):
            peak_detect(hm, off.cuda(), wh)
    det = peak_detect(hm.clone().requires_grad_(True), off, wh, top_k=1024)
    assert not det.xy.requires_grad and det.xy.shape == (3, 1024, 2) and det.box.shape == (3, 1024, 4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_non_finite_logits_neither_fault_nor_hide_distant_peaks(dtype):
    g = torch.Generator().manual_seed(11)
    hm = P.lattice((2, 1, 12, 16), g, -256, -64).to(dtype)
    hm[0, 0, 2, 3], hm[0, 0, 2, 9], hm[0, 0, 6, 12] = float("nan"), float("inf"), float("-inf")
    hm[0, 0, 0, 0], hm[0, 0, 11, 15] = float("nan"), float("nan")
    hm[1] = float("nan")
    peaks = [(2, 5, 3.0), (4, 3, 2.0), (9, 9, 1.0), (6, 14, 0.5)]           # two or more cells away from every NaN
    for r, c, v in peaks:
        hm[0, 0, r, c] = v
    det = peak_detect(hm, top_k=200)
    assert det.count.tolist()[1] == 0 and 5 <= int(det.count[0]) <= 12 * 16
    cells = det.cell[0, :int(det.count[0])].tolist()
    assert cells[0] == 2 * 16 + 9 and float(det.score[0, 0]) == 1.0         # +inf: score 1
    assert cells[1:5] == [r * 16 + c for r, c, _ in peaks]
    assert not {2 * 16 + 3, 0, 11 * 16 + 15} & set(cells)                   # a NaN is never a candidate
    assert torch.isfinite(det.score).all() and not det.score[1].any()


def test_detect_views_on_a_small_model():
    from mvdetr_amd import geometry
    from mvdetr_amd.model import build_model
    geom = geometry.MINI
    model = build_model("mini", seed=0).eval()
    g = torch.Generator().manual_seed(100)
    B, N = 2, geom.num_cam
    imgs = torch.randn(B, N, 3, *geom.input_img_shape, generator=g)
    M = geometry.random_affine_mats(B, N, geom.input_img_shape, seed=0, translate=0.05, scale=(0.9, 1.1))
    kw = dict(cls_thres=0.0, dist_thres=6, indexing=geom.indexing, max_det=64)
    seen = []
    hook = model.register_forward_hook(lambda module, args, out: seen.append(out))
    try:
        det, views = model.detect_views(imgs, M, view_top_k=20, **kw)
    finally:
        hook.remove()
    assert len(seen) == 1                                                   # one forward serves both results
    want_det = model.detect(imgs, M, **kw)
    assert all(torch.equal(a, b) for a, b in zip(det, want_det))
    _, (hm, off, wh) = seen[0]
    want = peak_detect(hm, off, wh, top_k=20, scale=geom.img_reduce)
    assert isinstance(views, PeakDetections)
    assert views.xy.shape == (B, N, 20, 2) and views.wh.shape == (B, N, 20, 2) and views.box.shape == (B, N, 20, 4)
    assert views.score.shape == views.cell.shape == (B, N, 20) and views.count.shape == (B, N)
    assert int(views.count.min()) >= 1
    for a, b in zip(views, want):
        assert torch.equal(a.reshape(b.shape), b)
    thres = float(torch.sigmoid(hm).median())
    _, cut = model.detect_views(imgs, M, view_top_k=20, view_cls_thres=thres, **kw)
    assert torch.equal(cut.count.view(-1), peak_detect(hm, off, wh, top_k=20, cls_thres=thres).count)
    assert int(cut.count.sum()) < int(views.count.sum())


def test_new_symbols_are_declared_and_the_abi_version_stays():
    names = ["mvdetr_peak_detect_workspace_bytes", "mvdetr_peak_detect_lds_capacity", "mvdetr_peak_detect_last_kernel",
             "mvdetr_peak_detect_launch_count"]
    names += [f"mvdetr_peak_detect_forward{host}_{t}" for host in ("", "_host") for t in ("f32", "f64")]
    assert set(names) <= set(_lib.SIGNATURES) and _lib.ABI_VERSION == 18
    lib = _lib.lib()
    assert lib.mvdetr_ops_abi_version() == 18
    assert lib.mvdetr_peak_detect_workspace_bytes(7, 90, 160, 4) > 0 and lib.mvdetr_peak_detect_workspace_bytes(1, 0, 160, 4) < 0
    assert lib.mvdetr_peak_detect_workspace_bytes(1, 90, 160, 2) < 0 and lib.mvdetr_peak_detect_lds_capacity(2) < 0
    assert lib.mvdetr_peak_detect_lds_capacity(4) >= 1024 and lib.mvdetr_peak_detect_lds_capacity(8) >= 1024
    assert np.dtype(np.int32).itemsize == 4
