"""The fused detection extraction on the library's host path (csrc/host_path.cpp): ops.bev_detect / ops.distance_nms, the
utils built on them, MVDeTr-shaped test loop.  Expected values: tests/detect_oracle.py (cells, counts and positions bit-exact,
scores to 1e-6 in fp32 / 1e-14 in fp64: one fp32 ulp at 1 is 6e-8 and torch's vectorised sigmoid already differs from
1 / (1 + exp(-x)) by 1.2e-7 on the CPU).  tests/test_detect_gpu.py runs the same cases on the kernels."""
import numpy as np
import pytest
import torch

import detect_oracle as D
from conftest import load_golden
from oracle import post_oracle
from mvdetr_amd import _lib
from mvdetr_amd.ops import bev_detect, distance_nms
from mvdetr_amd.utils import detections_from_heatmap, detections_from_heatmap_fused, nms, nms_fused


@pytest.fixture(scope="module")
def gold():
    return load_golden("post.npz")


def nms_cases(gold):
    """-> [(points, scores, dist_thres, top_k, expected keep, expected count, tied)] for the 72 golden cases: the reference's
    own answer where no two scores are equal, the loop checker's under the library's tie rule where some are."""
    out = []
    for i in range(int(gold["nms_cases"])):
        pts, sc = torch.from_numpy(gold[f"nms_{i}_points"]), torch.from_numpy(gold[f"nms_{i}_scores"])
        thres, topk = [float(v) for v in gold[f"nms_{i}_args"]]
        tied = len(np.unique(sc.numpy())) < sc.numel()
        if tied:
            keep, count = post_oracle.nms(pts.tolist(), sc.tolist(), thres, topk, order=None)
        else:
            keep, count = gold[f"nms_{i}_keep"].tolist(), int(gold[f"nms_{i}_count"])
        out.append((pts, sc, thres, topk, keep, count, tied))
    return out


def test_golden_fixture_split(gold):
    cases = nms_cases(gold)
    assert len(cases) == 72 and sum(c[6] for c in cases) == 9


def test_distance_nms_on_the_reference_goldens(gold):
    for i, (pts, sc, thres, topk, keep, count, _) in enumerate(nms_cases(gold)):
        got_keep, got_count = distance_nms(pts, sc, thres, topk)
        assert got_keep.dtype == torch.long and got_count.dtype == torch.int32
        assert int(got_count) == count and got_keep.tolist() == keep, i
        k2, c2 = nms_fused(pts, sc, thres, topk)
        assert isinstance(c2, int) and c2 == count and k2.tolist() == keep, i
        k3, c3 = distance_nms(pts.double(), sc.double(), thres, topk)
        assert int(c3) == count and k3.tolist() == keep, i


def test_nms_fused_contract_edges():
    keep, count = nms_fused(torch.zeros(0, 2), torch.zeros(0))
    assert count == 0 and keep.shape == (0,) and keep.dtype == torch.long
    assert nms_fused(torch.zeros(1, 2), torch.ones(1))[1] == 1
    pts, sc = torch.randn(40, 2, generator=torch.Generator().manual_seed(1)) * 100, torch.arange(40.0)
    assert nms_fused(pts, sc, 0.0, 7)[1] == 7
    assert torch.equal(nms_fused(pts, sc, 20, float("inf"))[0], nms(pts, sc, 20, float("inf"))[0])
    with pytest.raises(RuntimeError):
        nms_fused(pts, sc[:10])
    with pytest.raises(RuntimeError):
        distance_nms(pts, sc.double())


@pytest.mark.parametrize("name", D.CASES)
def test_bev_detect_against_the_reference_chain(name):
    hm, off, kw = D.make_case(name)
    D.assert_matches(bev_detect(hm, off, **D.call_kw(kw)), name, hm)


def test_exact_distance_case_is_what_it_says():
    (cells, pos, _), = D.expected("exact_distance")
    assert cells.tolist() == [2 * 24 + 3, 12 * 24 + 3, 12 * 24 + 9]          # the peak exactly 20 away is gone, the one 24 away stays
    assert pos.tolist() == [[12.0, 8.0], [12.0, 48.0], [36.0, 48.0]]


@pytest.mark.parametrize("name", ["plateau", "top9", "top50"])
def test_tie_cases_depend_on_the_tie_rule(name):
    """The opposite rule (equal scores: lower index first) gives another answer: the case does exercise the rule."""
    hm, off, kw = D.make_case(name)
    s = torch.sigmoid(hm)
    rows = post_oracle.mvdet_decode(s.numpy(), off.numpy(), D.REDUCE)
    differs = False
    for b, (cells, _, _) in enumerate(D.expected(name)):
        sel = np.nonzero(s[b, 0].reshape(-1).numpy() > np.float32(D.CLS_THRES))[0]
        sc = s[b, 0].reshape(-1).numpy()[sel]
        order = sorted(range(len(sel)), key=lambda i: (sc[i], -i))
        keep, count = post_oracle.nms(rows[b, sel, :2].tolist(), sc.tolist(), kw.get("dist_thres", D.DIST_THRES), kw.get("top_k", float("inf")), order=order)
        differs |= sel[keep[:count]].tolist() != cells.tolist()
    assert differs


def test_max_det_truncates_rows_and_keeps_the_true_count():
    hm, off, kw = D.make_case("all_above_cap5")
    det = bev_detect(hm, off, world_reduce=D.REDUCE, **kw)
    assert det.xy.shape == (2, 5, 2) and det.score.shape == det.cell.shape == (2, 5)
    assert det.count.tolist() == [len(w[0]) for w in D.expected("all_above_cap5")] and int(det.count.min()) > 5
    with pytest.raises(RuntimeError, match="max_det"):
        detections_from_heatmap_fused(hm, off, [0, 1], max_det=5)


def test_layouts_give_the_same_answer():
    hm, off, _ = D.make_case("all_above")
    want = bev_detect(hm, off)
    cl = bev_detect(hm.contiguous(memory_format=torch.channels_last), off.contiguous(memory_format=torch.channels_last))
    wide = torch.zeros(2, 3, 24, 83)
    wide[:, 1:2, :, 2:82:2] = hm
    sliced = wide[:, 1:2, :, 2:82:2]
    assert not sliced.is_contiguous() and off.contiguous(memory_format=torch.channels_last).stride() != off.stride()
    sl = bev_detect(sliced, off.flip(1).flip(1))
    for got in (cl, sl):
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    D.assert_matches(cl, "all_above", hm)


def test_misuse_raises():
    hm, off, _ = D.make_case("one_frame_empty")
    with pytest.raises(RuntimeError):
        bev_detect(hm[:, 0], off)
    with pytest.raises(RuntimeError):
        bev_detect(hm, off.double())
    with pytest.raises(RuntimeError):
        bev_detect(hm.half(), off.half())
    assert not bev_detect(hm.requires_grad_(True), off).xy.requires_grad


def test_fused_rows_equal_the_loop_on_tie_free_input():
    """CPU against CPU: the same rows, exactly, where no two scores of a frame are equal."""
    g = torch.Generator().manual_seed(5)
    perm = torch.stack([torch.randperm(513, generator=g)[:12 * 20] for _ in range(3)])
    hm = ((perm - 256).float() / 32).view(3, 1, 12, 20)
    D.check_input(hm)
    assert all(len(torch.unique(f)) == f.numel() for f in hm)
    off = torch.randn(3, 2, 12, 20, generator=g) * 3
    for kw in ({}, {"indexing": "ij"}, {"top_k": 20}, {"cls_thres": 0.7, "dist_thres": 10}):
        want = detections_from_heatmap(hm, off, [3, 5, 8], **kw)
        got = detections_from_heatmap_fused(hm, off, [3, 5, 8], **kw)
        assert want.shape[0] > 10 and got.dtype == want.dtype and torch.equal(got, want), kw
    assert torch.equal(detections_from_heatmap_fused(hm, None, [3, 5, 8]), detections_from_heatmap(hm, None, [3, 5, 8]))


class _Heads(torch.nn.Module):
    """Stands in for build_model('wildtrack'): returns fixed Wildtrack-shaped head outputs, frame by frame."""

    def __init__(self, maps):
        super().__init__()
        self.maps, self.at = maps, 0
        self.anchor = torch.nn.Parameter(torch.zeros(1))

        class G:
            world_reduce, indexing = 4, "ij"
        self.geom = G

    def forward(self, imgs, M):
        out = self.maps[self.at]
        self.at += 1
        return out, (None, None, None)

    def detect(self, imgs, M, **kw):
        (hm, off), _ = self.forward(imgs, M)
        kw.setdefault("world_reduce", self.geom.world_reduce)
        return bev_detect(hm, off, **kw)


def test_test_epoch_round_trips_through_evaluate(tmp_path):
    from mvdetr_amd.test_loop import test_epoch
    rng = np.random.default_rng(3)
    H, W = 120, 360
    maps, gt_rows, batches = [], [], []
    for k in range(2):                                      # two batches of two frames, ~12 people each
        hm, off = torch.full((2, 1, H, W), -2.1875), torch.full((2, 2, H, W), 0.5)
        for b in range(2):
            frame = 5 * (2 * k + b)
            for _ in range(12):
                r, c = int(rng.integers(2, H - 2)), int(rng.integers(2, W - 2))
                hm[b, 0, r, c] = float(rng.integers(0, 200)) / 32
                hm[b, 0, r, c + 1] = -0.25                  # a weaker neighbour the NMS removes
                gt_rows.append([frame, (r + 0.5) * 4 + rng.integers(-6, 7), (c + 0.5) * 4 + rng.integers(-6, 7)])
            gt_rows.append([frame, 7, 9])                   # one person nobody detects
        D.check_input(hm)
        maps.append((hm, off))
        batches.append((torch.zeros(2, 7, 3, 8, 8), None, None, None, torch.tensor([10 * k, 10 * k + 5])))
    gt_path, res_path = tmp_path / "gt.txt", tmp_path / "res.txt"
    np.savetxt(gt_path, np.asarray(gt_rows), "%d")
    model = _Heads(maps)
    mean_loss, moda = test_epoch(model, batches, str(res_path), str(gt_path))
    assert mean_loss is None and not model.training and model.at == 2
    res = np.loadtxt(res_path)
    want = torch.cat([detections_from_heatmap(hm, off, fr, indexing="ij") for (hm, off), (*_, fr) in zip(maps, batches)])
    assert np.array_equal(res, np.loadtxt(_saved(tmp_path, want)))
    recall, precision, want_moda, modp = post_oracle.clear_mod(res, np.loadtxt(gt_path))
    assert 0 < want_moda < 100 and abs(moda - want_moda) < 1e-9
    model.at = 0
    loss, moda2 = test_epoch(model, batches, str(res_path), str(gt_path), criterion=lambda out, wg, ig: out[0][0].mean())
    assert abs(loss - float(torch.stack([m[0].mean() for m in maps]).mean())) < 1e-6 and moda2 == moda
    model.at = 0
    assert test_epoch(model, batches) == (None, 0)


def _saved(tmp_path, rows):
    path = tmp_path / "want.txt"
    np.savetxt(path, rows.numpy(), "%d")
    return path


def test_new_symbols_are_declared_and_the_abi_version_stays():
    names = ["mvdetr_detect_workspace_bytes", "mvdetr_detect_last_kernel", "mvdetr_detect_launch_count"]
    names += [f"mvdetr_{op}{host}_{t}" for op in ("detect_forward", "distance_nms") for host in ("", "_host") for t in ("f32", "f64")]
    assert set(names) <= set(_lib.SIGNATURES) and _lib.ABI_VERSION == 18
    lib = _lib.lib()
    assert lib.mvdetr_ops_abi_version() == 18
    assert lib.mvdetr_detect_workspace_bytes(1, 120, 360, 4) > 0 and lib.mvdetr_detect_workspace_bytes(1, 0, 360, 4) < 0
    assert lib.mvdetr_detect_workspace_bytes(1, 120, 360, 2) < 0
