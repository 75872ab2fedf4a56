"""get_gt against the goldens the reference's own get_gt produced (tests/golden/make_golden_loss.py), bit for bit."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from mvdetr_amd import geometry
from mvdetr_amd.targets import get_gt, synthetic_frame_targets

G = load_golden("loss.npz")


def _case(i):
    kw = {k[len(f"gt_{i}_in_"):]: v for k, v in G.items() if k.startswith(f"gt_{i}_in_")}
    for k in ("reduce", "top_k", "kernel_size"):
        if k in kw:
            kw[k] = int(kw[k])
    kw["Rshape"] = [int(v) for v in kw["Rshape"]]
    want = {k[len(f"gt_{i}_out_"):]: v for k, v in G.items() if k.startswith(f"gt_{i}_out_")}
    return kw, want


@pytest.mark.parametrize("i", range(int(G["gt_cases"])))
def test_get_gt_equals_the_reference_bit_for_bit(i):
    kw, want = _case(i)
    got = get_gt(**kw)
    assert sorted(got) == sorted(want)                          # 'wh' exactly when sizes are given
    for k, v in want.items():
        assert isinstance(got[k], torch.Tensor)
        assert got[k].numpy().dtype == v.dtype, (k, got[k].dtype, v.dtype)
        assert got[k].shape == v.shape
        assert np.array_equal(got[k].numpy(), v), k


def test_goldens_cover_the_cases_they_claim():
    seen_dup = seen_hole = seen_wh = seen_nowh = False
    for i in range(int(G["gt_cases"])):
        _, want = _case(i)
        m, idx = want["reg_mask"], want["idx"]
        used = idx[m]
        seen_dup |= len(np.unique(used)) < len(used)
        n_obj = len(G[f"gt_{i}_in_x_s"])
        seen_hole |= bool((~m[:n_obj]).any() and m[:n_obj].any() and np.flatnonzero(m).max() > np.flatnonzero(~m[:n_obj]).min())
        seen_wh |= "wh" in want
        seen_nowh |= "wh" not in want
    assert seen_dup and seen_hole and seen_wh and seen_nowh


def test_more_than_top_k_objects_inside_raises_value_error():
    xs = np.linspace(1, 50, 7)
    with pytest.raises(ValueError):
        get_gt([10, 14], xs, np.full(7, 8.0), v_s=np.arange(7), top_k=6)
    # objects beyond top_k that fall outside the map take no slot
    xs[6] = 500.0
    assert int(get_gt([10, 14], xs, np.full(7, 8.0), v_s=np.arange(7), top_k=6)["reg_mask"].sum()) == 6


def test_synthetic_frame_targets_are_batched_like_a_dataloader_and_seeded():
    g = geometry.MINI
    w, im = synthetic_frame_targets(g, 8, seed=3, batch=2)
    assert w["heatmap"].shape == (2, 1, *g.Rworld_shape) and im["heatmap"].shape == (2, g.num_cam, 1, *g.Rimg_shape)
    assert w["idx"].shape == (2, 100) and im["wh"].shape == (2, g.num_cam, 100, 2) and "wh" not in w
    assert w["reg_mask"].dtype == torch.bool and w["idx"].dtype == torch.int64 and w["heatmap"].dtype == torch.float32
    assert int(w["reg_mask"].sum()) == 16 and 0 < int(im["reg_mask"].sum()) <= 2 * g.num_cam * 8
    w2, im2 = synthetic_frame_targets(g, 8, seed=3, batch=2)
    assert all(torch.equal(w[k], w2[k]) for k in w) and all(torch.equal(im[k], im2[k]) for k in im)
    assert float(w["heatmap"].max()) == 1.0
