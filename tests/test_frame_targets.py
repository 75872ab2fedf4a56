"""ops.map_targets / targets.frame_targets on CPU tensors (the library's host path, csrc/host_path.cpp) against the repository's
own yardsticks -- get_gt, affine_boxes, synthetic_frame_targets -- and against tests/targets_oracle.py, the same arithmetic as
plain Python float loops.  The kernel is compared with this host path in test_frame_targets_gpu.py."""
import re

import numpy as np
import pytest
import torch

import frame_targets_cases as C
import targets_oracle as O
from mvdetr_amd import _lib, geometry, ops
from mvdetr_amd.ops import map_targets
from mvdetr_amd.ops import targets as ops_targets
from mvdetr_amd.targets import frame_targets, synthetic_frame_annotations, synthetic_frame_targets

EXACT = C.edge_cases() + C.exact_cases()


def assert_equal(got, want, what):
    assert list(got) == list(want), (what, list(got), list(want))                 # 'wh' exactly for boxes, get_gt's key order
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert torch.equal(got[k], want[k]), (what, k)


def first_difference(got, want):
    return next((k for k in want if not torch.equal(got[k], want[k])), None)


# ---- without M: get_gt is the yardstick -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", C.golden_cases(), ids=lambda c: c[0])
def test_goldens_of_the_reference(case):
    """Every get_gt case of tests/golden/loss.npz, against the reference's recorded outputs themselves and against get_gt."""
    name, kw, want = case
    got = map_targets(**kw)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (name, k)
    assert_equal(got, C.yardstick(kw), name)


@pytest.mark.parametrize("case", EXACT, ids=lambda c: c[0])
def test_equals_get_gt_bit_for_bit(case):
    """The seeded edge cases without M and the exact cases with M (every product exact in fp64): torch.equal on every key with
    get_gt(affine_boxes(...)); the oracle agrees as well."""
    name, kw = case
    got = map_targets(**kw)
    assert_equal(got, C.yardstick(kw), name)
    assert_equal(got, O.map_targets(**kw), name + " (oracle)")


def test_edge_cases_are_the_ones_they_claim():
    cases = dict(C.edge_cases())
    got = {n: map_targets(**kw) for n, kw in cases.items()}
    assert got["map_smaller_than_patch"]["heatmap"].shape == (1, 1, 3, 5) and float(got["map_smaller_than_patch"]["heatmap"].min()) > 0
    b = got["borders"]
    assert b["reg_mask"][0, :8].tolist() == [True, True, True, False, False, True, True, False]      # -0.0 inside; W reduce outside
    assert b["idx"][0, 0] == 12 * 67 + 66 and b["idx"][0, 1] == 0 and b["idx"][0, 5] == 66
    f = got["fp32_rounds_to_the_edge"]
    assert (1920 - 1e-7) / 12 < 160 and np.float32((1920 - 1e-7) / 12) == 160                      # inside in fp64, outside in fp32
    assert f["reg_mask"][0, :3].tolist() == [False, True, False]
    z = got["count_zero"]
    assert not z["reg_mask"][0].any() and float(z["heatmap"][0].max()) == 0 and int(z["reg_mask"][1].sum()) == 1
    assert cases["full_100"]["points"].shape[1] == 100 and int(cases["full_100"]["count"][0]) == 100
    assert int(got["full_100"]["reg_mask"][0, 99]) + int(got["full_100"]["reg_mask"][0, 98]) >= 1  # the last slots are in use
    assert got["top_k_37"]["idx"].shape == (2, 37)
    assert sorted(got["one_cell_patch"]["heatmap"].unique().tolist()) == [0.0, 1.0]                # a 1 x 1 patch
    assert int(3 * cases["max_radius"]["kernel_size"] / cases["max_radius"]["reduce"]) == ops_targets.max_radius()
    assert cases["fp32_inputs"]["points"].dtype == torch.float32
    d = got["dropped_between_kept"]
    for m in (1, 3):
        assert all(not v[m].any() for v in d.values())
    assert d["reg_mask"][0].any() and d["reg_mask"][2].any() and float(d["heatmap"][2].max()) == 1
    used = got["duplicate_cell"]["idx"][0][got["duplicate_cell"]["reg_mask"][0]]
    assert len(used.unique()) < len(used)


def test_a_radius_above_the_maximum_raises():
    assert ops_targets.max_radius() >= 15
    kw = dict(C.edge_cases())["max_radius"]
    with pytest.raises(RuntimeError, match="radius 16"):
        map_targets(**{**kw, "kernel_size": 64, "reduce": 12})                                       # sigma = 5.33: r = 16


# ---- with M -----------------------------------------------------------------------------------------------------------------------

def test_exact_cases_cover_every_border_every_keep_rule_and_an_image_without_survivor():
    clipped = {"left": False, "right": False, "top": False, "bottom": False}
    failed = {"big_enough": False, "mostly_there": False, "not_a_sliver": False}
    no_survivor = False
    H, W = C.IMG_HW
    for name, kw in C.exact_cases():
        for m in range(len(kw["count"])):
            mat, kept_any = kw["M"][m].tolist(), False
            for box in kw["boxes"][m, :int(kw["count"][m])].tolist():
                (x1, y1, x2, y2), kept = O.move_box(box, mat, 1.0, C.IMG_HW)
                w, h, area = x2 - x1, y2 - y1, (box[2] - box[0]) * (box[3] - box[1])
                if kept:
                    kept_any = True
                    clipped["left"] |= x1 == 0
                    clipped["top"] |= y1 == 0
                    clipped["right"] |= x2 == W - 1
                    clipped["bottom"] |= y2 == H - 1
                rules = (w > 4 and h > 4, w * h / (area + 1e-16) > 0.1, max(w / (h + 1e-16), h / (w + 1e-16)) < 10)
                for rule, ok in zip(failed, rules):
                    failed[rule] |= (not ok) and sum(rules) == 2                                     # rejected by this rule ALONE
            no_survivor |= not kept_any
    assert all(clipped.values()) and all(failed.values()) and no_survivor, (clipped, failed, no_survivor)


def test_general_matrices_follow_the_oracle_bit_for_bit_and_get_gt_to_an_ulp():
    """Seeded random_affine draws, a third of them rotated, real-valued boxes.  Host path and oracle run the same operations in the
    same order: torch.equal.  numpy's matmul in affine_boxes may sum a corner's three terms in another order, an fp64 ulp that nearly
    always vanishes in the fp32 rounding: the discrete keys must still match exactly, offset and wh to 1 fp32 ulp of the value."""
    kw, yard = C.general_case()
    assert int((kw["angle"] != 0).sum()) == 20 and int(kw["count"].sum()) > 500
    got, oracle = map_targets(**kw), O.map_targets(**kw)
    assert_equal(got, oracle, "general")
    assert 0 < int(oracle["reg_mask"].sum()) < int(kw["count"].sum())                              # some rejected, some kept
    for k in ("heatmap", "reg_mask", "idx", "pid"):
        assert torch.equal(oracle[k], yard[k]), k
    for k in ("offset", "wh"):
        a, b = oracle[k].numpy(), yard[k].numpy()
        ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
        worst = float((np.abs(a - b) / ulp).max())
        print(f"{k}: worst difference {worst} ulp, {int((a != b).sum())} of {a.size} values differ")
        assert worst <= 1.0, k


def test_teeth_the_bars_can_fail():
    """The oracle broken on purpose misses the exact comparison with get_gt: the centre divided in fp32 (instead of ONE rounding of
    the fp64 quotient) on 'real_points_reduce_12', whose points are no fp32 numbers and whose divisor is no power of two -- on the
    integer exact cases x is an fp32 number, and then fp32(x) / fp32(reduce) IS the once-rounded quotient -- and step 5 without
    the compaction on an exact case with M."""
    cases = dict(EXACT)
    kw = cases["real_points_reduce_12"]
    assert first_difference(O.map_targets(**kw), C.yardstick(kw)) is None
    assert first_difference(O.map_targets(**kw, ct_fp32_division=True), C.yardstick(kw)) is not None
    kw = cases["exact_flip0_scale0.75_shift-120_31"]
    assert first_difference(O.map_targets(**kw), C.yardstick(kw)) is None
    assert first_difference(O.map_targets(**kw, compact=False), C.yardstick(kw)) in ("reg_mask", "idx")


# ---- the frame level ------------------------------------------------------------------------------------------------------------

def test_frame_targets_of_the_synthetic_annotations_are_the_synthetic_frame_targets():
    g = geometry.MINI
    ann = synthetic_frame_annotations(g, 8, seed=3, batch=2)
    assert ann.world_pts.shape == (2, 8, 2) and ann.boxes.shape == (2, g.num_cam, 8, 4) and ann.box_count.dtype == torch.int32
    world, imgs = frame_targets(g, *ann)
    want_world, want_imgs = synthetic_frame_targets(g, 8, seed=3, batch=2)
    assert_equal(world, want_world, "world")
    assert_equal(imgs, want_imgs, "imgs")
    padded_ann = synthetic_frame_annotations(g, 8, seed=3, batch=2, cap=13)                        # padding changes nothing
    world, imgs = frame_targets(g, *padded_ann)
    assert_equal(world, want_world, "world, padded")
    assert_equal(imgs, want_imgs, "imgs, padded")


def test_keep_cams_zeroes_exactly_the_dropped_cameras_view_targets():
    g = geometry.MINI
    ann = synthetic_frame_annotations(g, 8, seed=3, batch=2)
    world, imgs = frame_targets(g, *ann)
    keep = torch.tensor([[1, 0, 1], [0, 1, 1]], dtype=torch.bool)
    world_d, imgs_d = frame_targets(g, *ann, keep_cams=keep)
    assert_equal(world_d, world, "world")
    for k, v in imgs.items():
        assert v[keep].any()
        assert torch.equal(imgs_d[k][keep], v[keep]) and not imgs_d[k][~keep].any(), k


def test_frame_targets_moves_the_boxes_of_every_view_by_its_own_matrix():
    g = geometry.MINI
    ann = synthetic_frame_annotations(g, 8, seed=4, batch=2)
    from mvdetr_amd import augment
    M = torch.stack([torch.from_numpy(augment.affine_matrix(g.img_shape, hflip=i % 2 == 1, scale=0.75 + 0.25 * (i % 3), tx=7 * i, ty=-3 * i))
                     for i in range(2 * g.num_cam)]).unflatten(0, (2, g.num_cam))
    _, imgs = frame_targets(g, *ann, M=M)
    kw = dict(Rshape=list(g.Rimg_shape), boxes=ann.boxes.flatten(0, 1), count=ann.box_count.flatten(), pids=ann.box_pids.flatten(0, 1),
              M=M.flatten(0, 1), img_hw=g.img_shape, reduce=g.img_reduce, kernel_size=10)
    assert_equal({k: v.flatten(0, 1) for k, v in imgs.items()}, O.map_targets(**kw), "views")


# ---- symbols and misuse ---------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    import os
    names = {"mvdetr_frame_targets_f64", "mvdetr_frame_targets_host_f64", "mvdetr_frame_targets_max_radius",
             "mvdetr_frame_targets_launch_count"}
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mvdetr_ops.h")).read()
    assert names <= set(re.findall(r"\b(mvdetr_[a-z0-9_]+)\s*\(", hdr)) and names <= set(_lib.SIGNATURES)
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in names)
    assert _lib.ABI_VERSION == 18 and lib.mvdetr_ops_abi_version() == 18 and "#define MVDETR_OPS_ABI_VERSION 18 " in hdr
    assert ops.map_targets is map_targets
    n0 = ops_targets.launch_count()
    map_targets(**dict(C.edge_cases())["borders"])                                                   # the host path launches nothing
    assert ops_targets.launch_count() == n0


def test_misuse_raises():
    kw = dict(C.edge_cases())["borders"]
    box_kw = C.exact_cases()[0][1]
    with pytest.raises(ValueError, match="top_k = 5"):
        map_targets(**{**kw, "top_k": 5})                                                            # cap = 8 > top_k
    with pytest.raises(RuntimeError, match="exactly one"):
        map_targets(**{**kw, "boxes": box_kw["boxes"]})
    with pytest.raises(RuntimeError, match="exactly one"):
        map_targets(**{k: v for k, v in kw.items() if k != "points"})
    with pytest.raises(RuntimeError, match="points take neither"):
        map_targets(**kw, M=torch.eye(3, dtype=torch.float64)[None], img_hw=(10, 10))
    with pytest.raises(RuntimeError, match=r"count must be torch.int32, got torch.int64"):
        map_targets(**{**kw, "count": kw["count"].long()})
    with pytest.raises(RuntimeError, match=r"count must be \[1\], got \(2,\)"):
        map_targets(**{**kw, "count": torch.zeros(2, dtype=torch.int32)})
    with pytest.raises(RuntimeError, match=r"points must be \[maps, cap, 2\], got \(1, 8\)"):
        map_targets(**{**kw, "points": kw["points"][..., 0]})
    with pytest.raises(RuntimeError, match=r"M must be float \[1, 3, 3\], got \(3, 3\)"):
        map_targets(**{**box_kw, "M": box_kw["M"][0]})
    with pytest.raises(RuntimeError, match="img_hw"):
        map_targets(**{**box_kw, "img_hw": None})
    with pytest.raises(RuntimeError, match="angle without M"):
        map_targets(**{**box_kw, "M": None, "angle": torch.zeros(1)})
    with pytest.raises(RuntimeError, match="lives on"):
        map_targets(**{**kw, "count": kw["count"].to("meta")})                                       # mixed devices
    with pytest.raises(RuntimeError, match="lives on"):
        map_targets(**{**kw, "pids": kw["pids"].to("meta")})
