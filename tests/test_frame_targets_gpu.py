"""The training-target kernel (csrc/frame_targets.hip) against the library's host path, torch.equal on every key: the cases of
test_frame_targets.py on the device, map shapes / segment sizes / capacities across the kernel's tile and wave edges, every
element written (the outputs' memory is NaN-filled beforehand), run-to-run identity, launch counts, no host synchronise, M and
angles from the CPU, one training step from frames, and one full-size frame.  The host path itself is held to get_gt,
affine_boxes and the oracle in test_frame_targets.py."""
import numpy as np
import pytest
import torch

import frame_targets_cases as C
from mvdetr_amd import augment, geometry
from mvdetr_amd.ops import map_targets
from mvdetr_amd.ops import targets as ops_targets
from mvdetr_amd.targets import frame_targets, get_gt, synthetic_frame_annotations

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def on_device(kw, also=()):
    """The case's tensors on the device; M and angle only when named in `also` (a CPU M / angle is uploaded by the op)."""
    return {k: v.to(DEV) if isinstance(v, torch.Tensor) and (k not in ("M", "angle") or k in also) else v for k, v in kw.items()}


def poison(kw):
    """Allocate and free NaN / all-ones filled memory of the outputs' sizes: torch.empty then hands the op these blocks, and a
    cell or slot the kernel fails to write shows up."""
    maps, top_k = len(kw["count"]), kw.get("top_k", 100)
    H, W = kw["Rshape"]
    junk = [torch.full((maps, 1, H, W), float("nan"), device=DEV), torch.full((maps, top_k), 255, dtype=torch.uint8, device=DEV),
            torch.full((maps, top_k), -1, dtype=torch.int64, device=DEV), torch.full((maps, top_k), -1, dtype=torch.int64, device=DEV),
            torch.full((maps, top_k, 2), float("nan"), device=DEV), torch.full((maps, top_k, 2), float("nan"), device=DEV)]
    del junk


def device_result(kw, also=("M", "angle")):
    dkw = on_device(kw, also)
    poison(kw)
    got = map_targets(**dkw)
    assert all(v.device == torch.device(DEV) for v in got.values())
    return {k: v.cpu() for k, v in got.items()}


def assert_equal(got, want, what):
    assert list(got) == list(want), (what, list(got), list(want))
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert torch.equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("case", C.all_cases(), ids=lambda c: c[0])
def test_cpu_cases_on_the_device(case):
    name, kw = case
    assert_equal(device_result(kw), map_targets(**kw), name)


def test_a_radius_above_the_maximum_raises_on_the_device_too():
    kw = on_device(dict(C.edge_cases())["max_radius"])
    with pytest.raises(RuntimeError, match="radius 16"):
        map_targets(**{**kw, "kernel_size": 64, "reduce": 12})


def box_segment(Rshape, maps, cap, counts, seed, reduce=4, top_k=100):
    """`maps` maps of real-valued boxes under per-map augmentation matrices (every third one rotated), counts[m % len(counts)]
    boxes in map m: compaction ranks, holes and rejected boxes in every wave the capacity reaches."""
    rng = np.random.default_rng(seed)
    H, W = Rshape
    ih, iw = H * reduce, W * reduce
    rows, Ms, angles = [], [], []
    for m in range(maps):
        n = counts[m % len(counts)]
        x1, y1 = rng.uniform(-0.2 * iw, iw, n), rng.uniform(-0.2 * ih, ih, n)
        rows.append(np.stack([x1, y1, x1 + rng.uniform(2, max(0.6 * iw, 8), n), y1 + rng.uniform(2, max(0.6 * ih, 8), n)], 1))
        angles.append(float(rng.uniform(-10, 10)) if m % 3 == 2 else 0.0)
        Ms.append(augment.affine_matrix((ih, iw), hflip=bool(m % 2), angle=angles[-1], scale=float(rng.uniform(0.7, 1.3)),
                                        tx=float(rng.uniform(-0.1, 0.1) * iw), ty=float(rng.uniform(-0.1, 0.1) * ih)))
    boxes, count = C.padded(rows, 4, cap=cap)
    keep = torch.ones(maps, dtype=torch.bool)
    if maps > 2:
        keep[1] = False
    return dict(Rshape=list(Rshape), boxes=boxes, count=count, pids=C.pids_of(count, cap), M=torch.from_numpy(np.stack(Ms)),
                angle=torch.tensor(angles, dtype=torch.float64), img_hw=(ih, iw), keep=keep, reduce=reduce, kernel_size=10, top_k=top_k)


@pytest.mark.parametrize("Rshape", [[1, 1], [5, 7], [13, 67], [64, 64], [65, 129]], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("maps", [1, 3, 14])
def test_map_shapes_across_tile_edges(Rshape, maps):
    """[64, 64] is exactly four workgroups of 1024 cells, [65, 129] ends inside the ninth, the small ones inside the first."""
    kw = box_segment(Rshape, maps, cap=40, counts=[40, 17, 0, 33], seed=maps * 100 + Rshape[1])
    want = map_targets(**kw)
    assert_equal(device_result(kw), want, (Rshape, maps))
    if Rshape[0] >= 13:
        assert want["reg_mask"].any() and not want["reg_mask"][:, :40].all()


@pytest.mark.parametrize("cap,counts", [(1, [1, 0]), (63, [63, 62, 1]), (64, [64, 63, 0]), (65, [65, 64, 63]), (100, [100, 65, 64, 63, 1])],
                         ids=lambda v: str(v) if isinstance(v, int) else None)
def test_capacities_and_counts_on_either_side_of_a_wave(cap, counts):
    """Points (slot = index) and boxes under M (slot = rank among the kept: the ranks run across the waves' ballots)."""
    rng = np.random.default_rng(cap)
    maps = len(counts) + 1
    kw = box_segment([13, 67], maps, cap, counts, seed=cap, top_k=max(cap, 37))
    want = map_targets(**kw)
    assert_equal(device_result(kw), want, ("boxes", cap))
    if cap >= 63:
        kept = want["reg_mask"][0].sum()
        assert 0 < int(kept) < counts[0]                                                              # compaction had work to do
    pts, count = C.padded([C._uniform_points(rng, counts[m % len(counts)], [13, 67], 4) for m in range(maps)], 2, cap=cap)
    pkw = dict(Rshape=[13, 67], points=pts, count=count, pids=C.pids_of(count, cap), reduce=4, kernel_size=10, top_k=max(cap, 37))
    assert_equal(device_result(pkw), map_targets(**pkw), ("points", cap))


def test_a_capacity_of_several_rounds_of_the_workgroup():
    """cap = 1024, top_k = 1024: four rounds of 256 objects, the ranks carried from round to round."""
    kw = box_segment([13, 67], 2, 1024, [1024, 700], seed=9, top_k=1024)
    want = map_targets(**kw)
    assert int(want["reg_mask"][0].sum()) > 256
    assert_equal(device_result(kw), want, "cap 1024")


def test_two_calls_are_bit_equal_and_the_launches_are_counted_and_nothing_waits_for_the_device():
    kw = box_segment([13, 67], 3, 65, [65, 64, 63], seed=2)
    dkw = on_device(kw, also=("M", "angle"))
    first = map_targets(**dkw)
    torch.cuda.synchronize()
    n0 = ops_targets.launch_count()
    second = map_targets(**dkw)
    assert ops_targets.launch_count() - n0 == 1
    assert_equal(first, second, "run to run")
    g = geometry.MINI
    ann = [a.to(DEV) for a in synthetic_frame_annotations(g, 8, seed=3, batch=2)]
    n0 = ops_targets.launch_count()
    frame_targets(g, *ann)
    assert ops_targets.launch_count() - n0 == 2
    cpu_kw = on_device(kw)                                                                           # M, angle on the CPU
    map_targets(**cpu_kw)                                                                            # (pinned staging exists now)
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this build of torch has no torch.cuda.set_sync_debug_mode")
    try:
        torch.cuda.set_sync_debug_mode("error")
    except NotImplementedError as e:                                                                 # nothing else may drop the assertion
        pytest.skip(f"this build of torch does not implement torch.cuda.set_sync_debug_mode: {e}")
    try:
        third = map_targets(**dkw)
        fourth = map_targets(**cpu_kw)
        world, imgs = frame_targets(g, *ann)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert_equal(third, first, "under sync debug")
    assert_equal(fourth, first, "M and angle from the CPU, under sync debug")
    assert imgs["reg_mask"].any() and world["reg_mask"].any()


def test_m_and_angles_from_the_cpu_equal_m_and_angles_on_the_device():
    kw = box_segment([13, 67], 14, 40, [40, 17, 0, 33], seed=77)
    want = map_targets(**kw)
    assert_equal(device_result(kw, also=()), want, "M, angle on the CPU")
    assert_equal(device_result(kw, also=("M",)), want, "M on the device, angle on the CPU")
    assert_equal(device_result(kw, also=("M", "angle")), want, "M, angle on the device")
    with pytest.raises(RuntimeError, match="lives on"):
        map_targets(**{**on_device(kw), "count": kw["count"]})                                      # mixed devices
    with pytest.raises(RuntimeError, match="lives on"):
        map_targets(**{**kw, "pids": kw["pids"].to(DEV)})


def test_frame_targets_on_the_device_with_keep_cams():
    g = geometry.MINI
    ann = synthetic_frame_annotations(g, 8, seed=3, batch=2)
    keep = torch.tensor([[1, 0, 1], [0, 1, 1]], dtype=torch.bool)
    want_world, want_imgs = frame_targets(g, *ann, keep_cams=keep)
    world, imgs = frame_targets(g, *(a.to(DEV) for a in ann), keep_cams=keep.to(DEV))
    assert_equal({k: v.cpu() for k, v in world.items()}, want_world, "world")
    assert_equal({k: v.cpu() for k, v in imgs.items()}, want_imgs, "imgs")


def _host_frame_targets(g, ann, M):
    """get_gt over affine_boxes, frame by frame and view by view, collated as a dataloader does."""
    world, views = [], []
    for b in range(ann.boxes.shape[0]):
        n = int(ann.world_count[b])
        p = ann.world_pts[b, :n].numpy()
        world.append(get_gt(g.Rworld_shape, p[:, 0], p[:, 1], v_s=ann.world_pids[b, :n].numpy(), reduce=g.world_reduce, top_k=100,
                            kernel_size=10))
        per_view = []
        for c in range(g.num_cam):
            n = int(ann.box_count[b, c])
            bx, pid = augment.affine_boxes(ann.boxes[b, c, :n].numpy(), ann.box_pids[b, c, :n].numpy(), M[b, c].numpy(), g.img_shape)
            per_view.append(get_gt(g.Rimg_shape, (bx[:, 0] + bx[:, 2]) / 2, bx[:, 3], bx[:, 2] - bx[:, 0], bx[:, 3] - bx[:, 1], v_s=pid,
                                   reduce=g.img_reduce, top_k=100, kernel_size=10))
        views.append({k: torch.stack([v[k] for v in per_view]) for k in per_view[0]})
    return ({k: torch.stack([w[k] for w in world]) for k in world[0]}, {k: torch.stack([v[k] for v in views]) for k in views[0]})


def test_train_step_frames_on_the_mini_model():
    """One step from uint8 frames and device-resident annotations; and on that step's own model outputs (a forward hook hands
    them over) the criterion returns the same (loss, terms), torch.equal, for the device-built targets as for get_gt-built
    targets copied up -- and the loss the step returned."""
    from mvdetr_amd.model import build_model
    from mvdetr_amd.train import MVDeTrCriterion, train_step_frames
    g = geometry.MINI
    model = build_model("mini", seed=0).to(DEV).train()
    crit, opt = MVDeTrCriterion(), torch.optim.SGD(model.parameters(), lr=1e-4)
    gen = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 256, (1, g.num_cam, *g.img_shape, 3), dtype=torch.uint8, generator=gen).to(DEV)
    M = torch.stack([torch.from_numpy(augment.affine_matrix(g.img_shape, hflip=c == 1, scale=(0.75, 1.25, 1.0)[c], tx=5 * c, ty=-4 * c))
                     for c in range(g.num_cam)])[None]
    ann = synthetic_frame_annotations(g, 8, seed=6)
    dev_ann = type(ann)(*(a.to(DEV) for a in ann))
    before = [p.detach().clone() for p in model.parameters()]
    seen = []
    hook = model.register_forward_hook(lambda module, args, out: seen.append(out))                   # the step's own forward
    n0 = ops_targets.launch_count()
    try:
        step_loss = train_step_frames(model, crit, opt, frames, M, dev_ann)
    finally:
        hook.remove()
    assert ops_targets.launch_count() - n0 == 2 and len(seen) == 1
    assert step_loss.device == torch.device(DEV) and bool(torch.isfinite(step_loss))
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    outputs = tuple(tuple(t.detach() for t in head) for head in seen[0])
    world, imgs = frame_targets(g, *dev_ann, M=M)
    host_world, host_imgs = _host_frame_targets(g, ann, M)
    assert imgs["reg_mask"].any() and not imgs["reg_mask"][..., :8].all()
    loss, terms = crit(outputs, world, imgs)
    host_loss, host_terms = crit(outputs, host_world, host_imgs)
    assert torch.equal(loss, step_loss)
    assert torch.equal(loss, host_loss) and list(terms) == list(host_terms) and len(terms) == 5
    for k in terms:
        assert torch.equal(terms[k], host_terms[k]), k


def test_one_frame_at_full_size():
    """Wildtrack's shapes once: [7, 90, 160] views under an augmentation M and the [1, 120, 360] world map, 40 people."""
    g = geometry.WILDTRACK
    ann = synthetic_frame_annotations(g, 40, seed=1)
    M = torch.stack([torch.from_numpy(augment.affine_matrix(g.img_shape, hflip=c % 2 == 1, angle=(0.0, 7.5, -4.0)[c % 3],
                                                            scale=0.7 + 0.1 * c, tx=30.0 * c - 90, ty=11.5 * c))
                     for c in range(g.num_cam)])[None]
    angles = torch.tensor([[(0.0, 7.5, -4.0)[c % 3] for c in range(g.num_cam)]], dtype=torch.float64)
    want_world, want_imgs = frame_targets(g, *ann, M=M, angles=angles)
    assert want_imgs["heatmap"].shape == (1, 7, 1, 90, 160) and want_world["heatmap"].shape == (1, 1, 120, 360)
    assert int(want_world["reg_mask"].sum()) == 40 and 100 < int(want_imgs["reg_mask"].sum()) < 280
    world, imgs = frame_targets(g, *(a.to(DEV) for a in ann), M=M, angles=angles)
    assert_equal({k: v.cpu() for k, v in world.items()}, want_world, "world")
    assert_equal({k: v.cpu() for k, v in imgs.items()}, want_imgs, "imgs")
