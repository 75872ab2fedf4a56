"""The HIP detection losses (csrc/detection_loss.hip) on the device: parity with the fp64 oracle at the Wildtrack and
MultiviewX head shapes in both layouts, multi-segment launches against single ones, gradcheck, bit-reproducibility, no
host synchronise, launch counts and kernel names, the switch-off route in a child process, and the overfit run.

Bars: |hip32 - ref64| <= 2 |ref32 - ref64| + 1e-6 |ref64| for a loss; for a gradient the same with maxima taken over the
elements outside the clamp band (logit within 2e-3 of +-9.21024; their share is asserted <= 0.1 %).  ref64 / ref32 are
tests/loss_oracle.py in fp64 / fp32; tests/test_loss.py pins them to the reference's own fp64 results within 1e-12 and to
its own fp32 results within 1e-6 (the L1 gradient bit for bit), so the bars stay anchored to the reference."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import loss_oracle  # noqa: E402
from mvdetr_amd import geometry, loss  # noqa: E402
from mvdetr_amd.loss import FocalLoss, RegL1Loss, focal_loss_segments, reg_l1_loss_segments  # noqa: E402
from mvdetr_amd.model import build_model  # noqa: E402
from mvdetr_amd.targets import get_gt, synthetic_frame_targets  # noqa: E402
from mvdetr_amd.train import TERMS, MVDeTrCriterion, train_step  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PEOPLE, K = 40, 100

# (world map, image map, cameras)
SCENES = {"wildtrack": ((120, 360), (90, 160), 7), "multiviewx": ((160, 250), (90, 160), 6)}


def heatmaps(shape, reduce, rng):
    B, C, H, W = shape
    maps = [get_gt([H, W], rng.uniform(0, W * reduce, PEOPLE), rng.uniform(0, H * reduce, PEOPLE), v_s=np.arange(PEOPLE),
                   reduce=reduce, kernel_size=10)["heatmap"][0] for _ in range(B * C)]
    return torch.stack(maps).view(B, C, H, W)


def focal_inputs(shape, reduce, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 3 - 2.19                       # ~1 % of the elements sit in the clamped range
    return x, heatmaps(shape, reduce, np.random.default_rng(seed))


def l1_inputs(shape, seed):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    ind = torch.randint(0, H * W, (B, K), generator=g)
    mask = torch.zeros(B, K, dtype=torch.bool)
    for b in range(B):
        mask[b, torch.randperm(K, generator=g)[:PEOPLE]] = True
        on = mask[b].nonzero().flatten()
        ind[b, on[5]] = ind[b, on[2]]                                   # two and three people in one cell
        ind[b, on[9]] = ind[b, on[2]]
        ind[b, on[20]] = ind[b, on[19]]
    return x, mask, ind, torch.rand(B, K, C, generator=g) * 2 - 1


def layout(x, channels_last):
    return x.contiguous(memory_format=torch.channels_last) if channels_last else x.contiguous()


def loss_bar(got, r32, r64):
    return abs(got - r64), 2 * abs(r32 - r64) + 1e-6 * abs(r64)


def grad_bar(got, g32, g64, keep=None):
    keep = np.ones(g64.shape, bool) if keep is None else keep
    return np.abs(got - g64)[keep].max(), 2 * np.abs(g32.astype(np.float64) - g64)[keep].max() + 1e-6 * np.abs(g64)[keep].max()


def check(name, err_bar):
    err, bar = err_bar
    print(f"{name}: err {err:.3e} bar {bar:.3e}")
    assert err <= bar, (name, err, bar)


def scene_segments(scene, batch, seed):
    (H, W), (h, w), N = SCENES[scene]
    fshapes = [((batch, 1, H, W), 4), ((batch * N, 1, h, w), 12)]
    lshapes = [(batch, 2, H, W), (batch * N, 2, h, w), (batch * N, 2, h, w)]
    focal = [focal_inputs(s, r, seed + i) for i, (s, r) in enumerate(fshapes)]
    l1 = [l1_inputs(s, seed + 10 + i) for i, s in enumerate(lshapes)]
    return focal, l1


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("scene,batch", [("wildtrack", 1), ("wildtrack", 2), ("multiviewx", 1)])
def test_parity_with_the_fp64_oracle_and_multi_segment_equals_single(scene, batch, channels_last):
    focal, l1 = scene_segments(scene, batch, seed=100 * batch + len(scene))
    weights_f, weights_l = (1.0, 0.25), (1.0, 0.25, 0.025)

    # ---- focal: both heat maps in one launch ----
    xs = [layout(x, channels_last).to(DEV).requires_grad_(True) for x, _ in focal]
    ts = [t.to(DEV) for _, t in focal]
    out = focal_loss_segments(xs, ts, weights=weights_f)
    assert loss.last_kernel() == "focal_loss_fwd" and out.shape == (3,) and out.dtype == torch.float32
    out[:2].sum().backward()
    assert loss.last_kernel() == "focal_loss_bwd"
    ref_total = 0.0
    for s, (x, t) in enumerate(focal):
        l64, g64 = loss_oracle.focal(x.numpy(), t.numpy())
        l32, g32 = loss_oracle.focal(x.numpy(), t.numpy(), dtype=np.float32)
        band = loss_oracle.clamp_band(x.numpy())
        assert band.mean() <= 1e-3
        clamped = np.abs(x.numpy()) > loss_oracle.CLAMP_LOGIT
        assert 0.002 < clamped.mean() < 0.05
        assert xs[s].grad.stride() == xs[s].stride()                                  # the gradient has the input's layout
        got = xs[s].grad.cpu().numpy().astype(np.float64)
        check(f"focal[{s}] loss", loss_bar(float(out[s].detach()), float(l32), float(l64)))
        check(f"focal[{s}] grad", grad_bar(got, g32, g64, ~band))
        assert not got[clamped & ~band].any()                                         # zero where the sigmoid is clamped
        ref_total += weights_f[s] * float(l64)
        # the same segment launched alone: the same bits
        x1 = xs[s].detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
        single = FocalLoss()(x1, ts[s])
        single.backward()
        assert single.dim() == 0 and torch.equal(single, out[s].detach()) and torch.equal(x1.grad, xs[s].grad)
    assert abs(float(out[2].detach()) - ref_total) <= 2e-6 * abs(ref_total)

    # ---- masked L1: world offset, image offset, image wh in one launch ----
    xs = [layout(x, channels_last).to(DEV).requires_grad_(True) for x, _, _, _ in l1]
    side = [[a[i].to(DEV) for a in l1] for i in (1, 2, 3)]
    out = reg_l1_loss_segments(xs, *side, weights=weights_l)
    assert loss.last_kernel() == "reg_l1_loss_fwd" and out.shape == (4,)
    out[:3].sum().backward()
    assert loss.last_kernel() == "reg_l1_loss_bwd"
    ref_total = 0.0
    for s, (x, m, ind, t) in enumerate(l1):
        l64, g64 = loss_oracle.reg_l1(x.numpy(), m.numpy(), ind.numpy(), t.numpy())
        l32, g32 = loss_oracle.reg_l1(x.numpy(), m.numpy(), ind.numpy(), t.numpy(), dtype=np.float32)
        assert xs[s].grad.stride() == xs[s].stride()
        got = xs[s].grad.cpu().numpy().astype(np.float64)
        check(f"l1[{s}] loss", loss_bar(float(out[s].detach()), float(l32), float(l64)))
        check(f"l1[{s}] grad", grad_bar(got, g32, g64))
        assert np.array_equal(got != 0, g64 != 0)                                     # the rest of the map is zero-filled
        ref_total += weights_l[s] * float(l64)
        x1 = xs[s].detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
        single = RegL1Loss()(x1, side[0][s], side[1][s], side[2][s])
        single.backward()
        assert torch.equal(single, out[s].detach()) and torch.equal(x1.grad, xs[s].grad)
    assert abs(float(out[3].detach()) - ref_total) <= 2e-6 * abs(ref_total)


def test_special_cases_on_the_device():
    x, t = focal_inputs((2, 1, 24, 72), 4, 5)
    xd = x.to(DEV).requires_grad_(True)
    # no positive: -neg, resolved on the device; a mask on the negative term; a two-channel map in channel-last memory
    nopos = t.clamp(max=0.98)
    mask = (torch.rand(t.shape, generator=torch.Generator().manual_seed(1)) < 0.7).float()
    for tt, mm in ((nopos, None), (t, mask), (nopos, mask)):
        l64, g64 = loss_oracle.focal(x.numpy(), tt.numpy(), None if mm is None else mm.numpy())
        l32, g32 = loss_oracle.focal(x.numpy(), tt.numpy(), None if mm is None else mm.numpy(), dtype=np.float32)
        xd.grad = None
        out = FocalLoss()(xd, tt.to(DEV), None if mm is None else mm.to(DEV))
        out.backward()
        check("focal special loss", loss_bar(float(out.detach()), float(l32), float(l64)))
        check("focal special grad", grad_bar(xd.grad.cpu().numpy().astype(np.float64), g32, g64, ~loss_oracle.clamp_band(x.numpy())))
    x2, t2 = focal_inputs((3, 2, 10, 13), 4, 6)                                       # odd sizes: the strided scalar path
    for cl in (False, True):
        xd = layout(x2, cl).to(DEV).requires_grad_(True)
        out = FocalLoss()(xd, t2.to(DEV))
        out.backward()
        l64, g64 = loss_oracle.focal(x2.numpy(), t2.numpy())
        l32, g32 = loss_oracle.focal(x2.numpy(), t2.numpy(), dtype=np.float32)
        check("focal strided loss", loss_bar(float(out.detach()), float(l32), float(l64)))
        check("focal strided grad", grad_bar(xd.grad.cpu().numpy().astype(np.float64), g32, g64, ~loss_oracle.clamp_band(x2.numpy())))
        assert xd.grad.stride() == xd.stride()
    # all-false L1 mask: 0 and a zero gradient; indices outside the map are never read and contribute nothing
    x, m, ind, tg = l1_inputs((2, 2, 10, 13), 7)
    xd = x.to(DEV).requires_grad_(True)
    out = RegL1Loss()(xd, torch.zeros_like(m).to(DEV), ind.to(DEV), tg.to(DEV))
    out.backward()
    assert float(out) == 0.0 and not xd.grad.any()
    bad = ind.clone()
    on = m[0].nonzero().flatten()
    bad[0, on[0]], bad[0, on[1]] = 10 * 13, -1
    keep = m.clone()
    keep[0, on[0]] = keep[0, on[1]] = False
    xd.grad = None
    out = RegL1Loss()(xd, m.to(DEV), bad.to(DEV), tg.to(DEV))
    out.backward()
    l64, g64 = loss_oracle.reg_l1(x.numpy(), keep.numpy(), ind.numpy(), tg.numpy())
    den_all, den_keep = 2 * int(m.sum()) + 1e-4, 2 * int(keep.sum()) + 1e-4          # the mask sum still counts them
    assert abs(float(out) - float(l64) * den_keep / den_all) <= 2e-6 * float(l64)
    assert np.abs(xd.grad.cpu().numpy() - g64 * den_keep / den_all).max() <= 2e-6 * np.abs(g64).max()


@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
def test_gradcheck_fp64(channels_last):
    g = torch.Generator().manual_seed(3)
    shapes = [(2, 1, 6, 8), (3, 2, 5, 4)]
    xs = [layout((torch.randn(s, generator=g, dtype=torch.float64) * 2).clamp(-6, 6), channels_last).to(DEV).requires_grad_(True)
          for s in shapes]                                                             # well inside the clamp bounds
    ts = [heatmaps(s, 4, np.random.default_rng(4 + i)).double().to(DEV) for i, s in enumerate(shapes)]
    assert all((t == 1).any() for t in ts)
    mask = (torch.rand(shapes[0], generator=g) < 0.6).double().to(DEV)
    assert torch.autograd.gradcheck(lambda a, b: focal_loss_segments([a, b], ts, [mask, None], weights=(1.0, 0.3)), xs,
                                    eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)
    ins = [l1_inputs(s, 8 + i) for i, s in enumerate([(2, 2, 6, 8), (3, 1, 5, 4)])]
    xs = [layout(a[0].double(), channels_last).to(DEV).requires_grad_(True) for a in ins]
    side = [[a[i].to(DEV) for a in ins] for i in (1, 2, 3)]
    side[2] = [t.double() for t in side[2]]
    assert torch.autograd.gradcheck(lambda a, b: reg_l1_loss_segments([a, b], *side, weights=(1.0, 0.3)), xs,
                                    eps=1e-6, atol=1e-7, rtol=1e-6, nondet_tol=0.0)


def device_frame(scene="wildtrack", batch=1, channels_last=True, seed=9):
    focal, l1 = scene_segments(scene, batch, seed)
    N = SCENES[scene][2]
    heads = [layout(a[0], channels_last).to(DEV).requires_grad_(True) for a in (focal[0], l1[0], focal[1], l1[1], l1[2])]
    outputs = ((heads[0], heads[1]), (heads[2], heads[3], heads[4]))
    world_gt = {"heatmap": focal[0][1], "reg_mask": l1[0][1], "idx": l1[0][2], "offset": l1[0][3]}
    unflat = lambda t: t.view(batch, N, *t.shape[1:])  # noqa: E731
    imgs_gt = {"heatmap": unflat(focal[1][1]), "reg_mask": unflat(l1[1][1]), "idx": unflat(l1[1][2]), "offset": unflat(l1[1][3]),
               "wh": unflat(l1[2][3])}
    to_dev = lambda d: {k: v.to(DEV) for k, v in d.items()}  # noqa: E731
    return heads, outputs, to_dev(world_gt), to_dev(imgs_gt)


def test_three_runs_are_bit_identical():
    heads, outputs, world_gt, imgs_gt = device_frame(batch=2)
    crit = MVDeTrCriterion()
    runs = []
    for _ in range(3):
        for h in heads:
            h.grad = None
        total, terms = crit(outputs, world_gt, imgs_gt)
        total.backward()
        runs.append([total.detach().clone()] + [terms[k].clone() for k in TERMS] + [h.grad.clone() for h in heads])
    assert (imgs_gt["idx"][0, 0][imgs_gt["reg_mask"][0, 0]].unique().numel() < PEOPLE)  # duplicate indices are in
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], other))


def test_criterion_launch_counts_and_kernel_names():
    heads, outputs, world_gt, imgs_gt = device_frame()
    crit = MVDeTrCriterion()
    n0 = loss.launch_count()
    total, terms = crit(outputs, world_gt, imgs_gt)
    n1 = loss.launch_count()
    assert loss.last_kernel() == "reg_l1_loss_fwd"
    total.backward()
    n2 = loss.launch_count()
    assert loss.last_kernel() in ("focal_loss_bwd", "reg_l1_loss_bwd")
    assert 1 <= n1 - n0 <= 2 and 1 <= n2 - n1 <= 2, (n0, n1, n2)
    assert total.dim() == 0 and total.is_cuda and all(v.dim() == 0 and v.is_cuda for v in terms.values())
    N = 7
    want = terms["w_hm"] + terms["w_off"] + (terms["img_hm"] + terms["img_off"] + 0.1 * terms["img_wh"]) / N
    assert abs(float(total) - float(want)) <= 2e-6 * float(want)


def test_criterion_does_not_synchronise():
    heads, outputs, world_gt, imgs_gt = device_frame()
    crit = MVDeTrCriterion()
    crit(outputs, world_gt, imgs_gt)[0].backward()                                     # library load, ticket buffer
    torch.cuda.synchronize()
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this build of torch has no torch.cuda.set_sync_debug_mode")
    try:
        torch.cuda.set_sync_debug_mode("error")
    except NotImplementedError as e:                                                   # nothing else may drop the assertion
        pytest.skip(f"this build of torch does not implement torch.cuda.set_sync_debug_mode: {e}")
    try:
        total, _ = crit(outputs, world_gt, imgs_gt)
        total.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert float(total) > 0


def golden_frame_run(out_path=None):
    """The criterion on the golden mini-sized frame on the device -> terms, total, head gradients, fused launches."""
    from conftest import load_golden
    G = load_golden("loss.npz")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    heads = {k: T(G[f"frame_{k}"]).float().to(DEV).requires_grad_(True) for k in ("w_hm", "w_off", "i_hm", "i_off", "i_wh")}
    world_gt = {k[len("frame_world_"):]: T(v) for k, v in G.items() if k.startswith("frame_world_")}
    imgs_gt = {k[len("frame_imgs_"):]: T(v) for k, v in G.items() if k.startswith("frame_imgs_")}
    n0 = loss.launch_count()
    total, terms = MVDeTrCriterion()(((heads["w_hm"], heads["w_off"]), (heads["i_hm"], heads["i_off"], heads["i_wh"])), world_gt, imgs_gt)
    total.backward()
    res = {"total": float(total), "terms": [float(terms[k]) for k in TERMS], "launches": loss.launch_count() - n0,
           "grads": {k: v.grad.cpu() for k, v in heads.items()}}
    if out_path:
        torch.save(res, out_path)
    return res, G


def test_switch_off_route_takes_the_composition_and_agrees():
    fused, G = golden_frame_run()
    assert fused["launches"] == 4
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "off.pt")
        subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, MVDETR_LOSS_FUSION="0"), check=True,
                       timeout=300)
        off = torch.load(out)
    assert off["launches"] == 0
    r32, r64 = list(G["frame_terms32"]) + [float(G["frame_total32"])], list(G["frame_terms64"]) + [float(G["frame_total64"])]
    N = 3
    x = {k: G[f"frame_{k}"].astype(np.float32) for k in fused["grads"]}
    tg = lambda k: G[f"frame_imgs_{k}"].reshape(N, *G[f"frame_imgs_{k}"].shape[2:])  # noqa: E731
    ref = {}
    for dt in (np.float64, np.float32):
        ref[dt] = {"w_hm": loss_oracle.focal(x["w_hm"], G["frame_world_heatmap"], dtype=dt)[1],
                   "i_hm": loss_oracle.focal(x["i_hm"], tg("heatmap"), dtype=dt)[1] / N,
                   "w_off": loss_oracle.reg_l1(x["w_off"], G["frame_world_reg_mask"], G["frame_world_idx"], G["frame_world_offset"], dt)[1],
                   "i_off": loss_oracle.reg_l1(x["i_off"], tg("reg_mask"), tg("idx"), tg("offset"), dt)[1] / N,
                   "i_wh": loss_oracle.reg_l1(x["i_wh"], tg("reg_mask"), tg("idx"), tg("wh"), dt)[1] * 0.1 / N}
    for name, res in (("fused", fused), ("composition", off)):
        for i, got in enumerate(res["terms"] + [res["total"]]):
            check(f"{name} term {i}", loss_bar(got, float(r32[i]), float(r64[i])))
        for k, g in res["grads"].items():
            keep = ~loss_oracle.clamp_band(x[k]) if k.endswith("hm") else None
            check(f"{name} grad {k}", grad_bar(g.numpy().astype(np.float64), ref[np.float32][k], ref[np.float64][k], keep))


def test_train_step_overfits_one_synthetic_frame_on_the_device():
    g = geometry.MINI
    model = build_model("mini", seed=0, channels_last=True, dropout=0.0).to(DEV).train()
    world_gt, imgs_gt = synthetic_frame_targets(g, 8, seed=0)
    imgs = torch.randn(1, g.num_cam, 3, *g.input_img_shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    M = torch.eye(3).repeat(1, g.num_cam, 1, 1)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    crit = MVDeTrCriterion()
    n0 = loss.launch_count()
    losses = [train_step(model, crit, opt, imgs, M, world_gt, imgs_gt) for _ in range(12)]
    assert loss.launch_count() - n0 == 12 * 4 and all(v.is_cuda and v.dim() == 0 for v in losses)
    losses = [float(v) for v in losses]
    print("overfit losses:", " ".join(f"{v:.3f}" for v in losses))
    assert losses[-1] < 0.5 * losses[0], losses


if __name__ == "__main__":
    golden_frame_run(sys.argv[1])
