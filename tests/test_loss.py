"""CPU checks of the training objective: the loss modules (their torch route) and tests/loss_oracle.py against the goldens
the reference's own modules produced, the special cases of the formulas, the criterion against the golden frame, the
header's declarations, and an overfit run of train_step on the mini model.

Bars (fp32): |x32 - ref64| <= 2 |ref32 - ref64| + 1e-6 |ref64| for a loss, the same with maxima over the elements outside
the clamp band for a gradient; ref32 / ref64 are the reference's own fp32 / fp64 results from the golden file.  fp64: 1e-12
relative."""
import os
import re

import numpy as np
import pytest
import torch

import loss_oracle
from conftest import load_golden
from mvdetr_amd import geometry
from mvdetr_amd.loss import FocalLoss, GaussianMSE, RegCELoss, RegL1Loss
from mvdetr_amd.model import build_model
from mvdetr_amd.targets import synthetic_frame_targets
from mvdetr_amd.train import TERMS, MVDeTrCriterion, train_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = load_golden("loss.npz")


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def run(fn, x, dtype):
    x = T(x, dtype).requires_grad_(True)
    loss = fn(x)
    loss.backward()
    return float(loss.detach()), x.grad.numpy().astype(np.float64)


def check64(loss, grad, loss64, grad64):
    assert abs(loss - loss64) <= 1e-12 * abs(loss64) + 1e-300
    assert np.abs(grad - grad64).max() <= 1e-12 * max(np.abs(grad64).max(), 1e-300)


def check32(loss, grad, pre, keep=None):
    l32, l64, g32, g64 = float(G[pre + "_loss32"]), float(G[pre + "_loss64"]), G[pre + "_grad32"].astype(np.float64), G[pre + "_grad64"]
    keep = np.ones(g64.shape, bool) if keep is None else keep
    assert abs(loss - l64) <= 2 * abs(l32 - l64) + 1e-6 * abs(l64), (loss, l32, l64)
    bar = 2 * np.abs(g32 - g64)[keep].max() + 1e-6 * np.abs(g64)[keep].max()
    assert np.abs(grad - g64)[keep].max() <= bar, (np.abs(grad - g64)[keep].max(), bar)


def inp(key):
    """An input array of the golden file; one that repeats an earlier input is stored once, under that one's key."""
    return G[str(G[key + "_same_as"])] if key + "_same_as" in G else G.get(key)


def focal_case(i):
    return inp(f"focal_{i}_x"), inp(f"focal_{i}_t"), inp(f"focal_{i}_m")


@pytest.mark.parametrize("i", range(int(G["focal_cases"])))
def test_focal_module_against_the_reference(i):
    """cases: plain, with a negative-term mask, no positive (num_pos == 0), both, and C = 2 with targets clipped to 1"""
    x, t, m = focal_case(i)
    mod = FocalLoss()
    tt, mm = T(t), None if m is None else T(m)
    check64(*run(lambda z: mod(z, tt, mm), x, torch.float64), float(G[f"focal_{i}_loss64"]), G[f"focal_{i}_grad64"])
    check32(*run(lambda z: mod(z, tt, mm), x, torch.float32), f"focal_{i}", ~loss_oracle.clamp_band(x))


def test_focal_goldens_hold_the_special_cases():
    x, t, m = focal_case(0)
    assert (t == 1).sum() > 0 and (np.abs(x) > loss_oracle.CLAMP_LOGIT).sum() >= 4
    g = G["focal_0_grad64"]
    assert np.all(g[np.abs(x) > loss_oracle.CLAMP_LOGIT + 1e-6] == 0)                 # zero where the sigmoid is clamped
    assert (focal_case(2)[1] == 1).sum() == 0 and float(G["focal_2_loss64"]) > 0         # num_pos == 0: -neg, not a division by 0
    # the mask multiplies the negative term only: the positives' gradients are those of the unmasked call
    pos = t == 1
    assert np.array_equal(G["focal_1_grad64"][pos], g[pos]) and float(G["focal_1_loss64"]) < float(G["focal_0_loss64"])


@pytest.mark.parametrize("i", range(int(G["l1_cases"])))
def test_reg_l1_module_against_the_reference(i):
    """cases: duplicate indices and an exact zero difference, an all-false mask, one channel"""
    x, m, ind, t = (inp(f"l1_{i}_{k}") for k in ("x", "mask", "ind", "t"))
    mod = RegL1Loss()
    fn = lambda z: mod(z, T(m), T(ind), T(t))  # noqa: E731
    check64(*run(fn, x, torch.float64), float(G[f"l1_{i}_loss64"]), G[f"l1_{i}_grad64"])
    check32(*run(fn, x, torch.float32), f"l1_{i}")


def test_reg_l1_special_cases():
    assert float(G["l1_1_loss64"]) == 0.0 and not G["l1_1_grad64"].any()                 # all-false mask
    x, m, ind, t = (inp(f"l1_0_{k}") for k in ("x", "mask", "ind", "t"))
    W = x.shape[3]
    y, xx = divmod(int(ind[0, 1]), W)
    assert ind[0, 3] == ind[0, 1] == ind[0, 7] and m[0, [1, 3, 7]].all()
    den = float(np.float32(2 * m.sum()) + np.float32(1e-4))
    signs = np.sign(x[0, :, y, xx][None] - t[0, [1, 3, 7]].astype(np.float64)).sum(0)
    assert np.allclose(G["l1_0_grad64"][0, :, y, xx], signs / den, rtol=1e-12)           # duplicates add
    # sign(0) = 0: the slot whose fp32 target equals the fp32 prediction gets no gradient in fp32
    y, xx = divmod(int(ind[0, 2]), W)
    others = [(b, k) for b in range(2) for k in range(ind.shape[1]) if m[b, k] and ind[b, k] == ind[0, 2] and (b, k) != (0, 2)]
    if not others:
        assert not G["l1_0_grad32"][0, :, y, xx].any()


def test_oracle_is_pinned_to_the_reference():
    """fp64 oracle = the reference's fp64 within 1e-12.  The fp32 oracle serves as ref32 in the device tests' bars, so beyond
    meeting the bar itself it is held to the reference's OWN fp32 results: within 1e-6 relative (about 16 fp32 ulps: the
    focal formula chains some eight rounded fp32 operations per element through two libraries' exp / log, and a sum over
    3,456 elements adds log2(n) 2^-24 = 7e-7 at most), and bit for bit for the L1 gradient, whose entries are a sum of
    signs over one fp32 divisor."""
    for i in range(int(G["focal_cases"])):
        x, t, m = focal_case(i)
        loss, grad = loss_oracle.focal(x, t, m)
        check64(float(loss), grad, float(G[f"focal_{i}_loss64"]), G[f"focal_{i}_grad64"])
        loss, grad = loss_oracle.focal(x, t, m, np.float32)
        keep = ~loss_oracle.clamp_band(x)
        check32(float(loss), grad.astype(np.float64), f"focal_{i}", keep)
        l32, g32 = float(G[f"focal_{i}_loss32"]), G[f"focal_{i}_grad32"]
        assert abs(float(loss) - l32) <= 1e-6 * abs(l32), (i, float(loss), l32)
        assert np.abs(grad - g32)[keep].max() <= 1e-6 * np.abs(g32)[keep].max(), i
    for i in range(int(G["l1_cases"])):
        x, m, ind, t = (inp(f"l1_{i}_{k}") for k in ("x", "mask", "ind", "t"))
        loss, grad = loss_oracle.reg_l1(x, m, ind, t)
        check64(float(loss), grad, float(G[f"l1_{i}_loss64"]), G[f"l1_{i}_grad64"])
        loss, grad = loss_oracle.reg_l1(x, m, ind, t, np.float32)
        check32(float(loss), grad.astype(np.float64), f"l1_{i}")
        assert abs(float(loss) - float(G[f"l1_{i}_loss32"])) <= 1e-6 * abs(float(G[f"l1_{i}_loss32"]))
        assert np.array_equal(grad, G[f"l1_{i}_grad32"])


def test_reg_ce_and_gaussian_mse_against_the_reference():
    x, m, ind, t = (G[f"ce_{k}"] for k in ("x", "mask", "ind", "t"))
    mod = RegCELoss()
    fn = lambda z: mod(z, T(m), T(ind), T(t))  # noqa: E731
    check64(*run(fn, x, torch.float64), float(G["ce_loss64"]), G["ce_grad64"])
    check32(*run(fn, x, torch.float32), "ce")
    empty = mod(T(x), torch.zeros_like(T(m)), T(ind), T(t))
    assert empty == 0 and float(G["ce_empty"]) == 0.0
    gm = GaussianMSE()
    loss, grad = run(lambda z: gm(z, T(G["gmse_t"]), T(G["gmse_k"])), G["gmse_x"], torch.float32)
    assert abs(loss - float(G["gmse_loss"])) <= 1e-6 * abs(float(G["gmse_loss"]))
    assert np.abs(grad - G["gmse_grad"]).max() <= 1e-6 * np.abs(G["gmse_grad"]).max()


def frame(dtype, device="cpu"):
    heads = {k: T(G[f"frame_{k}"], dtype).to(device).requires_grad_(True) for k in ("w_hm", "w_off", "i_hm", "i_off", "i_wh")}
    world_gt = {k[len("frame_world_"):]: T(v) for k, v in G.items() if k.startswith("frame_world_")}
    imgs_gt = {k[len("frame_imgs_"):]: T(v) for k, v in G.items() if k.startswith("frame_imgs_")}
    return ((heads["w_hm"], heads["w_off"]), (heads["i_hm"], heads["i_off"], heads["i_wh"])), world_gt, imgs_gt


def check_frame(loss, terms, dtype):
    t32, t64, tot32, tot64 = G["frame_terms32"], G["frame_terms64"], float(G["frame_total32"]), float(G["frame_total64"])
    got = [float(terms[k]) for k in TERMS]
    if dtype == torch.float64:
        assert np.abs(np.array(got) - t64).max() <= 1e-12 * np.abs(t64).max() and abs(float(loss.detach()) - tot64) <= 1e-12 * tot64
    else:
        for a, r32, r64 in zip(got + [float(loss.detach())], list(t32) + [tot32], list(t64) + [tot64]):
            assert abs(a - r64) <= 2 * abs(r32 - r64) + 1e-6 * abs(r64), (a, r32, r64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_criterion_terms_and_total_against_the_golden_frame(dtype):
    outputs, world_gt, imgs_gt = frame(dtype)
    loss, terms = MVDeTrCriterion(alpha=1.0)(outputs, world_gt, imgs_gt)
    assert sorted(terms) == sorted(TERMS) and all(v.dim() == 0 and not v.requires_grad for v in terms.values())
    check_frame(loss, terms, dtype)
    loss.backward()
    assert all(h.grad is not None and h.grad.abs().sum() > 0 for pair in outputs for h in pair)


def test_criterion_use_mse():
    outputs, world_gt, imgs_gt = frame(torch.float64)
    only_heatmaps = lambda d: {"heatmap": d["heatmap"]}  # noqa: E731  (the MSE objective reads nothing else)
    loss, terms = MVDeTrCriterion(alpha=1.0, use_mse=True)(outputs, only_heatmaps(world_gt), only_heatmaps(imgs_gt))
    assert terms == {} and abs(float(loss.detach()) - float(G["frame_mse64"])) <= 1e-12 * float(G["frame_mse64"])
    loss.backward()
    (w_hm, w_off), (i_hm, i_off, i_wh) = outputs
    assert w_hm.grad is not None and i_hm.grad is not None and w_off.grad is None and i_wh.grad is None
    outputs, world_gt, imgs_gt = frame(torch.float32)
    loss, _ = MVDeTrCriterion(alpha=1.0, use_mse=True)(outputs, world_gt, imgs_gt)
    assert abs(float(loss.detach()) - float(G["frame_mse64"])) <= 2 * abs(float(G["frame_mse32"]) - float(G["frame_mse64"])) + 1e-6 * float(G["frame_mse64"])


def overfit(device, channels_last):
    g = geometry.MINI
    model = build_model("mini", seed=0, channels_last=channels_last, dropout=0.0).to(device).train()
    world_gt, imgs_gt = synthetic_frame_targets(g, 8, seed=0)
    imgs = torch.randn(1, g.num_cam, 3, *g.input_img_shape, generator=torch.Generator().manual_seed(1)).to(device)
    M = torch.eye(3).repeat(1, g.num_cam, 1, 1)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    crit = MVDeTrCriterion()
    losses = [train_step(model, crit, opt, imgs, M, world_gt, imgs_gt) for _ in range(12)]
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 for v in losses)
    return [float(v) for v in losses]


def test_train_step_overfits_one_synthetic_frame():
    losses = overfit("cpu", channels_last=False)
    print("overfit losses:", " ".join(f"{v:.3f}" for v in losses))
    assert losses[-1] < 0.5 * losses[0], losses


def test_header_declares_every_loss_export():
    hdr = open(os.path.join(ROOT, "include", "mvdetr_ops.h")).read()
    declared = set(re.findall(r"\b(mvdetr_[a-z0-9_]+)\s*\(", hdr))
    want = {f"mvdetr_{op}_{d}_{t}" for op in ("focal_loss", "reg_l1_loss") for d in ("forward", "backward") for t in ("f32", "f64")}
    want |= {"mvdetr_loss_last_kernel", "mvdetr_loss_launch_count", "mvdetr_focal_loss_workspace_bytes"}
    assert want <= declared, want - declared
    from mvdetr_amd import _lib
    assert want <= set(_lib.SIGNATURES)
    assert re.search(r"#define MVDETR_OPS_ABI_VERSION 18\b", hdr) and _lib.ABI_VERSION == 18


def test_switch_and_route_predicates():
    from mvdetr_amd import loss
    assert loss.loss_fusion_enabled() == (os.environ.get("MVDETR_LOSS_FUSION", "1") != "0")
    assert not loss.fused_loss_available(torch.zeros(1, 1, 4, 4))                     # CPU tensors take the composition
    prev = loss.set_loss_fusion(False)
    try:
        assert not loss.loss_fusion_enabled()
    finally:
        loss.set_loss_fusion(prev)
    with pytest.raises(RuntimeError):
        loss.focal_loss_segments([torch.zeros(1, 1, 4, 4)], [torch.zeros(1, 1, 4, 4)])  # no quiet fall-back from the HIP entry
    assert isinstance(loss.last_kernel(), str) and loss.launch_count() >= 0
