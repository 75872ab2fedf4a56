"""Times the training objective on the GPU: the HIP losses (csrc/detection_loss.hip, two launches forward and two backward)
against the torch composition of the same formulas (the loss switch off), alternated repetition by repetition in one process:

  objective   MVDeTrCriterion forward + backward on fixed seeded head outputs at the Wildtrack and MultiviewX head shapes
              (channel-last, as the model emits them), targets resident on the device;
  step        one whole Wildtrack training step: train_step with Adam, fp32, deform_trans, the switch on and off.

    python tools/train_step_bench.py [--reps N] [--skip-step]
    python tools/train_step_bench.py --winograd-train [--families shipped|all] [--out profiles/trunk_winograd_train_ab.txt]

--winograd-train times the same whole step with the trunk's Winograd training convolutions on and off
(set_trunk_winograd_training), alternated in one process, and counts the Winograd launches of a step on either side: with
the switch off there are none, so that side runs the launches of the code without the route.  ``--families all`` switches every
3x3 convolution the route can take on with both pieces (a measurement of the route as a whole; the shipped table is what
tools/conv_bench.py --backward filled).

Two clocks per repetition: device-event time between the first and the last enqueued kernel, and host wall time from the
call to the end of a synchronise behind it.  A host synchronise in the middle of the composition costs queue idle time that
only the wall clock sees in full.  Every figure is the median of N (>= 20) after warm-up with (min .. max) beside it.  Prints
one JSON line per row and a table."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mvdetr_amd import geometry, loss  # noqa: E402
from mvdetr_amd.model import build_model  # noqa: E402
from mvdetr_amd.targets import synthetic_frame_targets  # noqa: E402
from mvdetr_amd.train import MVDeTrCriterion, train_step  # noqa: E402

DEV = "cuda:0"
PEOPLE = 40


def alternated(fns, reps, warmup=3):
    """{name: {"device": (median, min, max), "wall": (...)}} in us; the functions take turns."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    times = {n: {"device": [], "wall": []} for n in fns}
    for _ in range(reps):
        for n, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[n]["wall"].append((time.perf_counter() - t0) * 1e6)
            times[n]["device"].append(a.elapsed_time(b) * 1e3)
    stat = lambda t: (sorted(t)[len(t) // 2], min(t), max(t))  # noqa: E731
    return {n: {k: stat(v) for k, v in d.items()} for n, d in times.items()}


def with_switch(on, fn):
    def run():
        prev = loss.set_loss_fusion(on)
        try:
            return fn()
        finally:
            loss.set_loss_fusion(prev)
    return run


def emit(rows, what, size, res, extra=None):
    for clock in ("device", "wall"):
        hip = res["hip"][clock][0]
        for impl, r in res.items():
            med, lo, hi = r[clock]
            row = {"what": what, "size": size, "clock": clock, "impl": impl, "median_us": round(med, 1), "min_us": round(lo, 1),
                   "max_us": round(hi, 1), "ratio_to_hip": round(med / hip, 2)}
            row.update(extra or {})
            print(json.dumps(row), flush=True)
            rows.append(row)


def bench_objective(name, reps, rows):
    geom = geometry.GEOMETRIES[name]
    N, (H, W), (h, w) = geom.num_cam, geom.Rworld_shape, geom.Rimg_shape
    g = torch.Generator().manual_seed(0)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last).to(DEV).requires_grad_(True)  # noqa: E731
    heads = [cl(torch.randn(1, 1, H, W, generator=g) * 3 - 2.19), cl(torch.randn(1, 2, H, W, generator=g)),
             cl(torch.randn(N, 1, h, w, generator=g) * 3 - 2.19), cl(torch.randn(N, 2, h, w, generator=g)),
             cl(torch.randn(N, 2, h, w, generator=g) * 3 + 4)]
    outputs = ((heads[0], heads[1]), (heads[2], heads[3], heads[4]))
    world_gt, imgs_gt = synthetic_frame_targets(geom, PEOPLE, seed=0)
    world_gt, imgs_gt = ({k: v.to(DEV) for k, v in d.items()} for d in (world_gt, imgs_gt))
    crit = MVDeTrCriterion()

    def objective():
        total, _ = crit(outputs, world_gt, imgs_gt)
        torch.autograd.grad(total, heads)
        return total

    on, off = with_switch(True, objective), with_switch(False, objective)
    n0 = loss.launch_count()
    a, b = float(on().detach()), float(off().detach())
    extra = {"hip_launches": loss.launch_count() - n0, "loss_hip": a, "loss_composition": b}
    emit(rows, "objective fwd+bwd", name, alternated({"hip": on, "torch_composition": off}, reps), extra)


def bench_step(reps, rows):
    geom = geometry.WILDTRACK
    model = build_model("wildtrack", seed=0, world_feat_arch="deform_trans", channels_last=True).to(DEV).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    world_gt, imgs_gt = synthetic_frame_targets(geom, PEOPLE, seed=0)
    world_gt, imgs_gt = ({k: v.to(DEV) for k, v in d.items()} for d in (world_gt, imgs_gt))
    imgs = torch.randn(1, geom.num_cam, 3, *geom.input_img_shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    M = torch.eye(3).repeat(1, geom.num_cam, 1, 1)
    crit = MVDeTrCriterion()
    step = lambda: train_step(model, crit, opt, imgs, M, world_gt, imgs_gt)  # noqa: E731
    res = alternated({"hip": with_switch(True, step), "torch_composition": with_switch(False, step)}, reps, warmup=2)
    emit(rows, "train step (Adam, fp32, deform_trans)", "wildtrack", res)


def bench_winograd_train(reps, families, out):
    """The whole Wildtrack step with the Winograd training route on against off, alternated; a table to ``out``."""
    from torch import nn
    from mvdetr_amd.ops import conv_winograd as cw
    geom = geometry.WILDTRACK
    model = build_model("wildtrack", seed=0, world_feat_arch="deform_trans", channels_last=True).to(DEV).train()
    if families == "all":
        for m in model.modules():
            if (type(m) is nn.Conv2d and m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == m.dilation and m.bias is None
                    and m.in_channels % 64 == 0 and m.out_channels % 64 == 0 and m.dilation[0] in cw.DILATIONS):
                cw.TRAIN_FAMILIES.setdefault((m.in_channels, m.out_channels), {})[m.dilation[0]] = cw.PIECES
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    world_gt, imgs_gt = synthetic_frame_targets(geom, PEOPLE, seed=0)
    world_gt, imgs_gt = ({k: v.to(DEV) for k, v in d.items()} for d in (world_gt, imgs_gt))
    imgs = torch.randn(1, geom.num_cam, 3, *geom.input_img_shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    M = torch.eye(3).repeat(1, geom.num_cam, 1, 1)
    crit = MVDeTrCriterion()
    launches = {}

    def side(name, on):
        def run():
            prev = cw.set_trunk_winograd_training(on)
            n0 = cw.launch_count()
            try:
                return train_step(model, crit, opt, imgs, M, world_gt, imgs_gt)
            finally:
                launches[name] = cw.launch_count() - n0
                cw.set_trunk_winograd_training(prev)
        return run

    res = alternated({"on": side("on", True), "off": side("off", False)}, reps, warmup=2)
    table = {f"{C}->{K} d {d}": "+".join(p) for (C, K), ds in sorted(cw.TRAIN_FAMILIES.items()) for d, p in sorted(ds.items()) if p}
    lines = [f"# one Wildtrack training step (train_step, Adam, fp32, deform_trans), set_trunk_winograd_training on against off, "
             f"alternated in one process; {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {reps} (min .. max), ms",
             f"# TRAIN_FAMILIES ({families}): {table if table else 'empty -- both sides run the same launches'}",
             f"# Winograd launches in a step: on {launches['on']}, off {launches['off']} (off: none -- the launches of the code without the route)"]
    for clock in ("device", "wall"):
        for name in ("on", "off"):
            med, lo, hi = res[name][clock]
            lines.append(f"{clock:<7} {name:<4} {med / 1e3:9.3f}  ({lo / 1e3:.3f} .. {hi / 1e3:.3f})")
        lines.append(f"{clock:<7} off - on = {(res['off'][clock][0] - res['on'][clock][0]) / 1e3:+.3f} ms")
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--winograd-train", action="store_true", help="A/B of the trunk's Winograd training convolutions on the whole step")
    ap.add_argument("--families", choices=("shipped", "all"), default="shipped")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_step_bench: needs a GPU (no CPU fallback for timings)")
    reps = max(20, a.reps)
    if a.winograd_train:
        return bench_winograd_train(reps, a.families, a.out)
    print(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {reps} alternated repetitions (min .. max)")
    rows = []
    for name in ("wildtrack", "multiviewx"):
        bench_objective(name, reps, rows)
    if not a.skip_step:
        bench_step(reps, rows)
    print(f"\n{'what':<40} {'size':<11} {'clock':<7} {'impl':<18} {'median us':>10} {'min':>10} {'max':>10} {'/ hip':>6}")
    for r in rows:
        print(f"{r['what']:<40} {r['size']:<11} {r['clock']:<7} {r['impl']:<18} {r['median_us']:>10.1f} {r['min_us']:>10.1f} "
              f"{r['max_us']:>10.1f} {r['ratio_to_hip']:>6.2f}")
    by = {(r["what"], r["size"], r["clock"], r["impl"]): r for r in rows}
    for (what, size, clock, impl), r in by.items():
        if impl != "hip":
            continue
        o = by[(what, size, clock, "torch_composition")]
        diff, spread = o["median_us"] - r["median_us"], max(o["max_us"] - o["min_us"], r["max_us"] - r["min_us"])
        verdict = "inside" if abs(diff) <= spread else "outside"
        print(f"# {what} / {size} / {clock}: composition - hip = {diff:+.1f} us; larger run-to-run spread {spread:.1f} us: {verdict} the spread")


if __name__ == "__main__":
    np.seterr(all="ignore")
    main()
