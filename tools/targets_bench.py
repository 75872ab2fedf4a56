"""Times the building of one frame's training targets two ways, alternated repetition by repetition in one process:

  host      what a dataset worker does: augment.affine_boxes (with M) + targets.get_gt per map in numpy, the dataloader's
            collate, and the copies of the collated dicts to the device;
  device    targets.frame_targets on annotations that already live on the device (two launches of csrc/frame_targets.hip);
            with M the matrices go up from the host, as they do for ingest anyway.

    python tools/targets_bench.py [--reps N] [--runs R]

Shapes: Wildtrack (7 views of [90, 160], world [120, 360]) and MultiviewX (6 views of [90, 160], world [160, 250]), B = 1, 40
people, with and without an augmentation M.  Each repetition is timed with the host clock from the call to the end of a device
synchronise (the host variant's time IS host work; the device variant's includes its launch overhead), after a warm-up of both;
the table gives the median over R >= 5 runs of the runs' medians and the p10 - p90 of all repetitions, plus the device-event time
of the device variant, its launches (the library's counter) and the bytes of targets the host variant copies up and the device
variant does not.  No ratio is claimed: what the device path buys is the host work and the copies.  Prints one JSON line per row
and a table."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mvdetr_amd import augment, geometry  # noqa: E402
from mvdetr_amd.ops import targets as ops_targets  # noqa: E402
from mvdetr_amd.targets import frame_targets, get_gt, synthetic_frame_annotations  # noqa: E402

DEV = "cuda:0"
PEOPLE = 40


def matrices(geom, seed):
    rng = np.random.default_rng(seed)
    angles = [float(rng.uniform(-10, 10)) if c % 3 == 0 else 0.0 for c in range(geom.num_cam)]
    M = [augment.affine_matrix(geom.img_shape, hflip=bool(rng.integers(2)), angle=angles[c], scale=float(rng.uniform(0.6, 1.4)),
                               tx=float(rng.uniform(-0.2, 0.2) * geom.img_shape[1]), ty=float(rng.uniform(-0.2, 0.2) * geom.img_shape[0]))
         for c in range(geom.num_cam)]
    return torch.from_numpy(np.stack(M))[None], torch.tensor([angles], dtype=torch.float64)


def host_targets(geom, ann, M, angles):
    """One frame (B = 1) as the dataset + collate build it, then copied to the device."""
    n = int(ann.world_count[0])
    p = ann.world_pts[0, :n].numpy()
    world = get_gt(geom.Rworld_shape, p[:, 0], p[:, 1], v_s=ann.world_pids[0, :n].numpy(), reduce=geom.world_reduce, top_k=100,
                   kernel_size=10)
    per_view = []
    for c in range(geom.num_cam):
        n = int(ann.box_count[0, c])
        b, pid = ann.boxes[0, c, :n].numpy(), ann.box_pids[0, c, :n].numpy()
        if M is not None:
            b, pid = augment.affine_boxes(b, pid, M[0, c].numpy(), geom.img_shape, float(angles[0, c]))
        per_view.append(get_gt(geom.Rimg_shape, (b[:, 0] + b[:, 2]) / 2, b[:, 3], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1], v_s=pid,
                               reduce=geom.img_reduce, top_k=100, kernel_size=10))
    world_gt = {k: v[None].to(DEV, non_blocking=True) for k, v in world.items()}
    imgs_gt = {k: torch.stack([v[k] for v in per_view])[None].to(DEV, non_blocking=True) for k in per_view[0]}
    return world_gt, imgs_gt


def one_run(fns, reps, warmup=3):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    wall, dev = {n: [] for n in fns}, {n: [] for n in fns}
    for _ in range(reps):
        for n, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            wall[n].append((time.perf_counter() - t0) * 1e6)
            dev[n].append(a.elapsed_time(b) * 1e3)
    return wall, dev


def pct(values, q):
    v = sorted(values)
    return v[min(len(v) - 1, int(q * len(v)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("targets_bench: needs a GPU (no CPU fallback for timings)")
    runs = max(5, a.runs)
    print(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; us per frame of targets (B = 1, {PEOPLE} people), host "
          f"clock from the call to the end of a device synchronise; median over {runs} runs of each run's median ({a.reps} alternated "
          f"repetitions a run), p10 - p90 of all repetitions")
    rows = []
    for geom in (geometry.WILDTRACK, geometry.MULTIVIEWX):
        ann = synthetic_frame_annotations(geom, PEOPLE, seed=0)
        dev_ann = [t.to(DEV) for t in ann]
        for with_m in (False, True):
            M, angles = matrices(geom, 1) if with_m else (None, None)
            fns = {"host": lambda: host_targets(geom, ann, M, angles),
                   "device": lambda: frame_targets(geom, *dev_ann, M=M, angles=angles)}
            want, got = fns["host"](), fns["device"]()
            same = all(torch.equal(w[k], g[k]) for w, g in zip(want, got) for k in ("heatmap", "reg_mask", "idx", "pid"))
            close = all(torch.allclose(w[k], g[k], rtol=2e-7, atol=0) for w, g in zip(want, got) for k in w if k in ("offset", "wh"))
            copied = sum(v.numel() * v.element_size() for d in want for v in d.values())
            n0 = ops_targets.launch_count()
            fns["device"]()
            launches = ops_targets.launch_count() - n0
            per_run = [one_run(fns, a.reps) for _ in range(runs)]
            for impl in fns:
                meds = [pct(w[impl], 0.5) for w, _ in per_run]
                every = [t for w, _ in per_run for t in w[impl]]
                dev_meds = [pct(d[impl], 0.5) for _, d in per_run]
                row = {"shape": geom.name, "with_M": with_m, "impl": impl, "targets_equal_host": bool(same and close),
                       "launches": launches if impl == "device" else None,
                       "target_bytes_copied": copied if impl == "host" else 0,
                       "median_us": round(pct(meds, 0.5), 1), "p10_us": round(pct(every, 0.1), 1), "p90_us": round(pct(every, 0.9), 1),
                       "device_event_median_us": round(pct(dev_meds, 0.5), 1)}
                rows.append(row)
                print(json.dumps(row), flush=True)
    print(f"\n{'shape':<11} {'M':<5} {'impl':<7} {'launches':>8} {'bytes copied':>13} {'median us':>10} {'p10':>9} {'p90':>9} {'dev events us':>14}")
    for r in rows:
        print(f"{r['shape']:<11} {str(r['with_M']):<5} {r['impl']:<7} {str(r['launches'] or '-'):>8} {r['target_bytes_copied']:>13} "
              f"{r['median_us']:>10.1f} {r['p10_us']:>9.1f} {r['p90_us']:>9.1f} {r['device_event_median_us']:>14.1f}")


if __name__ == "__main__":
    main()
