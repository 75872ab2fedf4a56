"""Times the last stage of inference on the GPU -- world heat map -> ground-plane detections -- four ways, alternated
repetition by repetition in one process, on maps that already live on the device (as the model returns them):

  ref_cpu         the reference's way (trainer.py:121-135): copy both maps to the host, decode + threshold + NMS loop there;
  loop_gpu        utils.detections_from_heatmap on the GPU tensors: the same loop, every iteration a few small kernels and a
                  read-back;
  fused           ops.bev_detect (csrc/detect.hip, two launches), result left on the device;
  fused_readback  utils.detections_from_heatmap_fused: the same plus its one read-back (the counts) and the row gather.

    python tools/detect_bench.py [--reps N]

Shapes: Wildtrack (120 x 360) and MultiviewX (160 x 250) maps, one frame, channels_last.  Inputs: `people` -- 40 Gaussian
blobs of peak logit +3 over a -2.19 background, the realistic case; `all_above` -- every cell over the threshold, the worst
case (every cell is a candidate, hundreds of sequential keeps).  Two clocks per repetition, as tools/train_step_bench.py:
device-event time between the first and the last enqueued kernel, and host wall time from the call to the end of a
synchronise behind it.  Medians of N after warm-up with (min .. max).  Prints one JSON line per row and a table."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mvdetr_amd.ops import bev_detect  # noqa: E402
from mvdetr_amd.utils import detections_from_heatmap, detections_from_heatmap_fused  # noqa: E402

DEV = "cuda:0"
SHAPES = {"wildtrack": (120, 360), "multiviewx": (160, 250)}


def alternated(fns, reps, warmup=2):
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


def maps(kind, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    off = torch.rand(1, 2, H, W, generator=g)
    if kind == "all_above":
        hm = torch.rand(1, 1, H, W, generator=g) * 4                       # scores 0.5 .. 0.98
    else:
        ys, xs = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
        cy, cx = torch.rand(40, generator=g) * H, torch.rand(40, generator=g) * W
        d2 = (ys[None] - cy[:, None, None]) ** 2 + (xs[None] - cx[:, None, None]) ** 2
        hm = (-2.19 + 5.19 * torch.exp(-d2 / (2 * 1.5 ** 2)).amax(0)).view(1, 1, H, W)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last).to(DEV)  # noqa: E731
    return cl(hm), cl(off)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detect_bench: needs a GPU (no CPU fallback for timings)")
    print(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; medians of alternated repetitions (min .. max)")
    rows = []
    for kind in ("people", "all_above"):
        reps = max(20, a.reps) if kind == "people" else 5
        for name, (H, W) in SHAPES.items():
            hm, off = maps(kind, H, W)
            fns = {
                "ref_cpu": lambda: detections_from_heatmap(hm.cpu(), off.cpu(), [0]),
                "loop_gpu": lambda: detections_from_heatmap(hm, off, [0]),
                "fused": lambda: bev_detect(hm, off),
                "fused_readback": lambda: detections_from_heatmap_fused(hm, off, [0]),
            }
            want, got = fns["ref_cpu"](), fns["fused_readback"]().cpu()
            det = bev_detect(hm, off)
            extra = {"candidates": int((torch.sigmoid(hm) > 0.4).sum()), "kept": int(det.count), "reps": reps,
                     "rows_equal_ref_cpu": bool(want.shape == got.shape and torch.equal(want, got))}
            res = alternated(fns, reps)
            for clock in ("device", "wall"):
                base = res["fused"][clock][0]
                for impl, r in res.items():
                    med, lo, hi = r[clock]
                    row = {"input": kind, "size": name, "clock": clock, "impl": impl, "median_us": round(med, 1),
                           "min_us": round(lo, 1), "max_us": round(hi, 1), "ratio_to_fused": round(med / base, 2)}
                    row.update(extra)
                    print(json.dumps(row), flush=True)
                    rows.append(row)
    print(f"\n{'input':<10} {'size':<11} {'cand':>6} {'kept':>5} {'clock':<7} {'impl':<15} {'median us':>11} {'min':>11} {'max':>11} {'/ fused':>8}")
    for r in rows:
        print(f"{r['input']:<10} {r['size']:<11} {r['candidates']:>6} {r['kept']:>5} {r['clock']:<7} {r['impl']:<15} {r['median_us']:>11.1f} "
              f"{r['min_us']:>11.1f} {r['max_us']:>11.1f} {r['ratio_to_fused']:>8.2f}")


if __name__ == "__main__":
    main()
