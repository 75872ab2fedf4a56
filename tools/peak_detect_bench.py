"""Times the per-view (and peak-based world) decode on the GPU -- heat map + offset + wh -> top-100 peaks -- three ways,
alternated repetition by repetition in one process, on maps that already live on the device (as the model returns them):

  ctdet_decode     utils.ctdet_decode on the GPU tensors: the reference's chain of torch ops (sigmoid, max_pool2d, compare,
                   multiply, two topk, index arithmetic, gathers, cat);
  fused            ops.peak_detect (csrc/peak_detect.hip, two launches), result left on the device;
  fused_readback   the same plus one read-back of ``count``.

    python tools/peak_detect_bench.py [--reps N] [--runs R]

Shapes: the Wildtrack view maps [7,1,90,160], MultiviewX's [6,1,90,160], and the two world maps [1,1,120,360] and
[1,1,160,250].  Inputs: `blobs` -- 40 Gaussian blobs of peak logit +3 over a -2.19 background per map, the realistic case;
`noise` -- white noise, about one cell in nine a peak.  A run is N alternated repetitions after a warm-up of every variant,
each timed with device events around the call; the table gives the median over R >= 5 runs of the runs' medians, and the
p10 - p90 of all repetitions.  Kernel launches per call: counted by the profiler for ctdet_decode, by the library's own
counter for the fused path.  Prints one JSON line per row and a table."""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mvdetr_amd.ops import peak_detect  # noqa: E402
from mvdetr_amd.utils import ctdet_decode  # noqa: E402

peak_mod = importlib.import_module("mvdetr_amd.ops.peak_detect")

DEV = "cuda:0"
SHAPES = {"wildtrack_views": (7, 90, 160), "multiviewx_views": (6, 90, 160), "wildtrack_world": (1, 120, 360),
          "multiviewx_world": (1, 160, 250)}
TOP_K = 100


def maps(kind, B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    off = torch.rand(B, 2, H, W, generator=g)
    wh = torch.rand(B, 2, H, W, generator=g) * 6 + 1
    if kind == "noise":
        hm = torch.randn(B, 1, H, W, generator=g) * 2
    else:
        ys, xs = torch.meshgrid(torch.arange(H).float(), torch.arange(W).float(), indexing="ij")
        cy, cx = torch.rand(B, 40, generator=g) * H, torch.rand(B, 40, generator=g) * W
        d2 = (ys - cy[..., None, None]) ** 2 + (xs - cx[..., None, None]) ** 2
        hm = (-2.19 + 5.19 * torch.exp(-d2 / (2 * 1.5 ** 2)).amax(1)).view(B, 1, H, W)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last).to(DEV)  # noqa: E731
    return cl(hm), cl(off), cl(wh)


def one_run(fns, reps, warmup=3):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    times = {n: [] for n in fns}
    for _ in range(reps):
        for n, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[n].append(a.elapsed_time(b) * 1e3)
    return times


def torch_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
               and "Memset" not in e.name)


def pct(values, q):
    v = sorted(values)
    return v[min(len(v) - 1, int(q * len(v)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("peak_detect_bench: needs a GPU (no CPU fallback for timings)")
    runs = max(5, a.runs)
    print(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; device-event time per call in us; median over "
          f"{runs} runs of each run's median ({a.reps} alternated repetitions a run), p10 - p90 of all repetitions")
    rows = []
    for kind in ("blobs", "noise"):
        for name, (B, H, W) in SHAPES.items():
            hm, off, wh = maps(kind, B, H, W)
            fns = {
                "ctdet_decode": lambda: ctdet_decode(hm, off, wh, top_K=TOP_K),
                "fused": lambda: peak_detect(hm, off, wh, top_k=TOP_K),
                "fused_readback": lambda: peak_detect(hm, off, wh, top_k=TOP_K).count.cpu(),
            }
            det = peak_detect(hm, off, wh, top_k=TOP_K)
            route = peak_mod.last_kernel()
            want = ctdet_decode(hm, off, wh, top_K=TOP_K)
            live = (torch.arange(TOP_K, device=DEV)[None] < det.count[:, None])
            same = bool(torch.equal(det.xy[live], want[..., :2][live]) and torch.equal(det.wh[live], want[..., 2:4][live]))
            n0 = peak_mod.launch_count()
            fns["fused"]()
            launches = {"ctdet_decode": None, "fused": peak_mod.launch_count() - n0}
            launches["fused_readback"] = launches["fused"]
            per_run = [one_run(fns, a.reps) for _ in range(runs)]
            base = None
            for impl in fns:
                meds = [pct(r[impl], 0.5) for r in per_run]
                every = [t for r in per_run for t in r[impl]]
                row = {"input": kind, "shape": name, "maps": B, "candidates_max": int(det.count.max()), "route": route,
                       "rows_equal_ctdet_decode": same, "impl": impl, "launches": launches[impl],
                       "median_us": round(pct(meds, 0.5), 1), "p10_us": round(pct(every, 0.1), 1), "p90_us": round(pct(every, 0.9), 1)}
                rows.append(row)
            base = next(r for r in rows[-3:] if r["impl"] == "fused")["median_us"]
            for r in rows[-3:]:
                r["ratio_to_fused"] = round(r["median_us"] / base, 2)
                print(json.dumps(r), flush=True)
    # the torch chain's launches, counted by the profiler once the timings are done (the profiler stays loaded afterwards)
    for kind in ("blobs", "noise"):
        for name, (B, H, W) in SHAPES.items():
            hm, off, wh = maps(kind, B, H, W)
            try:
                count = torch_launches(lambda: ctdet_decode(hm, off, wh, top_K=TOP_K))
            except Exception as e:                                          # noqa: BLE001  a build of torch without the profiler
                print(f"# launches of ctdet_decode not counted: {e}")
                count = -1
            for r in rows:
                if r["input"] == kind and r["shape"] == name and r["impl"] == "ctdet_decode":
                    r["launches"] = count
            print(json.dumps({"input": kind, "shape": name, "impl": "ctdet_decode", "launches": count}), flush=True)
    print(f"\n{'input':<6} {'shape':<17} {'cand':>6} {'impl':<15} {'launches':>8} {'median us':>10} {'p10':>8} {'p90':>8} {'/ fused':>8}")
    for r in rows:
        print(f"{r['input']:<6} {r['shape']:<17} {r['candidates_max']:>6} {r['impl']:<15} {r['launches']:>8} {r['median_us']:>10.1f} "
              f"{r['p10_us']:>8.1f} {r['p90_us']:>8.1f} {r['ratio_to_fused']:>8.2f}")


if __name__ == "__main__":
    main()
