"""Times the frame ingest (ops.ingest_frames: uint8 camera frames -> the trunk's normalised, resized, channels-last input) on the
GPU against the torch composition a user would otherwise write, interleaved in one process:

  hip        ingest_frames, one kernel (csrc/ingest.hip);
  torch      the reference's order on the device: permute, float, / 255, normalise, F.interpolate(bilinear), channels-last copy,
             cast (identity rows only: torch has no perspective image warp to compare the augmented rows with).

    python tools/ingest_bench.py [--reps N] [--out profiles/ingest_bench.txt]

Rows: Wildtrack (7 cameras) and MultiviewX (6 cameras), 1080 x 1920 -> 720 x 1280; identity and augmented (one random_affine
matrix per camera); float32 and bfloat16; channels-last.  Every figure is the median of N (>= 20) device-event times after
warm-up with p10 .. p90 beside it; the implementations of one row are timed alternately, repetition by repetition.  Bytes are
what the op must move -- the frames read once, the result written once -- and the share is that over the measured time against
the 6.29 TB/s device copy rate (profiles/r06_copy_calibration.txt).  Prints one JSON line per row, a table and, for the identity
float32 rows, whether the HIP median is below torch's by more than the two p10 .. p90 spreads added together."""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBS = 6.29
SCENES = {"wildtrack": 7, "multiviewx": 6}
SRC, DST = (1080, 1920), (720, 1280)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def interleaved(fns, reps, warmup=5):
    """{name: (median, p10, p90)} in us; the functions are run alternately so that clocks and caches treat them alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    times = {n: [] for n in fns}
    for _ in range(reps):
        for n, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[n].append(a.elapsed_time(b) * 1e3)
    out = {}
    for n, t in times.items():
        t = sorted(t)
        out[n] = (t[len(t) // 2], t[int(0.1 * (len(t) - 1))], t[int(round(0.9 * (len(t) - 1)))])
    return out


def torch_composition(frames, dtype):
    mean = torch.tensor(MEAN, device=frames.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, device=frames.device).view(1, 3, 1, 1)

    def run():
        x = frames.permute(0, 3, 1, 2).float() / 255.0
        x = (x - mean) / std
        x = F.interpolate(x, size=DST, mode="bilinear", align_corners=False, antialias=False)
        return x.contiguous(memory_format=torch.channels_last).to(dtype)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_bench: needs a GPU (no CPU fallback for timings)")
    from mvdetr_amd import augment
    from mvdetr_amd.ops import ingest_frames
    from mvdetr_amd.ops.ingest import last_kernel
    reps = max(20, a.reps)
    dev = torch.device("cuda:0")
    lines = [f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {reps} interleaved repetitions (p10 .. p90), "
             f"device events; {SRC} -> {DST}, channels-last; share = (bytes read + written) / time / {COPY_TBS} TB/s"]
    print(lines[0], flush=True)
    rows, verdicts = [], []
    for scene, K in SCENES.items():
        g = torch.Generator().manual_seed(K)
        frames = torch.randint(0, 256, (K,) + SRC + (3,), dtype=torch.uint8, generator=g).to(dev)
        np.random.seed(K)
        random.seed(K)
        M = torch.from_numpy(np.stack([augment.random_affine(SRC, np.zeros((0, 4)), np.zeros(0))[2] for _ in range(K)])).to(dev)
        for mode in ("identity", "augmented"):
            for dtype in (torch.float32, torch.bfloat16):
                mats = M if mode == "augmented" else None
                fns = {"hip": lambda: ingest_frames(frames, mats, DST, dtype=dtype)}
                if mode == "identity":
                    fns["torch"] = torch_composition(frames, dtype)
                    diff = (fns["hip"]().float() - fns["torch"]().float()).abs().max().item()
                else:
                    fns["hip"]()
                    diff = None
                kern = last_kernel()
                res = interleaved(fns, reps)
                nbytes = frames.numel() + K * 3 * DST[0] * DST[1] * torch.finfo(dtype).bits // 8
                for impl, (med, lo, hi) in res.items():
                    row = {"scene": scene, "cameras": K, "mode": mode, "dtype": str(dtype).replace("torch.", ""), "impl": impl,
                           "median_us": round(med, 1), "p10_us": round(lo, 1), "p90_us": round(hi, 1), "bytes": nbytes,
                           "tb_per_s": round(nbytes / med / 1e6, 3), "share_of_copy_rate": round(nbytes / med / 1e6 / COPY_TBS, 4)}
                    if impl == "hip":
                        row["kernel"] = kern
                        if diff is not None:
                            row["max_abs_diff_vs_torch"] = diff
                    lines.append(json.dumps(row))
                    print(lines[-1], flush=True)
                    rows.append(row)
                if mode == "identity" and dtype == torch.float32:
                    (hm, hl, hh), (tm, tl, th) = res["hip"], res["torch"]
                    ok = tm - hm > (hh - hl) + (th - tl)
                    verdicts.append(f"{scene} identity float32: hip {hm:.1f} us ({hl:.1f} .. {hh:.1f}), torch {tm:.1f} us ({tl:.1f} .. {th:.1f}); "
                                    f"difference {tm - hm:.1f} us vs spreads {(hh - hl) + (th - tl):.1f} us -> "
                                    + ("hip is faster beyond the spreads" if ok else "NOT separated: no claim"))
        del frames
        torch.cuda.empty_cache()
    lines.append("")
    lines.append(f"{'scene':<11} {'mode':<10} {'dtype':<9} {'impl':<6} {'median us':>10} {'p10':>9} {'p90':>9} {'MB':>7} {'TB/s':>7} {'share':>7}  kernel")
    for r in rows:
        lines.append(f"{r['scene']:<11} {r['mode']:<10} {r['dtype']:<9} {r['impl']:<6} {r['median_us']:>10.1f} {r['p10_us']:>9.1f} {r['p90_us']:>9.1f} "
                     f"{r['bytes'] / 1e6:>7.1f} {r['tb_per_s']:>7.3f} {100 * r['share_of_copy_rate']:>6.1f}%  {r.get('kernel', '')}")
    lines.append("")
    lines += verdicts
    print("\n".join(lines[len(rows) + 1:]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
