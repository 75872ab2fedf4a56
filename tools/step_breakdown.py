#!/usr/bin/env python3
"""Where one steady-state frame of the plain benchmark goes, kernel by kernel, from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace -d trace -o t -- python bench.py --steps 20 --warmup 5
    python tools/step_breakdown.py trace/t_results.db [--frames 10]

A plain run launches warp_fwd_cl exactly once per frame.  The last K+1 of those launches bound K windows of one frame
period each (the rest of frame j behind its warp, then frame j+1 up to its warp: in steady state the same kernels as one
frame), which keeps MIOpen's find phase and the calibration frames at the start of the process out of the averages.
Prints per kernel name: launches, microseconds and share per frame (averages over the K windows), and the totals of four
groups -- MIOpen / CK convolutions, the elementwise passes between them, this library's kernels, GEMMs."""
import argparse
import re
import sqlite3
from collections import defaultdict

GROUPS = ("convolutions (MIOpen / CK)", "elementwise passes", "this library", "GEMMs", "other")


def group_of(name):
    if "mvdetr::" in name:
        # the trunk's fused passes and its Winograd convolutions are work moved into this library: counted with what they replace
        if re.search(r"conv3x3_winograd", name):
            return GROUPS[0]
        return GROUPS[1] if re.search(r"bn_act_cl|bn_relu_maxpool", name) else GROUPS[2]
    if re.search(r"BatchNorm|elementwise_kernel|max_pool|batched_transpose|SubTensorOp|direct_copy|copy_kernel|CatArrayBatchedCopy|"
                 r"upsample|index_elementwise|reduce_kernel|FillFunctor|transpose_kernel", name):
        return GROUPS[1]
    if re.search(r"Cijk_|gemm|rocblas|hipblaslt", name, re.I) and not re.search(r"igemm|implicit|conv", name, re.I):
        return GROUPS[3]
    if re.search(r"miopen|igemm|implicit_gemm|winograd|conv_fwd|Conv|naive_conv|^_ZN2ck|ck::", name):
        return GROUPS[0]
    return GROUPS[4]


def short(name, n=96):
    name = re.sub(r"^void ", "", name)
    if name.endswith(")"):                                       # the argument list: the last balanced (...) group
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += (name[i] == ")") - (name[i] == "(")
            if depth == 0:
                name = name[:i]
                break
    name = name.replace("at::native::", "").replace("(anonymous namespace)::", "")
    name = re.sub(r"\(.*?\)::\{lambda\(.*?\)#\d+\}", "", name)    # launch_clamp_scalar(...)::{lambda()#1}::operator()...
    return name if len(name) <= n else name[:n - 3] + "..."


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--frames", type=int, default=10, help="K: frame periods averaged, counted back from the last warp launch")
    ap.add_argument("--marker", default="warp_fwd_cl", help="substring of the once-per-frame kernel's name")
    a = ap.parse_args()
    rows = sqlite3.connect(a.db).cursor().execute("select name, start, duration from kernels order by start").fetchall()
    marks = [i for i, (name, _, _) in enumerate(rows) if a.marker in name]
    if len(marks) < 2:
        raise SystemExit(f"{a.db}: {len(marks)} launches of {a.marker}: not a trace of the plain benchmark")
    K = min(a.frames, len(marks) - 1)
    first, last = marks[-K - 1], marks[-1]
    window = rows[first:last]
    wall_us = (rows[last][1] - rows[first][1]) / 1e3 / K
    per = defaultdict(lambda: [0, 0.0])
    groups = defaultdict(lambda: [0, 0.0])
    for name, _, dur in window:
        for d in (per[name], groups[group_of(name)]):
            d[0] += 1
            d[1] += dur / 1e3
    busy_us = sum(v[1] for v in per.values()) / K
    print(f"# {a.db}: {K} frame periods between the last {K + 1} launches of {a.marker} ({len(marks)} in the trace)")
    print(f"# per frame: {len(window) / K:.1f} launches, {busy_us:.1f} us of kernel time, {wall_us:.1f} us from marker to marker "
          f"(under the tracer)")
    print(f"{'group':32s} {'launches':>9s} {'us':>10s} {'share':>7s}")
    for g in GROUPS:
        n, us = groups[g]
        print(f"{g:32s} {n / K:9.1f} {us / K:10.1f} {us / K / busy_us * 100:6.1f}%")
    print()
    print(f"{'kernel':98s} {'group':>12s} {'launches':>9s} {'us':>10s} {'avg us':>9s} {'share':>7s}")
    for name, (n, us) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        print(f"{short(name):98s} {group_of(name).split()[0]:>12s} {n / K:9.1f} {us / K:10.1f} {us / n:9.1f} {us / K / busy_us * 100:6.1f}%")


if __name__ == "__main__":
    main()
