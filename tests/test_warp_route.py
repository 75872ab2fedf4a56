"""The perspective warp's route table (csrc/warp_route.h), checked without a GPU and without loading the library: the header is
plain C++, so a small stand-alone program compiled with g++ prints the route of every row below and the test compares it with
the route written next to the row.  The rows are the dispatch of every C ABI entry of the warp -- fp32 / fp64 forward and
backward, the 16-bit forward, and the two-step gradient's plan-bytes, plan and planned entries -- with every limit at which a
call changes kernel or is refused, from both sides.

A printed route is `<name> <zero_first> <lgG> <cgroups> <plan_bytes> <grid> <plan_key>`: the name mvdetr_warp_last_kernel reports
from the call on (`none`, `zero_fill` or `plan` for the kinds that leave it alone); whether grad_src is zeroed in front of the
kernel; the gather's lanes per hit stream (log2) and channel groups per block; the size of the plan; the workgroups of the launch;
and what the scratch cache keys a plan's contents by (from MVDETR_WARP_BWD_GEOMETRY and MVDETR_WARP_BWD_HEAVY).  A refused or
empty call prints its status alone; the C ABI turns `empty` into 0, `invalid_value` into 1, `not_supported` into 801 (the
plan-bytes entry: into 0 bytes).

Oddities the table pins as they are (the refactor that introduced it changed no behaviour): the 16-bit entry alone refuses
h * w beyond an int; a channel-last source with a partial 16-byte chunk or a misaligned pointer is not_supported in the fp32 /
fp64 entries but runs warp_fwd_half in the 16-bit one; a patch-kernel grid that does not fit falls back to warp_fwd<NCHW> instead
of refusing; the plan entries look at their pointers first and answer not_supported for non-positive sizes; the planned entry
does not look at the plan's alignment."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvdetr_amd", "csrc")

PROGRAM = r"""
#include "warp_route.h"
#include <stdio.h>
using namespace mvdetr;
int main()
{
    char entry[16], knob[5][32];
    int elem, N, C, h, w, H, W, layout, f[7];
    while (scanf("%15s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %31s %31s %31s %31s %31s", entry, &elem, &N, &C, &h, &w, &H, &W, &layout,
                 f, f + 1, f + 2, f + 3, f + 4, f + 5, f + 6, knob[0], knob[1], knob[2], knob[3], knob[4]) == 21) {
        static const char *const entries[] = {"forward", "backward", "half", "plan_bytes", "plan", "planned"};
        int e = 0;
        while (strcmp(entry, entries[e])) ++e;
        const char *k[5];
        for (int i = 0; i < 5; ++i) k[i] = strcmp(knob[i], "-") ? knob[i] : nullptr;
        const WarpKnobs knobs = warp_parse_knobs(k[0], k[1], k[2], k[3], k[4]);
        const WarpRoute r = warp_route(WarpQuery{(WarpEntry)e, elem, N, C, h, w, H, W, layout, f[0] != 0, f[1] != 0, f[2] != 0, f[3] != 0,
                                                 f[4] != 0, f[5] != 0, f[6] != 0, knobs});
        static const char *const status[] = {"ok", "empty", "invalid_value", "not_supported"};
        const char *name = r.name ? r.name : r.kind == WarpKind::zero_fill ? "zero_fill" : r.kind == WarpKind::plan ? "plan" : "none";
        if (r.status != WarpStatus::ok) printf("%s\n", status[(int)r.status]);
        else printf("%s %d %d %d %lld %lld %lld\n", name, r.zero_first, r.lgG, r.cgroups, (long long)r.plan_bytes, (long long)r.grid,
                    (long long)knobs.plan_key());
    }
    return 0;
}
"""

I31 = 2 ** 31 - 1
KNOBS = ("impl", "geometry", "heavy", "heavy_wgs", "fwd")


def row(entry, elem, want, *, N=1, C=8, h=5, w=6, H=7, W=9, layout=0, ptrs="1111", al="111", **knobs):
    """One query.  ptrs: in, M, out, plan non-null; al: in, out, plan 16-byte aligned; knobs: the five environment words."""
    assert not set(knobs) - set(KNOBS)
    args = (entry, elem, N, C, h, w, H, W, layout) + tuple(int(c) for c in ptrs + al) + tuple(knobs.get(k, "-") for k in KNOBS)
    return [(args, want)]


def rows(entry, elems, want, **kw):
    return sum((row(entry, e, want, **kw) for e in elems), [])


def plan_bytes(N, h, w, H, W):
    """[counts: 2 + 1024 ints | 2 scans of 40 bytes per 2 x 2 block | a block list | 1024 segments of destination pixels]"""
    nblk, npix = N * ((h + 1) // 2) * ((w + 1) // 2), N * H * W
    pad = lambda b: (b + 15) // 16 * 16
    return pad(1026 * 4) + nblk * 80 + pad(nblk * 4) + (npix + 1023) // 1024 * 1024 * 4


def tiles(H, W, th=8, tw=8):
    return ((H + th - 1) // th) * ((W + tw - 1) // tw)


PB = plan_bytes(1, 5, 6, 7, 9)                  # the default shapes' plan
assert PB == 8976
HW = 2048 + 3                                   # the default gather grid at the default shapes: 9 blocks in 3 light workgroups


def launch(name, grid, zero=0, key=0):
    return f"{name} {zero} 0 0 0 {grid} {key}"


def gather(lgG, cgroups, *, name="warp_bwd_gather", pb=PB, grid=HW, key=0):
    return f"{name} 0 {lgG} {cgroups} {pb} {grid} {key}"


F, D = (4,), (8,)
FD = (4, 8)

ROWS = (
    # ---- forward, NCHW source: every kind for every element size that reaches it, bilinear and nearest
    rows("forward", FD, launch("warp_fwd<NCHW>", 2))
    + rows("forward", FD, launch("warp_fwd<NHWC>", 2), layout=1)
    + rows("forward", FD, launch("warp_fwd<NCHW>", 2), layout=4)
    + rows("forward", FD, launch("warp_fwd<NHWC>", 2), layout=5)
    + rows("forward", FD, launch("warp_fwd<NCHW>", 6), C=129)                           # three channel groups of 64
    # the LDS-patch kernel: fp32, NCHW destination, rows of a multiple of 4 texels, aligned source, a view below 2 GiB
    + row("forward", 4, launch("warp_fwd_nchw_patch", 1), w=8)
    + row("forward", 4, launch("warp_fwd_nchw_patch", 1), w=8, layout=4)
    + row("forward", 4, launch("warp_fwd_nchw_patch", 8), w=8, C=33, H=9, W=33)         # 2 x 2 tiles of 8 x 32, 2 groups of 32
    + row("forward", 8, launch("warp_fwd<NCHW>", 2), w=8)
    + row("forward", 4, launch("warp_fwd<NHWC>", 2), w=8, layout=1)
    + sum((row("forward", 4, launch("warp_fwd<NCHW>", 2), w=w) for w in (5, 6, 7, 9)), [])
    + row("forward", 4, launch("warp_fwd<NCHW>", 2), w=8, al="011")                      # source not 16-byte aligned
    + row("forward", 4, launch("warp_fwd_nchw_patch", 1), w=8, al="100")                 # the destination need not be
    + row("forward", 4, launch("warp_fwd_nchw_patch", 1), w=4, C=1, h=(I31 // 16))       # C h w 4 = 2^31 - 16: the last view taken
    + row("forward", 4, launch("warp_fwd<NCHW>", 2), w=4, C=1, h=(I31 // 16) + 1)        # 2^31
    + row("forward", 4, launch("warp_fwd<NCHW>", 2), w=8, fwd="gather")
    + row("forward", 4, launch("warp_fwd_nchw_patch", 1), w=8, fwd="bogus")
    + row("forward", 4, launch("warp_fwd_nchw_patch", 1, key=257), w=8, fwd="scatter", impl="scatter", geometry="clip", heavy="0", heavy_wgs="1")
    # grids: the gather kernel's 8 x 8 tiles x channel groups of 64, the patch kernel's 8 x 32 tiles x groups of 32
    + rows("forward", FD, launch("warp_fwd<NCHW>", I31), N=I31, H=8, W=8, C=64)
    + rows("forward", FD, "invalid_value", N=I31, H=9, W=8, C=64)
    + rows("forward", FD, "invalid_value", N=I31, H=8, W=8, C=65)
    + row("forward", 4, launch("warp_fwd<NCHW>", I31), N=I31, H=8, W=8, C=64, w=8)       # the patch grid (2 groups of 32) does not fit
    + row("forward", 4, launch("warp_fwd_nchw_patch", I31), N=I31, H=8, W=8, C=32, w=8)
    # ---- forward, channel-last source
    + rows("forward", FD, launch("warp_fwd_cl", 2), layout=3)
    + rows("forward", FD, launch("warp_fwd_cl", 2), layout=7)
    + row("forward", 4, launch("warp_fwd_cl_nchw", 4), layout=2)                         # 2 x 32 tiles
    + row("forward", 4, launch("warp_fwd_cl_nchw", 4), layout=6)
    + row("forward", 8, "not_supported", layout=2)
    # whole 16-byte chunks per pixel: one short, whole, one over
    + sum((rows("forward", F, "not_supported", layout=lay, C=C) for lay in (2, 3) for C in (3, 6, 7, 9)), [])
    + sum((rows("forward", F, launch("warp_fwd_cl", 2), layout=3, C=C) for C in (4, 12)), [])
    + sum((rows("forward", D, "not_supported", layout=3, C=C) for C in (1, 3, 5)), [])
    + sum((rows("forward", D, launch("warp_fwd_cl", 2), layout=3, C=C) for C in (2, 4, 6)), [])
    + sum((rows("forward", FD, "not_supported", layout=lay, al=al) for lay in (2, 3) for al in ("011", "101", "001")), [])
    + rows("forward", FD, launch("warp_fwd_cl", 2), layout=3, al="110")
    # a view in 32-bit element offsets: h w C <= 2^31 - 1
    + rows("forward", FD, launch("warp_fwd_cl", 2), layout=3, C=4, w=1, h=I31 // 4)
    + rows("forward", FD, "not_supported", layout=3, C=4, w=1, h=I31 // 4 + 1)
    + row("forward", 4, launch("warp_fwd_cl_nchw", 4), layout=2, C=4, w=1, h=I31 // 4)
    + row("forward", 4, "not_supported", layout=2, C=4, w=1, h=I31 // 4 + 1)
    + rows("forward", FD, launch("warp_fwd_cl", I31), layout=3, N=I31, H=8, W=8)
    + rows("forward", FD, "invalid_value", layout=3, N=I31, H=8, W=9)
    + row("forward", 4, launch("warp_fwd_cl_nchw", I31), layout=2, N=I31, H=2, W=32)
    + row("forward", 4, "invalid_value", layout=2, N=I31, H=3, W=32)
    + row("forward", 4, "invalid_value", layout=2, N=I31, H=2, W=33)
    # ---- the order of the first checks
    + sum((rows("forward", FD, "invalid_value", **{k: -1}) for k in "NCHWhw"), [])
    + sum((rows("forward", FD, "invalid_value", **{k: 0}) for k in "hw"), [])
    + sum((rows("forward", FD, "invalid_value", layout=lay) for lay in (8, 11, -1)), [])
    + rows("forward", FD, "invalid_value", layout=8, H=0)                                # the layout before the empty call
    + sum((rows("forward", FD, "empty", **{k: 0}) for k in "NCHW"), [])
    + rows("forward", FD, "empty", H=0, ptrs="0000")                                     # the empty call before the pointers
    + rows("forward", FD, "empty", C=0, layout=3, al="000")
    + sum((rows("forward", FD, "invalid_value", ptrs=p) for p in ("0111", "1011", "1101")), [])
    + rows("forward", FD, launch("warp_fwd<NCHW>", 2), ptrs="1110")
    + rows("forward", FD, "invalid_value", layout=3, C=6, ptrs="0111")                   # the pointers before the chunks
    # ---- backward
    + rows("backward", FD, launch("warp_bwd<NCHW>", 2, 1))
    + rows("backward", FD, launch("warp_bwd<NHWC>", 2, 1), layout=1)
    + rows("backward", FD, launch("warp_bwd<NHWC>", 2, 1), layout=5)
    + rows("backward", FD, launch("warp_bwd<NCHW>", 2, 1), w=8, impl="gather", fwd="gather")
    + rows("backward", FD, launch("warp_bwd<NCHW>", I31, 1), N=I31, H=8, W=8, C=64)
    + rows("backward", FD, "invalid_value", N=I31, H=8, W=8, C=65)
    + rows("backward", FD, "not_supported", layout=2)                                    # NCHW destination: forward only
    + rows("backward", FD, "not_supported", layout=6)
    + row("backward", 4, gather(1, 1), layout=3)
    + row("backward", 8, gather(2, 1), layout=3)
    + row("backward", 4, gather(1, 1), layout=7)
    + row("backward", 4, gather(5, 1), layout=3, C=128)
    + row("backward", 4, gather(6, 1), layout=3, C=256)
    + row("backward", 4, gather(6, 2, grid=2048 + 5), layout=3, C=260)                   # 9 blocks x 2 channel groups in 5 workgroups
    + row("backward", 8, gather(6, 2, grid=2048 + 5), layout=3, C=130)
    + row("backward", 4, gather(0, 1), layout=3, C=4)
    # MVDETR_WARP_BWD_IMPL: `scatter` alone selects the atomic kernel
    + rows("backward", FD, launch("warp_bwd_cl", 2, 1), layout=3, impl="scatter")
    + rows("backward", FD, launch("warp_bwd_cl", 2, 1), layout=7, impl="scatter")
    + sum((row("backward", 4, gather(1, 1), layout=3, impl=word) for word in ("gather", "bogus", "Scatter", "clip")), [])
    # the other backward knobs: the plan's key and the gather's heavy workgroups, never the kernel
    + row("backward", 4, gather(1, 1, key=1), layout=3, geometry="clip")
    + row("backward", 4, gather(1, 1), layout=3, geometry="bogus")
    + row("backward", 4, gather(1, 1, key=256), layout=3, heavy="0")
    + row("backward", 4, gather(1, 1, key=129 * 256 + 1), layout=3, heavy="128", geometry="clip")
    + row("backward", 4, gather(1, 1, key=256), layout=3, heavy="bogus")                 # atoi: 0
    + row("backward", 4, gather(1, 1, grid=3 + 64), layout=3, heavy_wgs="64")
    + row("backward", 4, gather(1, 1, grid=3 + 1), layout=3, heavy_wgs="0")              # at least one
    + row("backward", 4, gather(1, 1, grid=3 + 1), layout=3, heavy_wgs="bogus")
    + row("backward", 4, launch("warp_bwd_cl", 2, 1, key=257), layout=3, impl="scatter", geometry="clip", heavy="0", heavy_wgs="64")
    # the same refusals as the forward
    + sum((rows("backward", F, "not_supported", layout=3, C=C) for C in (6, 9)), [])
    + sum((rows("backward", D, "not_supported", layout=3, C=C) for C in (1, 3)), [])
    + sum((rows("backward", FD, "not_supported", layout=3, al=al) for al in ("011", "101")), [])
    + rows("backward", FD, "not_supported", layout=3, C=4, w=1, h=I31 // 4 + 1)
    + rows("backward", FD, "invalid_value", layout=3, N=I31, H=8, W=9)
    # the gather's own limits: N H W C <= 2^31 - 1 and at most 2^31 - 1 light workgroups (4 (block, channel group) items each)
    + row("backward", 4, gather(0, 1, pb=plan_bytes(1, 5, 6, 1, I31 // 4), grid=2048 + 3), layout=3, C=4, H=1, W=I31 // 4)
    + row("backward", 4, launch("warp_bwd_cl", tiles(1, I31 // 4 + 1), 1), layout=3, C=4, H=1, W=I31 // 4 + 1)
    + row("backward", 4, gather(0, 1, pb=plan_bytes(127, 2, 2 ** 27, 1, 1), grid=2048 + 127 * 2 ** 24), layout=3, C=4, N=127, h=2, w=2 ** 27,
          H=1, W=1)
    + row("backward", 4, launch("warp_bwd_cl", 128, 1), layout=3, C=4, N=128, h=2, w=2 ** 27, H=1, W=1)
    + row("backward", 4, gather(6, 2, pb=plan_bytes(127, 2, 2 ** 17, 1, 1), grid=2048 + 127 * 2 ** 15), layout=3, C=260, N=127, h=2,
          w=2 ** 17, H=1, W=1)
    # the order of the first checks: an empty grad_src succeeds before anything is looked at, a missing one is refused before
    # the call can be empty, no destination pixels means zeros
    + rows("backward", FD, "none 0 0 0 0 0 0", C=0)
    + rows("backward", FD, "none 0 0 0 0 0 0", C=0, ptrs="0000")
    + rows("backward", FD, "none 0 0 0 0 0 0", N=0, H=0, layout=3, C=6)
    + rows("backward", FD, "zero_fill 0 0 0 0 0 0", H=0)
    + rows("backward", FD, "zero_fill 0 0 0 0 0 0", W=0, ptrs="0010", layout=3, C=6, al="000")
    + rows("backward", FD, "invalid_value", H=0, ptrs="1101")
    + rows("backward", FD, "invalid_value", ptrs="1101")
    + rows("backward", FD, "invalid_value", C=0, layout=8)
    + rows("backward", FD, "invalid_value", C=0, h=0)
    + sum((rows("backward", FD, "invalid_value", ptrs=p) for p in ("0111", "1011")), [])
    # ---- the 16-bit forward
    + sum((row("half", 2, launch("warp_fwd_half", 2), layout=lay) for lay in (0, 1, 2, 4, 5, 6)), [])
    + sum((row("half", 2, launch("warp_fwd_cl_half", 2), layout=lay) for lay in (3, 7)), [])
    + sum((row("half", 2, launch("warp_fwd_cl_half", 2), layout=3, C=C) for C in (16, 24)), [])
    + sum((row("half", 2, launch("warp_fwd_half", 2), layout=3, C=C) for C in (4, 7, 9, 12)), [])
    + sum((row("half", 2, launch("warp_fwd_half", 2), layout=3, al=al) for al in ("011", "101")), [])
    + row("half", 2, launch("warp_fwd_half", 6), layout=3, C=129)
    + row("half", 2, launch("warp_fwd_cl_half", 2), layout=3, w=1, h=I31 // 8)
    + row("half", 2, launch("warp_fwd_half", 2), layout=3, w=1, h=I31 // 8 + 1)
    + row("half", 2, launch("warp_fwd_half", 2), w=1, h=I31)                             # a texel offset is an int
    + row("half", 2, "invalid_value", w=2, h=2 ** 30)
    + row("half", 2, launch("warp_fwd_cl_half", I31), layout=3, N=I31, H=8, W=8)
    + row("half", 2, "invalid_value", layout=3, N=I31, H=8, W=9)                          # (not the other kernel)
    + row("half", 2, launch("warp_fwd_half", I31), N=I31, H=8, W=8, C=64)
    + row("half", 2, "invalid_value", N=I31, H=8, W=8, C=65)
    + sum((row("half", 2, "invalid_value", **{k: -1}) for k in "NCHWhw"), [])
    + sum((row("half", 2, "invalid_value", layout=lay) for lay in (8, -1)), [])
    + sum((row("half", 2, "empty", **{k: 0}) for k in "NCHW"), [])
    + row("half", 2, "empty", H=0, ptrs="0000", w=2, h=2 ** 30)
    + sum((row("half", 2, "invalid_value", ptrs=p) for p in ("0111", "1011", "1101")), [])
    + row("half", 2, launch("warp_fwd_half", 2), w=8, impl="scatter", fwd="gather")
    # ---- the two-step gradient: plan bytes, plan, planned
    + rows("plan_bytes", FD, f"plan 0 {{}} 1 {PB} 0 0")
    + rows("plan_bytes", FD, f"plan 0 {{}} 1 {PB} 0 0", ptrs="0000", al="000")
    + rows("plan", FD, f"plan 0 {{}} 1 {PB} 0 0")
    + rows("plan", FD, f"plan 0 {{}} 1 {PB} 0 0", ptrs="0101", al="001")
    + row("planned", 4, gather(1, 1, name="warp_bwd_gather[planned]"), layout=3)
    + row("planned", 8, gather(2, 1, name="warp_bwd_gather[planned]"), layout=7)
    + row("planned", 4, gather(1, 1, name="warp_bwd_gather[planned]"), layout=3, al="110")      # the plan's alignment is not looked at
    + row("planned", 4, gather(1, 1, name="warp_bwd_gather[planned]", grid=3 + 64, key=257), layout=3, heavy_wgs="64", heavy="0", geometry="clip")
    + sum((rows(e, FD, "not_supported", **{k: v}) for e in ("plan_bytes", "plan") for k in "NCHWhw" for v in (0, -1)), [])
    + sum((rows("planned", FD, "not_supported", layout=3, **{k: v}) for k in "NCHWhw" for v in (0, -1)), [])
    + sum((row(e, elem, "not_supported", layout=3) for e in ("plan_bytes", "plan", "planned") for elem in (2, 1, 0, 16, -4)), [])
    + sum((rows(e, FD, "not_supported", layout=3, impl="scatter") for e in ("plan_bytes", "plan", "planned")), [])
    + sum((rows(e, FD, f"plan 0 {{}} 1 {PB} 0 0", impl=word) for e in ("plan_bytes", "plan") for word in ("gather", "bogus")), [])
    + sum((rows(e, F, "not_supported", layout=3, C=6) for e in ("plan_bytes", "plan", "planned")), [])
    + sum((rows(e, D, "not_supported", layout=3, C=3) for e in ("plan_bytes", "plan", "planned")), [])
    + sum((rows(e, FD, "not_supported", layout=3, C=4, w=1, h=I31 // 4 + 1) for e in ("plan_bytes", "plan", "planned")), [])
    + row("plan_bytes", 4, f"plan 0 0 1 {plan_bytes(1, I31 // 4, 1, 7, 9)} 0 0", C=4, w=1, h=I31 // 4)
    + sum((rows(e, FD, "not_supported", layout=3, C=4, H=1, W=I31 // 4 + 1) for e in ("plan_bytes", "plan", "planned")), [])
    + row("plan_bytes", 4, f"plan 0 0 1 {plan_bytes(1, 5, 6, 1, I31 // 4)} 0 0", C=4, H=1, W=I31 // 4)
    + sum((rows(e, F, "not_supported", layout=3, C=4, N=128, h=2, w=2 ** 27, H=1, W=1) for e in ("plan_bytes", "plan", "planned")), [])
    + row("plan_bytes", 4, f"plan 0 0 1 {plan_bytes(127, 2, 2 ** 27, 1, 1)} 0 0", C=4, N=127, h=2, w=2 ** 27, H=1, W=1)
    + sum((rows("plan", FD, "invalid_value", ptrs=p) for p in ("1011", "1110", "0010")), [])
    + rows("plan", FD, "invalid_value", al="110")                                        # a misaligned plan
    + rows("plan", FD, "invalid_value", al="110", N=0)                                   # the pointers first
    + sum((rows("planned", FD, "invalid_value", layout=lay) for lay in (0, 1, 2, 4, 5, 6, 8, 11, -1)), [])
    + sum((rows("planned", FD, "invalid_value", layout=3, ptrs=p) for p in ("0111", "1011", "1101", "1110")), [])
    + rows("planned", FD, "invalid_value", layout=3, ptrs="0111", N=0)
    + sum((rows("planned", FD, "not_supported", layout=3, al=al) for al in ("011", "101")), [])
)
# (lgG depends on the element size where a row serves both: 8 channels are 2 chunks of fp32, 4 of fp64)
ROWS = tuple((args, want.format(1 if args[1] == 4 else 2)) for args, want in ROWS)


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("warp_route")
    src, exe = tmp / "route.cpp", tmp / "route"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = "".join(" ".join(str(x) for x in args) + "\n" for args, _ in ROWS)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(ROWS)
    return out


def test_every_row_of_the_route_table(routes):
    bad = [(args, want, got) for (args, want), got in zip(ROWS, routes) if got != want]
    assert not bad, "\n".join(f"{a}: want {w!r}, got {g!r}" for a, w, g in bad)


def test_every_kind_and_status_is_reached(routes):
    names = {g.split()[0] for g in routes}
    assert names >= {"warp_fwd<NCHW>", "warp_fwd<NHWC>", "warp_fwd_nchw_patch", "warp_fwd_cl", "warp_fwd_cl_nchw", "warp_fwd_half",
                     "warp_fwd_cl_half", "warp_bwd<NCHW>", "warp_bwd<NHWC>", "warp_bwd_cl", "warp_bwd_gather", "warp_bwd_gather[planned]",
                     "plan", "zero_fill", "none", "empty", "invalid_value", "not_supported"}


def test_unknown_and_unset_knobs_agree(routes):
    """A typo in a knob selects nothing: every row with `bogus` for MVDETR_WARP_BWD_IMPL, _BWD_GEOMETRY or MVDETR_WARP_FWD_NCHW has
    the route of the same call with the knob unset."""
    got = {args: g for (args, _), g in zip(ROWS, routes)}
    pairs = []
    for a in got:
        for pos in (16, 17, 20):
            if a[pos] == "bogus":
                pairs.append((a, a[:pos] + ("-",) + a[pos + 1:]))
    assert len(pairs) >= 6 and all(u in got and got[b] == got[u] for b, u in pairs)
