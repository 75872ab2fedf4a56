"""The deformable convolution's route table (csrc/deform_conv_route.h), checked without a GPU and without loading the library:
the header is plain C++, so a small stand-alone program compiled with g++ prints the route of every row below and the test
compares it with the route written next to the row.  The rows are the dispatch of every C ABI entry of the operator -- fp32 /
fp64 forward and backward, the 16-bit forward -- with every limit at which a call changes kernel, grid or zero-fill, or is
refused, from both sides.

A printed route is `<name> <KC> <grid 0> <grid 1> <zero flags> <pps>`: the name mvdetr_deform_conv2d_last_kernel reports from the
call on (`zero_fill` for the backward that only zeroes its outputs and leaves the name alone); the input channels per K chunk of
the MFMA forwards; the workgroups x,y,z of the launches in order; whether grad_offset and grad_weight are zeroed first; the pixels
per range of dc_bwd_weight_mfma.  A refused or empty call prints its status alone; the C ABI turns `empty` into 0,
`invalid_value` into 1, `not_supported` into 801.

Oddities the table pins as they are: the 16-bit entry looks at its pointers before it says not_supported and at
out_batch_stride after; the fp32 / fp64 forward is empty before it looks at a pointer and takes a null input / weight when there
are no input channels; only the MFMA forwards' grid is checked (new with the table: 65535 blocks of 128 output channels)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvdetr_amd", "csrc")

PROGRAM = r"""
#include "deform_conv_route.h"
#include <stdio.h>
#include <string.h>
using namespace mvdetr;
int main()
{
    char entry[16];
    int elem, s[14], nhwc, f[11];
    long long obs;
    for (;;) {
        if (scanf("%15s %d", entry, &elem) != 2) break;
        for (int i = 0; i < 14; ++i) if (scanf("%d", s + i) != 1) return 1;
        if (scanf("%d %lld", &nhwc, &obs) != 2) return 1;
        for (int i = 0; i < 11; ++i) if (scanf("%d", f + i) != 1) return 1;
        static const char *const entries[] = {"forward", "backward", "half"};
        int e = 0;
        while (strcmp(entry, entries[e])) ++e;
        const DcRoute r = dc_route(DcQuery{(DcEntry)e, elem, s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], s[9], s[10], s[11], s[12],
                                           s[13], nhwc, obs, f[0] != 0, f[1] != 0, f[2] != 0, f[3] != 0, f[4] != 0, f[5] != 0, f[6] != 0,
                                           f[7] != 0, f[8] != 0, f[9] != 0, f[10] != 0});
        static const char *const status[] = {"ok", "empty", "invalid_value", "not_supported"};
        if (r.status != DcStatus::ok) printf("%s\n", status[(int)r.status]);
        else printf("%s %d %u,%u,%u %u,%u,%u %d%d %lld\n", r.name ? r.name : "zero_fill", r.KC, r.grid[0].x, r.grid[0].y, r.grid[0].z,
                    r.grid[1].x, r.grid[1].y, r.grid[1].z, r.zero_goff, r.zero_gw, (long long)r.pps);
    }
    return 0;
}
"""

I31 = 2 ** 31 - 1
ENTRIES = ("forward", "backward", "half")
SHAPE = ("B", "C", "H", "W", "Co", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw", "G")
DEFAULT = dict(B=1, C=16, H=5, W=6, Co=32, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, G=1)      # 5 x 6 output: 30 pixels
K1 = dict(kh=1, kw=1, ph=0, pw=0)                                                                       # a 1 x 1 kernel


def row(entry, elem, want, *, nhwc=1, obs=0, ptrs="11111111", al="111", **shape):
    """One query.  obs: out_batch_stride minus its floor C_out H_out W_out; ptrs: input, offset, weight, out, grad_out, grad_input,
    grad_offset, grad_weight non-null; al: input, weight 16-byte aligned, the 16-bit entry's other pointers 2-byte aligned."""
    assert not set(shape) - set(SHAPE)
    s = dict(DEFAULT, **shape)
    out = [max((s[n] + 2 * s["p" + a] - s["d" + a] * (s["k" + a] - 1) - 1) // max(s["s" + a], 1) + 1, 0) for n, a in (("H", "h"), ("W", "w"))]
    args = (entry, elem) + tuple(s[k] for k in SHAPE) + (nhwc, max(s["Co"], 0) * out[0] * out[1] + obs) + tuple(int(c) for c in ptrs + al)
    return [(args, want)]


def rows(entry, elems, want, **kw):
    return sum((row(entry, e, want, **kw) for e in elems), [])


def ok(name, KC, g0=(1, 1, 1), g1=(1, 1, 1), zero="00", pps=0):
    return f"{name} {KC} {g0[0]},{g0[1]},{g0[2]} {g1[0]},{g1[1]},{g1[2]} {zero} {pps}"


F, D = (4,), (8,)
FD = (4, 8)
MFMA, GEN, HALF = "dc_fwd_mfma", "dc_fwd_generic", "dc_fwd_mfma_half"
BWD, BGEN = "dc_bwd_mfma", "dc_bwd_generic"

ROWS = (
    # ---- forward: fp32, channel-last, one offset group, C % 16 == 0, C_out % 32 == 0, aligned input take the MFMA kernel
    row("forward", 4, ok(MFMA, 16))
    + row("forward", 8, ok(GEN, 16, (4, 1, 1)))                                          # fp64 never does; 30 x 32 outputs / 256
    + rows("forward", FD, ok(GEN, 16, (4, 1, 1)), nhwc=0)
    + rows("forward", FD, ok(GEN, 16, (4, 1, 1)), G=2)
    + rows("forward", FD, ok(GEN, 16, (4, 1, 1)), al="011")                              # a misaligned input
    + row("forward", 4, ok(MFMA, 16), al="100")                                          # (nothing else is looked at)
    + rows("forward", FD, ok(GEN, 32, (4, 1, 1)), C=0)                                   # no input channels: bias alone
    + rows("forward", FD, ok(GEN, 16, (4, 1, 1)), C=8)
    + rows("forward", FD, ok(GEN, 16, (4, 1, 1)), C=24)
    + row("forward", 4, ok(MFMA, 32), C=32)
    + row("forward", 4, ok(MFMA, 16), C=48)
    + row("forward", 8, ok(GEN, 32, (4, 1, 1)), C=32)
    + rows("forward", FD, "empty", Co=0)
    + rows("forward", FD, ok(GEN, 16, (2, 1, 1)), Co=16)
    + rows("forward", FD, ok(GEN, 16, (4, 1, 1)), Co=33)
    + row("forward", 4, ok(MFMA, 16), Co=128)
    + row("forward", 4, ok(MFMA, 16, (1, 2, 1)), Co=160)                                 # 128 output channels per workgroup
    + row("forward", 4, ok(MFMA, 16), H=8, W=8)                                          # 64 pixels per workgroup
    + row("forward", 4, ok(MFMA, 16, (2, 1, 1)), H=5, W=13)                              # 65
    + row("forward", 4, ok(MFMA, 16), B=2)                                               # pixels run across the batch: 60
    + row("forward", 4, ok(MFMA, 16, (2, 1, 1)), B=3)                                    # 90
    + rows("forward", FD, ok(GEN, 16, (1 << 20, 1, 1)), nhwc=0, B=1 << 18, Co=1 << 10, H=1, W=1, **K1)      # 2^28 outputs: capped
    # the MFMA grid: 65535 blocks of output channels (beyond: refused, where the launch used to fail)
    + row("forward", 4, ok(MFMA, 16, (1, 65535, 1)), Co=65535 * 128, H=1, W=1, **K1)
    + row("forward", 4, "not_supported", Co=65535 * 128 + 32, H=1, W=1, **K1)
    + row("forward", 8, ok(GEN, 16, (32768, 1, 1)), Co=65535 * 128 + 32, H=1, W=1, **K1)
    + row("forward", 4, "invalid_value", Co=65535 * 128 + 32, H=1, W=1, ptrs="11101111", **K1)     # the pointers first
    # ---- the order of the first checks: the shape, the empty call, the pointers
    + sum((rows(e, (elem,), "invalid_value", **{k: -1}) for e, elem in (("forward", 4), ("forward", 8), ("backward", 4), ("half", 2))
           for k in ("B", "C", "Co", "ph", "pw")), [])
    + sum((rows(e, (elem,), "invalid_value", **{k: 0}) for e, elem in (("forward", 4), ("forward", 8), ("backward", 4), ("half", 2))
           for k in ("H", "W", "kh", "kw", "sh", "sw", "dh", "dw", "G")), [])
    + sum((rows(e, (elem,), "invalid_value", G=3) for e, elem in (("forward", 4), ("backward", 8), ("half", 2))), [])     # 16 % 3
    + rows("forward", FD, ok(GEN, 16), nhwc=0, H=2, kh=4)                               # the taps just cover the padded rows
    + sum((rows(e, (elem,), "invalid_value", H=2, kh=5) for e, elem in (("forward", 4), ("backward", 4), ("half", 2))), [])
    + sum((rows(e, (elem,), "invalid_value", W=2, kw=3, dw=2) for e, elem in (("forward", 4), ("backward", 4), ("half", 2))), [])
    # the three products that must stay below 2^31: the input, the output, the offsets
    + rows("forward", FD, ok(GEN, 16, (1, 1, 1)), nhwc=0, C=I31, H=1, W=1, Co=1, **K1)
    + rows("forward", FD, "invalid_value", nhwc=0, B=2, C=1 << 30, H=1, W=1, Co=1, **K1)
    + rows("forward", FD, ok(GEN, 16, (1 << 20, 1, 1)), nhwc=0, C=1, H=1, W=1, Co=I31, **K1)
    + rows("forward", FD, "invalid_value", nhwc=0, B=2, C=1, H=1, W=1, Co=1 << 30, **K1)
    + rows("forward", FD, ok(GEN, 16, (1 << 20, 1, 1)), nhwc=0, B=(1 << 30) - 1, C=1, H=1, W=1, Co=1, **K1)
    + rows("forward", FD, "invalid_value", nhwc=0, B=1 << 30, C=1, H=1, W=1, Co=1, **K1)
    + rows("backward", FD, "invalid_value", B=1 << 30, C=1, H=1, W=1, Co=1, **K1)
    + row("half", 2, "invalid_value", B=2, C=1 << 30, H=1, W=1, **K1)
    + rows("forward", FD, "empty", B=0)
    + rows("forward", FD, "empty", B=0, ptrs="00000000", al="000")                       # the empty call before the pointers
    + rows("forward", FD, "empty", Co=0, ptrs="00000000")
    + rows("forward", FD, "invalid_value", B=0, H=0)                                     # the shape before the empty call
    + sum((rows("forward", FD, "invalid_value", ptrs=p) for p in ("01111111", "10111111", "11011111", "11101111")), [])
    + rows("forward", FD, ok(GEN, 32, (4, 1, 1)), C=0, ptrs="01010000")                  # no channels: input and weight may be null
    + row("forward", 4, ok(MFMA, 16), ptrs="11110000")
    # ---- backward
    + row("backward", 4, ok(BWD, 16, (1, 1, 9), (9, 1, 1), pps=32))
    + row("backward", 8, ok(BGEN, 16, (2, 1, 1), (144, 1, 1)))                           # 30 x 9 (pixel, tap) lanes; 16 x 9 rows of grad_W
    + rows("backward", FD, ok(BGEN, 16, (2, 1, 1), (144, 1, 1)), nhwc=0)
    + rows("backward", FD, ok(BGEN, 16, (3, 1, 1), (144, 1, 1)), G=2)
    + rows("backward", FD, ok(BGEN, 16, (2, 1, 1), (144, 1, 1)), al="011")
    + rows("backward", FD, ok(BGEN, 16, (2, 1, 1), (216, 1, 1)), C=24)
    + rows("backward", FD, ok(BGEN, 16, (2, 1, 1), (144, 1, 1)), Co=33)
    + rows("backward", FD, ok(BGEN, 16, (2, 1, 1), (144, 2, 1)), Co=257)                 # 256 output channels per workgroup
    # one block of 128 input channels writes grad_offset, more add into it: zeroed first
    + row("backward", 4, ok(BWD, 32, (1, 1, 9), (36, 1, 1), pps=32), C=128)
    + row("backward", 4, ok(BWD, 16, (1, 2, 9), (45, 1, 1), "10", 32), C=144)
    + row("backward", 4, ok(BWD, 16, (2, 1, 9), (9, 2, 3), "01", 32), H=5, W=13, Co=160)
    # the pixel ranges of grad_weight: one 32-pixel chunk writes, more ranges add into it: zeroed first
    + row("backward", 4, ok(BWD, 16, (1, 1, 9), (9, 1, 1), pps=32), H=4, W=8)            # 32 pixels
    + row("backward", 4, ok(BWD, 16, (1, 1, 9), (9, 1, 2), "01", 32), H=3, W=11)         # 33
    + row("backward", 4, ok(BWD, 16, (4, 1, 9), (9, 1, 8), "01", 32), B=8)               # 240 pixels in 8 chunks, 9 K blocks
    # ranges until ~2048 workgroups: 2047 K blocks (23 x 89) take two, 2048 (32 x 64) one
    + row("backward", 4, ok(BWD, 32, (1, 6, 1), (23, 89, 2), "11", 32), B=2, C=736, Co=11392, **K1)
    + row("backward", 4, ok(BWD, 32, (1, 8, 1), (32, 64, 1), "10", 64), B=2, C=1024, Co=8192, **K1)
    + row("backward", 4, ok(BWD, 16, (1, 1, 1), (1, 65536, 1), pps=32), Co=65536 * 128, H=1, W=1, **K1)    # (its grids are not checked)
    # nothing flows: the written outputs are zeroed, the name stays
    + rows("backward", FD, ok("zero_fill", 16, zero="01"), B=0)
    + rows("backward", FD, ok("zero_fill", 16, zero="10"), Co=0)
    + rows("backward", FD, ok("zero_fill", 32, zero="10"), C=0)
    + rows("backward", FD, ok("zero_fill", 16, zero="00"), B=0, Co=0)
    + rows("backward", FD, ok("zero_fill", 16, zero="01"), B=0, ptrs="00000001", al="000")
    + rows("backward", FD, ok("zero_fill", 16, zero="10"), Co=0, ptrs="00000010")
    + rows("backward", FD, ok("zero_fill", 16, zero="00"), B=0, Co=0, ptrs="00000000")
    + rows("backward", FD, "invalid_value", B=0, ptrs="11111110")
    + rows("backward", FD, "invalid_value", Co=0, ptrs="11111101")
    + sum((rows("backward", FD, "invalid_value", ptrs=p) for p in ("01111111", "10111111", "11011111", "11110111", "11111011", "11111101",
                                                                   "11111110")), [])
    + row("backward", 4, ok(BWD, 16, (1, 1, 9), (9, 1, 1), pps=32), ptrs="11101111")     # (`out` is the forward's)
    # ---- the 16-bit forward
    + row("half", 2, ok(HALF, 16))
    + row("half", 2, ok(HALF, 32), C=32)
    + row("half", 2, ok(HALF, 16), C=48)
    + row("half", 2, ok(HALF, 16, (2, 2, 1)), H=5, W=13, Co=160)
    + row("half", 2, ok(HALF, 16), obs=7)                                                # a channel slice of a larger tensor
    + row("half", 2, "invalid_value", obs=-1)
    + row("half", 2, ok(HALF, 32, (1, 512, 1)), C=1 << 15, Co=(1 << 16) - 32, H=1, W=1, **K1)
    + row("half", 2, "invalid_value", C=1 << 15, Co=1 << 16, H=1, W=1, **K1)             # the permuted weight: 2^31 elements
    + row("half", 2, ok(HALF, 16, (1, 65535, 1)), Co=65535 * 128, H=1, W=1, **K1)
    + row("half", 2, "not_supported", Co=65535 * 128 + 32, H=1, W=1, **K1)
    # not_supported, one condition at a time
    + row("half", 2, "not_supported", G=2)
    + row("half", 2, "not_supported", nhwc=0)
    + sum((row("half", 2, "not_supported", C=C) for C in (0, 8, 24)), [])
    + sum((row("half", 2, "not_supported", Co=Co) for Co in (0, 16, 33, 48)), [])
    + sum((row("half", 2, "not_supported", al=al) for al in ("011", "101", "110")), [])
    # the order: the shape, the pointers, not_supported, out_batch_stride, the empty call
    + sum((row("half", 2, "invalid_value", ptrs=p) for p in ("01111111", "10111111", "11011111", "11101111")), [])
    + row("half", 2, ok(HALF, 16), ptrs="11110000")
    + row("half", 2, "invalid_value", G=2, ptrs="01111111")
    + row("half", 2, "not_supported", G=2, obs=-1)
    + row("half", 2, "not_supported", B=0, C=24)
    + row("half", 2, "not_supported", B=0, al="011")
    + row("half", 2, "invalid_value", B=0, ptrs="11101111")
    + row("half", 2, "invalid_value", B=0, obs=-1)
    + row("half", 2, "empty", B=0)
)


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("deform_conv_route")
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
    assert {g.split()[0] for g in routes} >= {MFMA, GEN, HALF, BWD, BGEN, "zero_fill", "empty", "invalid_value", "not_supported"}
