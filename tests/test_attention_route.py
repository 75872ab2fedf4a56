"""The fused attention's route table (csrc/attention_route.h), checked without a GPU and without loading the library: the
header is plain C++, so a small stand-alone program compiled with g++ prints the route of every row below and the test compares
it with the route written next to the row.  The rows are the dispatch of every C ABI entry of the operator -- fp32 / fp64 forward
and backward, the 16-bit forward -- with every limit at which a call changes kernel, instantiation or grid, or is refused, from
both sides.

A printed route is `<name> <D> <drop> <tile> <dq> <grid> <grid kv> <grid delta>`: the name mvdetr_attention_last_kernel reports
from the call on; the MFMA kernels' head-dimension instantiation (0: a generic kernel); the dropout instantiation; the queries
per workgroup of the MFMA forwards; whether the backward has queries (attn_delta and the dQ kernel run); the workgroups x,y,z of
the forward or dQ kernel, of the dK / dV kernel, and those of attn_delta.  A refused or empty call prints its status alone; the
C ABI turns `empty` into 0, `invalid_value` into 1, `not_supported` into 801.

Oddities the table pins as they are: no key or no channel is invalid_value in the fp32 / fp64 entries and not_supported in the
16-bit one, which also says not_supported before it says empty or looks at a pointer; a dropout probability below 2^-32 drops
nothing and takes the kernels without dropout; a backward without queries runs the generic dK / dV kernel alone (zeros), reports
attn_bwd_generic and still refuses a head dimension above 256."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvdetr_amd", "csrc")

PROGRAM = r"""
#include "attention_route.h"
#include <stdio.h>
#include <string.h>
using namespace mvdetr;
int main()
{
    char entry[16];
    int elem, B, H, Sq, Sk, D, tile, f[13];
    double p;
    for (;;) {
        if (scanf("%15s %d %d %d %d %d %d %lf %d", entry, &elem, &B, &H, &Sq, &Sk, &D, &p, &tile) != 9) break;
        for (int i = 0; i < 13; ++i) if (scanf("%d", f + i) != 1) return 1;
        static const char *const entries[] = {"forward", "backward", "half"};
        int e = 0;
        while (strcmp(entry, entries[e])) ++e;
        const AttnRoute r = attn_route(AttnQuery{(AttnEntry)e, elem, B, H, Sq, Sk, D, p, tile, f[0] != 0, f[1] != 0, f[2] != 0, f[3] != 0,
                                                 f[4] != 0, f[5] != 0, f[6] != 0, f[7] != 0, f[8] != 0, f[9] != 0, f[10] != 0, f[11] != 0,
                                                 f[12] != 0});
        static const char *const status[] = {"ok", "empty", "invalid_value", "not_supported"};
        if (r.status != AttnStatus::ok) printf("%s\n", status[(int)r.status]);
        else printf("%s %d %d %d %d %u,%u,%u %u,%u,%u %u\n", r.name, r.D, r.drop, r.tile, r.with_dq, r.grid.x, r.grid.y, r.grid.z,
                    r.grid_kv.x, r.grid_kv.y, r.grid_kv.z, r.grid_delta);
    }
    return 0;
}
"""

CAP = 1 << 20           # workgroups of the grid-stride kernels


def row(entry, elem, want, *, B=1, H=2, Sq=70, Sk=65, D=16, p=0.0, tile=0, strides="11", ptrs="1111111111", al=1):
    """One query.  strides: the pointer is non-null, every stride is a multiple of 4 (16-bit: 8); ptrs: q, k, v, out, lse, grad_out,
    workspace, grad_q, grad_k, grad_v non-null; al: every pointer the entry looks at is 16-byte aligned."""
    args = (entry, elem, B, H, Sq, Sk, D, p, tile) + tuple(int(c) for c in strides + ptrs) + (al,)
    return [(args, want)]


def rows(entry, elems, want, **kw):
    return sum((row(entry, e, want, **kw) for e in elems), [])


def fwd(name, D=0, tile=0, grid=(35, 1, 1), drop=0):
    return f"{name} {D} {drop} {tile} 0 {grid[0]},{grid[1]},{grid[2]} 1,1,1 0"


def bwd(name, D=0, tile=0, grid=(35, 1, 1), kv=(33, 1, 1), delta=1, drop=0, dq=1):
    return f"{name} {D} {drop} {tile} {dq} {grid[0]},{grid[1]},{grid[2]} {kv[0]},{kv[1]},{kv[2]} {delta}"


F, D8 = (4,), (8,)
FD = (4, 8)
MFMA, GEN, HALF = "attn_fwd_mfma", "attn_fwd_generic", "attn_fwd_mfma_half"
BWD, BGEN = "attn_bwd_mfma", "attn_bwd_generic"
T1 = (1, 2, 1)          # one tile of queries (or keys) x 2 heads x 1 batch: the default shapes' MFMA grid

ROWS = (
    # ---- forward: fp32, D 16 or 32, aligned pointers, strides in float4s, batch and heads that fit a grid take the MFMA kernel;
    # everything else the generic one, one workgroup per 4 of the 140 rows
    row("forward", 4, fwd(MFMA, 16, 128, T1))
    + row("forward", 4, fwd(MFMA, 32, 128, T1), D=32)
    + sum((row("forward", 4, fwd(GEN), D=D) for D in (1, 15, 17, 31, 33, 64, 256)), [])
    + sum((row("forward", 8, fwd(GEN), D=D) for D in (1, 16, 17, 32, 33, 256)), [])
    + rows("forward", FD, "invalid_value", D=257)
    + rows("forward", FD, "invalid_value", D=0)
    + rows("forward", FD, fwd(GEN), al=0)
    + rows("forward", FD, fwd(GEN), strides="10")
    + row("forward", 4, fwd(MFMA, 16, 128, (1, 65535, 1)), H=65535, Sq=1)
    + rows("forward", FD, fwd(GEN, grid=(16384, 1, 1)), H=65536, Sq=1)
    + row("forward", 4, fwd(MFMA, 16, 128, (1, 1, 65535)), B=65535, H=1, Sq=1)
    + rows("forward", FD, fwd(GEN, grid=(16384, 1, 1)), B=65536, H=1, Sq=1)
    + row("forward", 4, fwd(MFMA, 16, 128, T1), Sq=128)                                  # 128 queries per workgroup
    + row("forward", 4, fwd(MFMA, 16, 128, (2, 2, 1)), Sq=129)
    + row("forward", 4, fwd(MFMA, 16, 128, T1), Sk=1)
    # dropout: the instantiation follows the 32-bit threshold, not the probability
    + row("forward", 4, fwd(MFMA, 16, 128, T1, drop=1), p=0.5)
    + rows("forward", FD, fwd(GEN, drop=1), p=0.5, D=17)
    + rows("forward", FD, fwd(GEN, drop=0), p=2e-10, D=17)                               # 0.86 / 2^32: nothing is dropped
    + rows("forward", FD, fwd(GEN, drop=1), p=3e-10, D=17)                               # 1.29 / 2^32
    + sum((rows("forward", FD, "invalid_value", p=p) for p in (-0.1, 1.0, "nan")), [])
    # the generic grid: a workgroup per 4 rows, at most 2^20
    + rows("forward", D8, fwd(GEN, grid=(CAP - 256, 1, 1)), H=4095, Sq=1024)
    + rows("forward", D8, fwd(GEN, grid=(CAP, 1, 1)), H=4096, Sq=1024)
    + rows("forward", D8, fwd(GEN, grid=(CAP, 1, 1)), H=4096, Sq=1025)
    # the order: the arguments, the empty call, the pointers, D beyond the generic kernels
    + sum((rows("forward", FD, "invalid_value", **{k: -1}) for k in ("B", "H", "Sq", "Sk", "D")), [])
    + rows("forward", FD, "invalid_value", Sk=0)                                         # (the 16-bit entry: not_supported)
    + rows("forward", FD, "invalid_value", strides="01")
    + rows("forward", FD, "invalid_value", strides="01", Sq=0)
    + sum((rows("forward", FD, "empty", **{k: 0}) for k in ("B", "H", "Sq")), [])
    + rows("forward", FD, "empty", Sq=0, ptrs="0000000000", al=0, D=257)
    + sum((rows("forward", FD, "invalid_value", ptrs=p) for p in ("0111111111", "1011111111", "1101111111", "1110111111", "1111011111")), [])
    + row("forward", 4, fwd(MFMA, 16, 128, T1), ptrs="1111100000")
    # ---- backward: attn_delta, then the MFMA pair under the forward's conditions (strides of all 8 tensors, 7 pointers), else the
    # generic pair (65 keys x 2 heads: 33 workgroups)
    + row("backward", 4, bwd(BWD, 16, 128, T1, T1))
    + row("backward", 4, bwd(BWD, 32, 128, T1, T1, drop=1), D=32, p=0.25)
    + row("backward", 8, bwd(BGEN))
    + sum((rows("backward", FD, bwd(BGEN), D=D) for D in (1, 17, 33, 256)), [])
    + rows("backward", FD, "invalid_value", D=257)
    + rows("backward", FD, bwd(BGEN), al=0)
    + rows("backward", FD, bwd(BGEN, drop=1), strides="10", p=0.5)
    + row("backward", 4, bwd(BWD, 16, 128, (1, 65535, 1), (1, 65535, 1), delta=256), H=65535, Sq=1, Sk=1)
    + rows("backward", FD, bwd(BGEN, grid=(16384, 1, 1), kv=(16384, 1, 1), delta=256), H=65536, Sq=1, Sk=1)
    + row("backward", 4, bwd(BWD, 16, 128, (1, 2, 1), (1, 2, 1)), Sq=128, Sk=128)
    + row("backward", 4, bwd(BWD, 16, 128, (2, 2, 1), (2, 2, 1), delta=2), Sq=129, Sk=129)       # 258 rows: 2 workgroups of attn_delta
    + rows("backward", D8, bwd(BGEN, grid=(CAP, 1, 1), kv=(CAP, 1, 1), delta=CAP), B=64, H=4096, Sq=1024, Sk=1024)    # 2^28 rows
    + rows("backward", D8, bwd(BGEN, grid=(CAP, 1, 1), kv=(CAP, 1, 1), delta=CAP - 256), B=64, H=4095, Sq=1024, Sk=1024)
    # no queries: the dK / dV generic kernel alone writes zeros; no batch or no head: nothing
    + rows("backward", FD, bwd(BGEN, grid=(0, 1, 1), delta=0, dq=0), Sq=0)
    + rows("backward", FD, bwd(BGEN, grid=(0, 1, 1), delta=0, dq=0), Sq=0, ptrs="0110000011")
    + rows("backward", FD, "invalid_value", Sq=0, D=257)
    + sum((rows("backward", FD, "invalid_value", Sq=0, ptrs=p) for p in ("1011111111", "1101111111", "1111111101", "1111111110")), [])
    + sum((rows("backward", FD, "empty", **{k: 0}) for k in ("B", "H")), [])
    + rows("backward", FD, "empty", H=0, ptrs="0000000000", D=257)
    + rows("backward", FD, "invalid_value", H=0, Sk=0)
    + sum((rows("backward", FD, "invalid_value", ptrs="".join("0" if i == j else "1" for j in range(10))) for i in range(10)), [])
    + sum((rows("backward", FD, "invalid_value", **{k: -1}) for k in ("B", "H", "Sq", "Sk", "D")), [])
    + rows("backward", FD, "invalid_value", strides="01")
    + sum((rows("backward", FD, "invalid_value", p=p) for p in (-0.1, 1.0, "nan")), [])
    # ---- the 16-bit forward: 128 queries per workgroup unless one 64-query workgroup holds them all, or the tile is forced
    + row("half", 2, fwd(HALF, 16, 128, T1))
    + row("half", 2, fwd(HALF, 32, 128, T1), D=32)
    + row("half", 2, fwd(HALF, 16, 64, T1), Sq=64)
    + row("half", 2, fwd(HALF, 16, 128, T1), Sq=65)
    + row("half", 2, fwd(HALF, 16, 128, (2, 2, 1)), Sq=129)
    + row("half", 2, fwd(HALF, 16, 64, (2, 2, 1)), Sq=65, tile=64)
    + row("half", 2, fwd(HALF, 16, 64, (3, 2, 1)), Sq=129, tile=64)
    + row("half", 2, fwd(HALF, 16, 128, T1), Sq=64, tile=128)
    + row("half", 2, fwd(HALF, 16, 64, (1, 65535, 65535)), B=65535, H=65535, Sq=1)
    + row("half", 2, fwd(HALF, 16, 128, T1), ptrs="1111000000")
    + row("half", 2, fwd(HALF, 16, 128, T1), p=0.5)                                      # (the entry has no dropout: not looked at)
    # the order of its refusals: invalid_value, not_supported, empty, the pointers, the alignment
    + sum((row("half", 2, "invalid_value", **{k: -1}) for k in ("B", "H", "Sq")), [])
    + row("half", 2, "invalid_value", strides="01")
    + row("half", 2, "invalid_value", strides="01", D=17)
    + sum((row("half", 2, "not_supported", D=D) for D in (-1, 0, 1, 15, 17, 31, 33, 64, 256, 257)), [])
    + sum((row("half", 2, "not_supported", Sk=Sk) for Sk in (0, -1)), [])
    + row("half", 2, "not_supported", H=65536)
    + row("half", 2, "not_supported", B=65536)
    + row("half", 2, "not_supported", strides="10")
    + row("half", 2, "not_supported", D=17, Sq=0)
    + row("half", 2, "not_supported", strides="10", Sq=0, ptrs="0000000000")
    + sum((row("half", 2, "empty", **{k: 0}) for k in ("B", "H", "Sq")), [])
    + row("half", 2, "empty", Sq=0, ptrs="0000000000", al=0)
    + sum((row("half", 2, "invalid_value", ptrs=p) for p in ("0111000000", "1011000000", "1101000000", "1110000000")), [])
    + row("half", 2, "invalid_value", ptrs="0111000000", al=0)
    + row("half", 2, "not_supported", al=0)
)


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("attention_route")
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
    assert {g.split()[0] for g in routes} >= {MFMA, GEN, HALF, BWD, BGEN, "empty", "invalid_value", "not_supported"}
