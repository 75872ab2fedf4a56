"""The MSDA forward's route table (csrc/msda_forward_route.h), checked without a GPU and without loading the library: the
header is plain C++, so a small stand-alone program compiled with g++ prints the route of every row below and the test
compares it with the route written next to the row.  The rows are the dispatch of the public fp32 / fp64 entries, the fused
inference entry and the fused training entry, with every limit at which a call changes route or is refused.

A printed route is `<name> <probe> <standdown> <stats_pass> <ref_mode> <gather_vec>`: the route's name (msda_forward_route_name);
whether msda_locality_probe runs in front of the kernel; whether a camera-grouped launch carries GROUP_OPT_STANDDOWN; whether
msda_softmax_stats follows the kernel; the launchers' `fused` template argument (0 public contract, 1 a reference point per
(query, level, point), 2 one per (query, level)); and msda_fwd_gather's channels per lane.  A refused or empty call prints its
status alone.

Oddities the table pins as they are (the refactor that introduced it changed no behaviour): the fused entries have no `empty`
status -- B = 0 is not_supported, S = Lq = 0 launches over nothing; MVDETR_MSDA_FWD_IMPL does not reach the fused entries; a
forced `tile` means "no gather kernel, no probe", the camera-grouped kernels still take the calls they take under `auto`."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvdetr_amd", "csrc")

PROGRAM = r"""
#include "msda_forward_route.h"
#include <stdio.h>
using namespace mvdetr;
int main()
{
    char entry[16], knob[32];
    int B, S, M, D, L, Lq, P, layout, qs_l, qs_w, ql0, ql1, follow, all16, a16, group, stats;
    while (scanf("%15s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %31s %d %d", entry, &B, &S, &M, &D, &L, &Lq, &P, &layout, &qs_l, &qs_w, &ql0,
                 &ql1, &follow, &all16, &a16, knob, &group, &stats) == 19) {
        const MsdaFwdEntry e = !strcmp(entry, "fused") ? MsdaFwdEntry::fused : !strcmp(entry, "train") ? MsdaFwdEntry::fused_train
                             : !strcmp(entry, "f64") ? MsdaFwdEntry::public_f64 : MsdaFwdEntry::public_f32;
        const MsdaFwdRoute r = msda_forward_route(MsdaFwdQuery{e, B, S, M, D, L, Lq, P, layout, qs_l, qs_w, ql0, ql1, follow != 0, all16 != 0,
                                                               a16 != 0, msda_forward_parse_knob(knob), group != 0, stats != 0});
        static const char *const status[] = {"ok", "empty", "invalid_value", "not_supported"};
        if (r.status != MsdaFwdStatus::ok) printf("%s\n", status[(int)r.status]);
        else printf("%s %d %d %d %d %d\n", msda_forward_route_name(r.kind), r.probe, r.standdown, r.stats_pass, r.ref_mode, r.gather_vec);
    }
    return 0;
}
"""

ALL = ("auto", "gather", "tile", "bogus")
AUTO = ("auto", "bogus")
KNOB = 16       # position of the knob in a row's arguments


def pub(M, D, L, knobs, want, *, entry="f32", S=None, Lq=None, B=1, P=4, all16=1, a16=1, group=1):
    """The public entries: dense reference layout, all levels' tokens as queries."""
    S = L * 240 if S is None else S
    Lq = S if Lq is None else Lq
    return [((entry, B, S, M, D, L, Lq, P, 0, 0, 0, 0, L, 0, all16, a16, k, group, 0), want) for k in knobs]


def fused(M, D, L, want, *, layout=0, knobs=("auto",), entry="fused", S=None, Lq=None, B=1, P=4, pad_l=0, pad_w=0, ql=None, follow=1,
          all16=1, group=1):
    """The fused entries: dense query strides (+ pad), which for the slice-interleaved layouts (bit 2) means one stride of
    offsets + logits for both tensors.  `train`: layout 30, statistics wanted."""
    S = L * 240 if S is None else S
    Lq = S if Lq is None else Lq
    ql0, ql1 = (0, L) if ql is None else ql
    dense_l, dense_w = M * L * P * 2, M * L * P
    qs_l, qs_w = (dense_l + dense_w + pad_l, dense_l + dense_w + pad_w) if layout & 4 else (dense_l + pad_l, dense_w + pad_w)
    return [((entry, B, S, M, D, L, Lq, P, layout, qs_l, qs_w, ql0, ql1, follow, all16, all16, k, group, int(entry == "train")), want)
            for k in knobs]


def train(M, D, L, want, **kw):
    return fused(M, D, L, want, layout=30, entry="train", **kw)


def _layouts(M, D, L, name, **kw):
    """Every valid layout of the fused inference entry: ref_mode 2 when bit 1 (one reference point per (query, level)) is set."""
    return sum((fused(M, D, L, f"{name} 0 0 0 {2 if lay & 2 else 1} 0", layout=lay, **kw) for lay in (0, 1, 2, 3, 6, 10, 22, 30)), [])


TRAIN_S_LIMIT = -(-(1 << 29) // (12 * 8 * 7))       # the smallest S with 12 S M L >= 2^29 at M = 8, L = 7

ROWS = (
    # ---- public fp32 entry
    pub(8, 16, 7, AUTO, "group2 0 1 0 0 0")
    + pub(8, 16, 7, ("tile",), "group2 0 0 0 0 0")
    + pub(8, 16, 7, ("gather",), "gather 0 0 0 0 4")
    + pub(8, 16, 7, AUTO, "tile 1 0 0 0 0", group=0)
    + pub(8, 16, 7, ("tile",), "tile 0 0 0 0 0", group=0)
    + pub(4, 32, 6, AUTO, "group2 0 1 0 0 0")
    + pub(8, 16, 9, AUTO, "group-many 1 1 0 0 0")                 # the many-camera kernel takes the probe's verdict
    + pub(8, 16, 9, ("tile",), "group-many 0 0 0 0 0")
    + pub(8, 32, 16, AUTO, "group-many 1 1 0 0 0")
    + pub(8, 16, 8, AUTO, "tile 1 0 0 0 0")
    + pub(8, 16, 5, AUTO, "tile 1 0 0 0 0")
    + pub(8, 16, 1, AUTO, "tile 1 0 0 0 0")
    + pub(8, 16, 17, ALL, "gather 0 0 0 0 4")                     # more than TILE_MAX_LEVELS levels
    + pub(7, 16, 7, ALL, "gather 0 0 0 0 4")                      # an odd number of 16-channel heads
    + pub(8, 24, 7, ALL, "gather 0 0 0 0 4")
    + pub(8, 16, 7, ALL, "gather 0 0 0 0 4", P=3)
    + pub(8, 16, 7, ALL, "gather 0 0 0 0 4", Lq=7 * 240 - 1)      # a decoder-style call
    + pub(8, 16, 7, ALL, "gather 0 0 0 0 4", all16=0)             # e.g. sampling_loc only 8-byte aligned
    + pub(8, 30, 7, ALL, "gather 0 0 0 0 1")
    + pub(8, 16, 7, ALL, "gather 0 0 0 0 1", all16=0, a16=0)      # `value` only 8-byte aligned
    # one batch element's value tensor reaches 2 GiB: gather; one token less: the tile kernel (msda_group_fits fails)
    + pub(8, 16, 7, ALL, "gather 0 0 0 0 4", S=4194304)
    + pub(8, 16, 7, AUTO, "tile 1 0 0 0 0", S=4194303)
    # msda_group_fits: the sampling locations (448 floats per query) in 2^30 floats
    + pub(8, 16, 7, AUTO, "group2 0 1 0 0 0", S=2396745)
    + pub(8, 16, 7, AUTO, "tile 1 0 0 0 0", S=2396746)
    + pub(8, 16, 7, ("tile",), "tile 0 0 0 0 0", S=2396746)
    + pub(8, 16, 7, ALL, "empty", B=0)
    + pub(8, 16, 7, ALL, "empty", Lq=0)
    + pub(0, 16, 7, ALL, "invalid_value")
    # ---- public fp64 entry
    + pub(8, 16, 7, ALL, "gather 0 0 0 0 2", entry="f64")
    + pub(8, 30, 7, ALL, "gather 0 0 0 0 2", entry="f64")
    + pub(8, 15, 7, ALL, "gather 0 0 0 0 1", entry="f64")
    + pub(8, 16, 7, ALL, "gather 0 0 0 0 1", entry="f64", all16=0, a16=0)
    + pub(8, 16, 7, ALL, "empty", entry="f64", B=0)
    + pub(0, 16, 7, ALL, "invalid_value", entry="f64")
    # ---- fused inference entry
    + _layouts(8, 16, 7, "fused-group2")
    + _layouts(8, 16, 6, "fused-group2")
    + _layouts(4, 32, 7, "fused-group2")
    + _layouts(8, 16, 9, "fused-group-many")
    + _layouts(8, 16, 16, "fused-group-many")
    + _layouts(8, 16, 5, "fused-tile")
    + _layouts(8, 16, 8, "fused-tile")
    + _layouts(8, 16, 7, "fused-tile", group=0)
    + fused(8, 16, 7, "fused-group2 0 0 0 2 0", layout=30, knobs=ALL)                 # the knob does not reach this entry
    + _layouts(8, 16, 7, "fused-tile", ql=(0, 3), Lq=720)                            # a query-sharded call never groups
    + fused(8, 16, 7, "fused-tile 0 0 0 2 0", layout=30, ql=(4, 7), Lq=720)
    + fused(8, 16, 7, "not_supported", layout=30, ql=(0, 3), Lq=7 * 240 + 1)          # more queries than tokens
    + fused(8, 16, 7, "not_supported", layout=30, Lq=720)                            # all levels' queries: Lq == S
    + _layouts(8, 16, 7, "fused-group2", pad_l=64, pad_w=64)                         # a column block of a wider GEMM
    + fused(8, 16, 7, "fused-group2 0 0 0 1 0", S=0)                                  # launches over nothing
    + fused(8, 16, 7, "fused-group2 0 0 0 1 0", S=2396745)
    + fused(8, 16, 7, "fused-tile 0 0 0 1 0", S=2396746)                             # msda_group_fits, as for the public entry
    + fused(8, 16, 7, "invalid_value", pad_l=2)
    + fused(8, 16, 7, "invalid_value", pad_w=2)
    + fused(8, 16, 7, "invalid_value", pad_l=-4)
    + fused(8, 16, 7, "invalid_value", pad_w=-4)
    + fused(8, 16, 7, "invalid_value", ql=(3, 3))
    + fused(8, 16, 7, "invalid_value", ql=(4, 3))
    + fused(8, 16, 7, "invalid_value", ql=(-1, 3))
    + fused(8, 16, 7, "invalid_value", ql=(0, 8))
    + sum((fused(8, 16, 7, "invalid_value", layout=lay) for lay in (5, 8, 16, 24, 32)), [])
    + fused(8, 16, 7, "fused-group2 0 0 0 1 0", layout=20)                            # level-outermost slices, a reference point per point
    + fused(8, 24, 7, "invalid_value", layout=6)
    + fused(8, 16, 7, "invalid_value", layout=6, pad_l=64)                            # unequal strides
    + fused(8, 16, 7, "invalid_value", layout=6, pad_l=-4, pad_w=-4)                  # below offsets + logits
    + fused(8, 16, 7, "invalid_value", layout=6, follow=0)
    + fused(0, 16, 7, "invalid_value")
    + fused(8, 16, 7, "not_supported", all16=0)
    + fused(8, 16, 17, "not_supported")
    + fused(8, 16, 7, "not_supported", P=8)
    + fused(7, 16, 7, "not_supported")
    + fused(8, 24, 7, "not_supported")
    + fused(8, 24, 7, "not_supported", layout=3)
    + fused(8, 16, 7, "not_supported", B=0)
    + fused(8, 16, 7, "not_supported", S=4194304)
    # ---- fused training entry
    + train(8, 16, 7, "fused-group2 0 0 0 2 0", knobs=ALL)                            # the kernel writes the statistics
    + train(8, 16, 6, "fused-group2 0 0 0 2 0")
    + train(8, 16, 9, "fused-group-many 0 0 0 2 0")
    + train(8, 16, 5, "fused-tile 0 0 1 2 0")
    + train(4, 32, 5, "fused-tile 0 0 1 2 0")
    + train(8, 16, 7, "fused-tile 0 0 1 2 0", group=0)
    + train(8, 16, 7, "fused-group2 0 0 0 2 0", pad_l=64, pad_w=64)
    + train(8, 16, 7, "fused-group2 0 0 0 2 0", S=TRAIN_S_LIMIT - 1)
    + train(8, 16, 7, "not_supported", S=TRAIN_S_LIMIT)
    + train(8, 16, 7, "not_supported", S=TRAIN_S_LIMIT, pad_l=2, pad_w=2)             # refused before the strides are looked at
    + train(8, 16, 7, "invalid_value", pad_l=2, pad_w=2)
    + train(8, 16, 7, "invalid_value", pad_l=-4, pad_w=-4)
    + train(8, 16, 7, "not_supported", all16=0)
    + train(8, 16, 7, "not_supported", P=8)
    + train(8, 16, 7, "not_supported", B=0)
    + train(8, 16, 7, "not_supported", B=22, S=60 * 180 * 7)                          # the whole raw tensor in 2^30 floats
    + train(8, 16, 7, "fused-group2 0 0 0 2 0", B=21, S=60 * 180 * 7)
    + train(0, 16, 7, "invalid_value")
)


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("route")
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


def test_unknown_and_unset_knob_agree(routes):
    """A typo in MVDETR_MSDA_FWD_IMPL selects nothing: every `bogus` row has the route of the `auto` row of the same call."""
    got = {args: g for (args, _), g in zip(ROWS, routes)}
    pairs = [(a, a[:KNOB] + ("auto",) + a[KNOB + 1:]) for a in got if a[KNOB] == "bogus"]
    assert len(pairs) > 30 and all(u in got and got[b] == got[u] for b, u in pairs)
