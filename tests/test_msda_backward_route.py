"""The MSDA backward's route table (csrc/msda_backward_route.h), checked without a GPU and without loading the library: the
header is plain C++, so a small stand-alone program compiled with g++ prints the route of every row below and the test
compares it with the route written next to the row.  The rows are the two entries' dispatch as INTEGRATION.md's knob table
describes it, with every limit at which a call changes route or is refused.

A printed route is `<name> <sampling kernel> <lanes VEC> <lanes G>`: the name mvdetr_msda_last_backward_route() reports; the
sampling kernel of a two-kernel route (`resident` = msda_bwd_sampling_resident, `groups` = msda_bwd_sampling_groups<16, 7> for
16-channel and <32, 3> for 32-channel heads, `fused` = msda_bwd_fused_sampling<NG = L>); and for `atomic` the
msda_bwd_lanes<T, VEC, G> instantiation, G = 0 meaning msda_bwd_serial<T>.  A refused or empty call prints its status alone."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvdetr_amd", "csrc")

PROGRAM = r"""
#include "msda_backward_route.h"
#include <stdio.h>
using namespace mvdetr;
int main()
{
    char entry[16], knob[32];
    int B, S, M, D, L, Lq, P, raw_q, all16, a16, det;
    while (scanf("%15s %d %d %d %d %d %d %d %d %d %d %31s %d", entry, &B, &S, &M, &D, &L, &Lq, &P, &raw_q, &all16, &a16, knob, &det) == 13) {
        const MsdaBwdEntry e = !strcmp(entry, "fused") ? MsdaBwdEntry::fused : !strcmp(entry, "f64") ? MsdaBwdEntry::public_f64 : MsdaBwdEntry::public_f32;
        const MsdaBwdRoute r = msda_backward_route(e, B, S, M, D, L, Lq, P, raw_q, all16 != 0, a16 != 0,
                                                   msda_backward_parse_knob(strcmp(knob, "unset") ? knob : nullptr), det != 0);
        static const char *const status[] = {"ok", "empty", "invalid_value", "not_supported"};
        static const char *const sampling[] = {"-", "resident", "groups", "fused"};
        if (r.status != MsdaBwdStatus::ok) printf("%s\n", status[(int)r.status]);
        else printf("%s %s %d %d\n", msda_backward_route_name(r.kind), sampling[(int)r.sampling], r.lanes_vec, r.lanes_g);
    }
    return 0;
}
"""

ALL = ("unset", "twopass", "split", "onepass", "atomic", "bogus")
LANES16 = "atomic - 1 16"


def pub(M, D, L, knobs, want, *, entry="f32", S=None, Lq=None, B=1, P=4, all16=1, a16=1, det=0):
    S = L * 240 if S is None else S
    Lq = S if Lq is None else Lq
    return [((entry, B, S, M, D, L, Lq, P, 0, all16, a16, k, det), want) for k in knobs]


def fused(M, D, L, knobs, want, *, S=None, P=4, raw_q=None, pad=0, all16=1, det=0):
    S = L * 240 if S is None else S
    raw_q = M * L * 12 + pad if raw_q is None else raw_q
    return [(("fused", 1, S, M, D, L, S, P, raw_q, all16, all16, k, det), want) for k in knobs]


ROWS = (
    # ---- public fp32 entry
    pub(8, 16, 7, ("unset", "twopass", "bogus"), "twopass resident 0 0")
    + pub(8, 16, 7, ("split",), "split resident 0 0")
    + pub(8, 16, 7, ("onepass",), "onepass - 0 0")
    + pub(8, 16, 7, ("atomic",), LANES16)
    + pub(8, 16, 9, ("unset",), "twopass groups 0 0")
    + pub(8, 16, 9, ("split",), "split groups 0 0")
    + pub(8, 16, 9, ("onepass",), "onepass - 0 0")
    + pub(4, 32, 5, ("unset", "split", "onepass"), "twopass groups 0 0")
    + pub(4, 32, 5, ("atomic",), "atomic - 1 32")
    + pub(7, 16, 7, ALL, LANES16)                                   # an odd number of 16-channel heads
    + pub(7, 16, 7, ALL, "not_supported", det=1)
    + pub(8, 16, 17, ALL, LANES16)                                  # more than TILE_MAX_LEVELS levels
    + pub(8, 16, 7, ALL, LANES16, Lq=7 * 240 - 1)
    + pub(8, 16, 7, ALL, LANES16, P=8)
    + pub(8, 16, 7, ALL, LANES16, all16=0)                          # e.g. grad_loc only 8-byte aligned
    + pub(8, 24, 7, ALL, "atomic - 0 0")                            # serial
    + pub(8, 128, 7, ALL, "atomic - 4 32")
    + pub(8, 128, 7, ALL, "atomic - 0 0", all16=0, a16=0)           # `value` only 8-byte aligned
    + pub(8, 16, 7, ALL, "atomic - 1 16", entry="f64")
    + pub(8, 128, 7, ALL, "atomic - 2 64", entry="f64")
    + pub(8, 256, 7, ALL, "atomic - 0 0", entry="f64")
    # one query's locations reach 2^31 bytes per batch element: the one-pass kernels do not take the call, value_tok does
    + pub(8, 16, 16, ("unset", "split", "onepass"), "twopass groups 0 0", S=524288)
    + pub(8, 16, 7, ("unset", "twopass", "split", "onepass", "bogus"), "deterministic - 0 0", det=1)
    + pub(8, 16, 7, ("atomic",), "not_supported", det=1)
    + pub(4, 32, 5, ALL, "not_supported", det=1)
    + pub(8, 16, 7, ALL, "not_supported", entry="f64", det=1)
    + pub(8, 128, 7, ALL, "not_supported", entry="f64", det=1)
    + pub(8, 16, 16, ALL, "not_supported", S=262144, det=1)         # S * L * P = 2^24
    + pub(8, 16, 16, ("split",), "split groups 0 0", S=262144)
    + pub(8, 16, 7, ALL, "empty", B=0)
    + pub(8, 16, 7, ALL, "empty", Lq=0)
    + pub(0, 16, 7, ALL, "invalid_value")
    # ---- fused entry
    + fused(8, 16, 7, ("unset", "split", "atomic", "bogus"), "fused-split fused 0 0")
    + fused(8, 16, 6, ("unset", "split", "atomic", "bogus"), "fused-split fused 0 0")
    + fused(8, 16, 7, ("twopass",), "fused-twopass fused 0 0")
    + fused(8, 16, 7, ("onepass",), "fused-onepass - 0 0")
    + fused(8, 16, 5, ALL, "fused-onepass - 0 0")
    + fused(8, 16, 9, ALL, "fused-onepass - 0 0")
    + fused(4, 32, 5, ALL, "fused-groups groups 0 0")
    + fused(8, 16, 7, ALL, "fused-deterministic - 0 0", det=1)
    + fused(8, 16, 9, ALL, "fused-deterministic - 0 0", det=1)
    + fused(4, 32, 5, ALL, "not_supported", det=1)
    + fused(8, 16, 7, ALL, "invalid_value", pad=-4)
    + fused(8, 16, 7, ALL, "invalid_value", pad=2)
    + fused(8, 16, 7, ("unset", "split", "atomic", "bogus"), "fused-split fused 0 0", pad=64)
    + fused(8, 16, 7, ("twopass",), "fused-twopass fused 0 0", pad=64)
    + fused(8, 16, 7, ("onepass",), "fused-onepass - 0 0", pad=64)
    + fused(8, 16, 7, ALL, "not_supported", raw_q=(1 << 29) // (7 * 240) // 4 * 4 + 4)      # S * raw_q >= 2^29
    + fused(8, 16, 7, ALL, "not_supported", all16=0)                # `raw` only 8-byte aligned, or an odd ref_bstride
    + fused(8, 16, 7, ALL, "not_supported", P=8)
    + fused(0, 16, 7, ALL, "invalid_value")
    + fused(8, 16, 7, ALL, "empty", S=0)
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
    """A typo in MVDETR_MSDA_BWD_IMPL selects nothing: every `bogus` row has the route of the `unset` row of the same call."""
    got = {args: g for (args, _), g in zip(ROWS, routes)}
    pairs = [(a, a[:11] + ("unset",) + a[12:]) for a in got if a[11] == "bogus"]
    assert len(pairs) > 20 and all(u in got and got[b] == got[u] for b, u in pairs)
