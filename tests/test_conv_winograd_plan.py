"""How a Winograd convolution call is split between the persistent kernel and the half-unit tail (mvdetr_winograd_plan,
mvdetr_amd/csrc/conv_winograd.hip), without a GPU: the workload's eight shapes at 256 CUs against the table worked out by
hand, and 200 seeded small shapes, grids and caps against a brute-force count of tiles and of the units each launch runs."""
import random

import pytest

WILDTRACK = [  # C, K, d, (N, H, W), units, R, rem at 256 CUs
    (64, 64, 1, (7, 180, 320), 1575, 6, 39),
    (128, 128, 1, (7, 90, 160), 788, 3, 20),
    (128, 256, 1, (7, 90, 160), 1576, 6, 40),
    (256, 256, 1, (7, 90, 160), 1576, 6, 40),
    (256, 256, 2, (7, 90, 160), 1612, 6, 76),
    (512, 512, 1, (7, 90, 160), 3152, 12, 80),
    (256, 512, 2, (7, 90, 160), 3224, 12, 152),
    (512, 512, 4, (7, 90, 160), 3224, 12, 152),
]


@pytest.fixture()
def cw():
    from mvdetr_amd.ops import conv_winograd
    prev = conv_winograd.set_winograd_tail(1), conv_winograd.set_winograd_max_workgroups(0)
    yield conv_winograd
    conv_winograd.set_winograd_tail(prev[0])
    conv_winograd.set_winograd_max_workgroups(prev[1])


def _tiles(N, H, W, d):
    """2x2 output tiles, counted: every sub-lattice (y mod d, x mod d) of every image has its own grid."""
    per_image = 0
    for sy in range(d):
        for sx in range(d):
            h, w = len(range(sy, H, d)), len(range(sx, W, d))
            per_image += len(range(0, h, 2)) * len(range(0, w, 2))
    return N * per_image


@pytest.mark.parametrize("C,K,d,pixels,units,R,rem", WILDTRACK)
def test_the_workloads_shapes_at_256_cus(cw, C, K, d, pixels, units, R, rem):
    assert cw.set_winograd_tail(2) == 1
    p = cw.plan(*pixels, C, K, d, 256)
    assert (p["units"], p["G"], p["R"], p["rem"], p["half_units"]) == (units, 256, R, rem, 2 * rem)
    cw.set_winograd_tail(0)
    assert cw.plan(*pixels, C, K, d, 256)["half_units"] == 0
    cw.set_winograd_tail(1)
    p = cw.plan(*pixels, C, K, d, 256)
    assert p["half_units"] in (0, 2 * rem)                                    # the family table decides ...
    if rem > 128:
        assert p["half_units"] == 0                                           # ... but never past half a round


def test_the_default_tail_runs_where_it_measured_faster(cw):
    on = {(C, K, d) for C, K, d, pixels, *_ in WILDTRACK if cw.plan(*pixels, C, K, d, 256)["half_units"]}
    assert on == set(cw.TAIL_FAMILIES)


def test_the_default_variant_is_the_eight_wave_kernel_on_the_workloads_families_only(cw):
    assert cw.set_winograd_variant(0) == 0
    for C, K, d, pixels, *_ in WILDTRACK:
        assert cw.plan(*pixels, C, K, d, 256)["variant"] == 2
        assert cw.plan(2, 16, 16, C, K, d, 256)["variant"] == 2               # the table has no pixel floor: the callers do
    for C, K, d in ((24, 192, 1), (64, 64, 2), (256, 512, 1), (512, 512, 2), (64, 128, 1)):
        assert cw.plan(7, 90, 160, C, K, d, 256)["variant"] == 1
    try:
        for v in (1, 2):
            cw.set_winograd_variant(v)
            assert cw.plan(7, 90, 160, 24, 192, 1, 256)["variant"] == v == cw.plan(7, 90, 160, 512, 512, 1, 256)["variant"]
    finally:
        assert cw.set_winograd_variant(0) == 2
    assert cw.set_winograd_variant(5) == 0 and cw.set_winograd_variant(0) == 0    # anything else: the table


def test_seeded_small_shapes_against_a_count(cw):
    rng = random.Random(20260)
    tails = 0
    for _ in range(200):
        N, H, W = rng.randint(1, 9), rng.randint(1, 40), rng.randint(1, 40)
        C, K, d = 8 * rng.randint(1, 4), 64 * rng.randint(1, 4), rng.choice((1, 2, 4))
        cus, cap, tail = rng.randint(1, 40), rng.choice((0, 0, 1, 2, 3, 7)), rng.choice((0, 1, 2))
        cw.set_winograd_max_workgroups(cap)
        cw.set_winograd_tail(tail)
        p = cw.plan(N, H, W, C, K, d, cus)
        units = -(-_tiles(N, H, W, d) // 64) * (K // 64)
        G = min(units, cus, cap) if cap else min(units, cus)
        assert (p["units"], p["G"], p["R"], p["rem"]) == (units, G, units // G, units % G), (N, H, W, C, K, d, cus, cap)
        # the units each launch runs, one by one: workgroup g of the persistent kernel takes g, g + G, ... below its limit
        limit = units - units % G if p["half_units"] else units
        main = sorted(u for g in range(G) for u in range(g, limit, G))
        rest = sorted({units - units % G + j // 2 for j in range(p["half_units"])})
        assert main + rest == list(range(units))
        if tail == 0 or units % G == 0 or (tail == 1 and 2 * (units % G) > G):
            assert p["half_units"] == 0
        if tail == 2 and units % G:
            assert p["half_units"] == 2 * (units % G)
        tails += bool(p["half_units"])
    assert tails >= 20, tails


def test_plan_refuses_what_the_convolution_refuses(cw):
    from mvdetr_amd import _lib
    import ctypes
    out = (ctypes.c_int64 * 6)()
    ptr = ctypes.cast(out, ctypes.c_void_p)
    lib = _lib.lib()
    assert lib.mvdetr_winograd_plan(1, 8, 8, 8, 64, 1, 4, ptr) == 0
    assert lib.mvdetr_winograd_plan(1, 8, 8, 12, 64, 1, 4, ptr) == 801        # C % 8
    assert lib.mvdetr_winograd_plan(1, 8, 8, 8, 96, 1, 4, ptr) == 801         # K % 64
    assert lib.mvdetr_winograd_plan(1, 8, 8, 8, 64, 3, 4, ptr) == 801         # dilation
    assert lib.mvdetr_winograd_plan(1, 8, 8, 8, 64, 1, 0, ptr) == 1           # no workgroups
    assert lib.mvdetr_winograd_plan(1, 8, 8, 8, 64, 1, 4, None) == 1


def test_the_tail_setter_returns_the_previous_mode(cw):
    assert cw.set_winograd_tail(0) == 1
    assert cw.set_winograd_tail(2) == 0
    assert cw.set_winograd_tail(7) == 2                                       # anything else: the default
    assert cw.set_winograd_tail(1) == 1
