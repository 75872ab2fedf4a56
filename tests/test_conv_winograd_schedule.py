"""The schedule switch of the 8-wave Winograd kernel (mvdetr_winograd_set_schedule, mvdetr_amd/csrc/conv_winograd.hip), without a
GPU: the setter's values, the family table on both sides of the C ABI, and the plan, which does not depend on the schedule."""
import pytest

FAMILIES = [(64, 64, 1), (128, 128, 1), (128, 256, 1), (256, 256, 1), (256, 256, 2), (256, 512, 2), (512, 512, 1), (512, 512, 4)]
OUTSIDE = [(24, 192, 1), (64, 64, 2), (256, 512, 1), (512, 512, 2), (64, 128, 1)]


@pytest.fixture()
def cw():
    from mvdetr_amd.ops import conv_winograd
    prev = conv_winograd.set_winograd_schedule(0)
    yield conv_winograd
    conv_winograd.set_winograd_schedule(prev)


def test_the_setter_returns_the_previous_value(cw):
    assert cw.set_winograd_schedule(1) == 0
    assert cw.set_winograd_schedule(2) == 1
    assert cw.set_winograd_schedule(0) == 2
    assert cw.set_winograd_schedule(0) == 0


@pytest.mark.parametrize("value", [3, 4, 5, -1, 100])
def test_anything_else_means_the_table(cw, value):
    assert cw.set_winograd_schedule(2) == 0
    assert cw.set_winograd_schedule(value) == 2
    for C, K, d in FAMILIES + OUTSIDE:
        assert cw.schedule_of(C, K, d) == (2 if (C, K, d) in cw.SCHEDULE_FAMILIES else 1)
    assert cw.set_winograd_schedule(0) == 0


def test_the_table_is_the_c_librarys_and_inside_the_eight_families(cw):
    assert set(cw.SCHEDULE_FAMILIES) <= set(FAMILIES) and len(set(cw.SCHEDULE_FAMILIES)) == len(cw.SCHEDULE_FAMILIES)
    on = {f for f in FAMILIES + OUTSIDE if cw.schedule_of(*f) == 2}
    assert on == set(cw.SCHEDULE_FAMILIES)
    assert all(cw.schedule_of(*f) in (1, 2) for f in FAMILIES + OUTSIDE)
    try:
        for v in (1, 2):
            cw.set_winograd_schedule(v)
            assert all(cw.schedule_of(*f) == v for f in FAMILIES + OUTSIDE)
    finally:
        assert cw.set_winograd_schedule(0) == 2


def test_the_plan_does_not_depend_on_the_schedule(cw):
    shapes = [(7, 90, 160, C, K, d) for C, K, d in FAMILIES + OUTSIDE] + [(5, 9, 13, 24, 192, 1), (1, 1, 1, 8, 64, 4)]
    want = [cw.plan(*s, 256) for s in shapes]
    assert all(tuple(p) == ("units", "G", "R", "rem", "half_units", "variant") for p in want)
    assert all(p["variant"] == 2 for p in want[:len(FAMILIES)])
    try:
        for v in (1, 2, 7):
            cw.set_winograd_schedule(v)
            assert [cw.plan(*s, 256) for s in shapes] == want
    finally:
        cw.set_winograd_schedule(0)

