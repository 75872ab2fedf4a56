"""MSDA backward under skewed attention-weight mass: parity per (level, head) block, not per tensor.

Some levels or heads of a call can carry many decades less weight than others (a camera that does not see a ground point:
softmax logits 10-20 lower).  Their grad_value blocks are then tiny in absolute terms, so the suite's other bars --
err / (1 + |ref|) and err relative to the whole tensor's maximum -- pass even when those blocks are all zeros.  The bars here
are taken per block (helpers.block_bar):

* grad_value: blocks [b, level, head] = gv[b, lsi[l] : lsi[l] + H*W, m, :] (band_cliff: [b, level, band, head], only tokens
  BAND_EDGE_MARGIN or more columns from an inner band edge), max |got - ref| <= 2e-5 * the block's max |ref|;
* sampling gradients: blocks [b, head, level] over (query, point) (band_cliff: [b, band, head, level] by the query's column):
  public grad_attn_weight and grad_sampling_loc, fused the gradients of the raw offsets and logits (chained by hand through
  the module arithmetic, helpers.fused_reference), <= 2e-4 * the block's max |ref|, offsets away from texel centres;
* deterministic mode: grad_value <= 2e-5 * block max + 16 steps of the call's one binary point (det_binary_point: 2^-(38 - eg
  - ea)): every job's flush and every far tap rounds once to that step, and a token lies in a few job windows.

The cases are Wildtrack / MultiviewX sized so that msda_bwd_onepass's workgroups run MIN_JOBS_PER_WORKGROUP or more jobs each:
only a workgroup's first job measures its fixed-point scale, the others guess it from the job before.  The env-knob routes
(split, onepass, spread, atomic; fused twopass / onepass) run the same cases in test_knob_routes_gpu.py's child processes."""
import math

import pytest
import torch

from helpers import (MIN_JOBS_PER_WORKGROUP, ONEPASS_MAX_GRID, SKEW_CASES, assert_skew_bars, onepass_jobs, skew_bars,
                     skew_case, skew_reference)

pytestmark = pytest.mark.gpu

PUBLIC = [c for c, v in SKEW_CASES.items() if v[0] == "public"]
FUSED = [c for c, v in SKEW_CASES.items() if v[0] == "fused"]


@pytest.fixture(scope="module")
def MSDA():
    import mvdetr_amd.ops  # noqa: F401
    import MultiScaleDeformableAttention as MSDA
    return MSDA


@pytest.fixture
def deterministic(MSDA):
    prev = MSDA.set_backward_deterministic(True)
    yield MSDA
    MSDA.set_backward_deterministic(prev)
    torch.cuda.synchronize()
    MSDA.release_scratch()


def _disturb():
    """Other work on the device between two runs (test_msda_deterministic_gpu.py)."""
    a = torch.randn(2048, 2048, device="cuda")
    (a @ a).sum().item()


def assert_enough_jobs(case):
    """A one-pass case must give every workgroup several jobs, or the guessed scale is hardly used (do not shrink it)."""
    form, a, _ = SKEW_CASES[case]
    if form == "fused" and a["D"] != 16:
        return                                                # (32-channel heads: msda_bwd_value_tok, exact bound per job)
    assert onepass_jobs(a["B"], a["L"], a["H"], a["W"], a["M"]) >= MIN_JOBS_PER_WORKGROUP * ONEPASS_MAX_GRID, case


def run_public(MSDA, case):
    value, shapes, lsi, loc, aw, go = skew_case(case)[1]
    return [x.cpu() for x in MSDA.ms_deform_attn_backward(*[x.cuda() for x in (value, shapes, lsi, loc, aw, go)], 64)]


def run_fused(MSDA, case):
    value, shapes, lsi, ref, raw, rows, go = skew_case(case)[1]
    dv, ds, dl, dr, draw = value.cuda(), shapes.cuda(), lsi.cuda(), ref.cuda(), raw.cuda()
    out, stats = MSDA.ms_deform_attn_forward_fused_train(dv, ds, dl, dr, draw)
    gv, graw = MSDA.ms_deform_attn_backward_fused(go.cuda(), dv, ds, dl, dr, draw, stats, out)
    return [gv.cpu(), graw.cpu()]


def det_step(case):
    """The deterministic mode's fixed-point step for the call: 2^-(38 - eg - ea), eg / ea the frexp exponents of max |grad_out|
    and max(1, max |attention weight|) (the fused pair's weights are softmax outputs: ea = 1)."""
    form, x = skew_case(case)
    go = x[-1]
    ea = math.frexp(max(1.0, float(x[4].abs().max())))[1] if form == "public" else 1
    return 2.0 ** -(38 - math.frexp(float(go.abs().max()))[1] - ea)


@pytest.mark.parametrize("case", PUBLIC)
def test_public_backward_per_block_under_mass_skew(MSDA, case):
    """The public contract's default route (msda_bwd_value_tok + the sampling kernels) against the fp64 C oracle, per block."""
    assert_enough_jobs(case)
    assert_skew_bars(case, skew_bars(case, run_public(MSDA, case), skew_reference(case)))


@pytest.mark.parametrize("case", FUSED)
def test_fused_training_backward_per_block_under_mass_skew(MSDA, case):
    """The fused training pair's default route: msda_bwd_onepass<fused> (16-channel heads, 7 levels: its grad_value-only form;
    12 levels: all three gradients) or msda_bwd_value_tok<32, fused> (32-channel heads)."""
    assert_enough_jobs(case)
    assert_skew_bars(case, skew_bars(case, run_fused(MSDA, case), skew_reference(case)))


@pytest.mark.parametrize("case", ["level_cliff_wildtrack", "head_cliff_wildtrack", "fused_level_cliff_wildtrack"])
def test_deterministic_backward_per_block_under_mass_skew(deterministic, case):
    """msda_bwd_onepass<DET>: bit-identical over two runs with other device work in between, and every block within 2e-5 of
    its maximum plus 16 steps of the call's binary point."""
    MSDA = deterministic
    assert_enough_jobs(case)
    run = run_public if SKEW_CASES[case][0] == "public" else run_fused
    first = run(MSDA, case)
    _disturb()
    for a, b in zip(first, run(MSDA, case)):
        assert torch.equal(a, b)
    assert_skew_bars(case, skew_bars(case, first, skew_reference(case), gv_floor=16 * det_step(case)))


def test_whole_tensor_bars_cannot_see_a_light_block(MSDA):
    """The suite's older bars -- err / (1 + |ref|) < 2e-4 for all three gradients -- on the fused Wildtrack case.  They pass
    whether or not the light levels' grad_value blocks are right (the library before the one-pass kernel's lower guess check
    passed them with light blocks 14 % to 100 % off): the block bars above are the ones that bite."""
    from helpers import fused_plain
    case = "fused_level_cliff_wildtrack"
    gv, graw = run_fused(MSDA, case)
    ref = skew_reference(case)
    a = SKEW_CASES[case][1]
    goff, glogit = fused_plain(graw, ref["rows"], a["M"], a["L"])
    assert ((gv.double() - ref["gv"].double()).abs() / (1.0 + ref["gv"].double().abs())).max().item() < 2e-4
    smooth = ref["smooth"][..., None]
    assert (((goff.double() - ref["gl"].double()).abs() / (1.0 + ref["gl"].double().abs())) * smooth).max().item() < 2e-4
    assert ((glogit.double() - ref["ga"].double()).abs() / (1.0 + ref["ga"].double().abs())).max().item() < 2e-4
