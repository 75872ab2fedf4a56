"""The block bar of test_msda_mass_skew_gpu.py (helpers.block_bar / skew_bars) checked on its own, and applied to the library's
host path (csrc/host_path.cpp: CPU tensors through MultiScaleDeformableAttention) on scaled-down skewed inputs against the fp64
C oracle.  Runs without a GPU."""
import pytest
import torch

from helpers import HOST_SKEW_CASES, assert_skew_bars, block_bar, skew_bars, skew_case, skew_reference


def test_block_bar_names_the_worst_block():
    ref = torch.ones(2, 3, 5)
    ref[1, 2] = 1e-9                                           # a light block
    got = ref.clone()
    got[0, 1, 4] += 1e-6                                       # 1e-6 of its block: inside 2e-5
    r = block_bar(got, ref, (0, 1), 2e-5)
    assert r["ratio"] < 1.0 and r["block"] == (0, 1)
    got[1, 2, 0] = 0.0                                         # the light block loses an element: 1e-9 absolute
    r = block_bar(got, ref, (0, 1), 2e-5)
    assert r["ratio"] > 1e4 and r["block"] == (1, 2) and r["ref_max"] == pytest.approx(1e-9)
    assert r["blocks_min"] == pytest.approx(1e-9) and r["blocks_max"] == 1.0
    # a floor (the deterministic mode's step) absorbs it ...
    assert block_bar(got, ref, (0, 1), 2e-5, floor=2e-9)["ratio"] <= 1.0
    # ... and so does a mask, which also leaves the entry out of the block's maximum
    mask = torch.ones_like(ref, dtype=torch.bool)
    mask[1, 2, 0] = False
    assert block_bar(got, ref, (0, 1), 2e-5, mask=mask)["ratio"] < 1.0
    mask[1, 2] = False
    mask[1, 2, 1] = True
    assert block_bar(got, ref, (0, 1), 2e-5, mask=mask)["blocks_min"] == pytest.approx(1e-9)
    # blocks along non-leading dims; NaN fails its block
    got = ref.clone()
    got[1, 0, 3] = float("nan")
    r = block_bar(got, ref, (1, 2), 2e-5)
    assert r["ratio"] == float("inf") and r["block"] == (0, 3)


@pytest.fixture(scope="module")
def host_results():
    import mvdetr_amd.ops  # noqa: F401
    import MultiScaleDeformableAttention as MSDA
    out = {}
    for case in HOST_SKEW_CASES:
        value, shapes, lsi, loc, aw, go = skew_case(case)[1]
        got = MSDA.ms_deform_attn_backward(value, shapes, lsi, loc, aw, go, 64)
        assert got[0].device.type == "cpu"
        out[case] = got
    return out


@pytest.mark.parametrize("case", sorted(HOST_SKEW_CASES))
def test_host_path_per_block_under_mass_skew(host_results, case):
    """The host path's fp32 backward passes the GPU kernels' block bars, and the case is not vacuous (block maxima spanning 2^20
    and more)."""
    assert_skew_bars(case, skew_bars(case, host_results[case], skew_reference(case)))


@pytest.mark.parametrize("corrupt", ["zeroed", "scaled"])
def test_block_bar_rejects_a_corrupted_light_block_the_old_bar_accepts(host_results, corrupt):
    """One [b, level, head] block of grad_value zeroed, or scaled by 1 + 1e-3: the block bar fails it, while the whole-tensor bar
    err / (1 + |ref|) < 2e-4 does not notice."""
    case = "level_cliff_host"
    ref = skew_reference(case)
    _, a, (_, ks) = HOST_SKEW_CASES[case]
    L, H, W, M = a["L"], a["H"], a["W"], a["M"]
    gv = host_results[case][0].clone()
    for level, head in ((3, 5), (1, 0)):                       # 2^-29 and 2^-20 of the heavy levels
        blk = gv.view(1, L, H * W, M, -1)[0, level, :, head]
        if corrupt == "zeroed":
            blk.zero_()
        else:
            blk.mul_(1.0 + 1e-3)
        got = (gv,) + tuple(host_results[case][1:])
        bars = skew_bars(case, got, ref)
        assert bars["grad_value"]["ratio"] > 1.0 and bars["grad_value"]["block"] == (0, level, head), (level, head, bars)
        old = ((gv.double() - ref["gv"].double()).abs() / (1.0 + ref["gv"].double().abs())).max().item()
        assert old < 2e-4
        gv = host_results[case][0].clone()
