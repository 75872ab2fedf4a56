"""16-bit inference on the GPU, the routes and edges tests/test_half_inference_gpu.py leaves out: both work mappings of the
fused deformable attention and its limits, strides, refusals and non-finite inputs; the two converters of csrc/half_types.h on
every bit pattern (ties, subnormals, overflow); the unaligned and the grid-stride instantiations of add + LayerNorm; the warp at
channel counts and alignments that change its route.  Oracles and bars are those of the existing file: the oracle runs on the
CPU on the same already rounded inputs, upcast, and the bar is one rounding of the storage type plus the op's fp32 bar --
except where a test compares bit patterns, with no tolerance at all."""
import functools

import pytest
import torch
from torch import nn

from helpers import assert_rounded_once, fused_plain, fused_train_inputs, ulp_of
from oracle import c_oracle
from test_half_inference_gpu import DST_HW, DTYPES, FP32_TOL, LN_FP32_TOL, MSDA_CASES, N_VIEWS, check_warp, warp_case, warp_mats

pytestmark = pytest.mark.gpu


def _msda():
    from mvdetr_amd.ops import MultiScaleDeformableAttention as MSDA
    return MSDA


# ---- 1. fused deformable attention ------------------------------------------------------------------------------------------
def fused_oracle(value, shapes, lsi, ref, raw, rows):
    """msda_case's oracle (test_half_inference_gpu.py) for reference points [1 or B, L, Lq, 2]: fp32 softmax,
    loc = ref + off / (W, H), then the C oracle's core, all on the rounded inputs, upcast.  -> want [B, Lq, M*D], loc."""
    M, L = value.shape[2], shapes.shape[0]
    H, W = int(shapes[0, 0]), int(shapes[0, 1])
    off, logit = fused_plain(raw.float(), rows, M, L)
    wh = torch.tensor([W, H], dtype=torch.float32)
    ref_ql = ref.transpose(1, 2)                                             # [1 or B, Lq, L, 2]
    loc = (ref_ql[:, :, None, :, None, :] + off / wh).contiguous()
    B, Lq = logit.shape[:2]
    aw = torch.softmax(logit.flatten(-2), -1).view(B, Lq, M, L, 4).contiguous()
    return c_oracle.msda_forward(value.float(), shapes, lsi, loc, aw), loc


def repack(off, logit, rows):
    """Plain offsets [B, Lq, M, L, P, 2] and logits [B, Lq, M, L, P] -> the fused call's raw layout (fused_plain's inverse)."""
    B, Lq = logit.shape[:2]
    return torch.cat([off.reshape(B, Lq, -1), logit.reshape(B, Lq, -1)], -1).index_select(-1, rows).contiguous()


@functools.lru_cache(maxsize=None)
def fused_case(L, H, W, M, D, B, noise_px, dtype, logit_offsets=None):
    """Rounded inputs of one fused call, the row permutation, the oracle's result and the share of taps outside the map."""
    value, shapes, lsi, ref, raw, rows = fused_train_inputs(L, H, W, M=M, D=D, B=B, seed=3, noise_px=noise_px,
                                                            level_logit_offsets=logit_offsets)
    value, raw = value.to(dtype), raw.to(dtype)
    want, loc = fused_oracle(value, shapes, lsi, ref, raw, rows)
    outside = ((loc < 0) | (loc > 1)).any(-1).float().mean().item()
    return value, shapes, lsi, ref, raw, rows, want, outside


def named_case(name, noise_px, dtype):
    c = MSDA_CASES[name]
    return fused_case(c["L"], c["H"], c["W"], c["M"], c["D"], c["B"], noise_px, dtype)


def run_fused(value, shapes, lsi, ref, raw):
    MSDA = _msda()
    args = [a.cuda() for a in (value, shapes, lsi, ref, raw)]
    assert MSDA.fused_half_supported(args[0], shapes.shape[0], value.shape[1], 4)
    out = MSDA.ms_deform_attn_forward_fused_half(*args)
    assert MSDA.last_forward_kernel() == "msda_fwd_fused_half"
    return out


# (M, D) -> lanes per (query, workgroup), 128-byte slices per token row (None: the narrow mapping, one head per query slot)
WORK_MAPPINGS = {(2, 16): (2, None), (6, 16): (2, None), (1, 32): (4, None), (3, 32): (4, None),
                 (4, 16): (8, 1), (16, 16): (8, 4), (8, 32): (8, 4)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("noise_px", [1.0, 6.0])
@pytest.mark.parametrize("M,D", sorted(WORK_MAPPINGS))
def test_fused_msda_half_work_mappings(M, D, noise_px, dtype):
    """Both work mappings of msda_fwd_fused_half: eight lanes per 128-byte slice (1 and 4 slices; 2 are in the existing file) and
    one head per query slot (2 or 4 lanes per query, tiles 16 and 8 queries high), on a map whose width is ragged against the
    8-wide tile and whose height is ragged against tile heights 4, 8 and 16 and is more than one tile of the tallest."""
    chunks = M * D // 8
    lpq = 8 if chunks % 8 == 0 else D // 8                                   # the launcher's choice (the library names no mapping)
    assert (lpq, M * D // 64 if lpq == 8 else None) == WORK_MAPPINGS[(M, D)]
    value, shapes, lsi, ref, raw, _, want, outside = fused_case(3, 18, 11, M, D, 2, noise_px, dtype)
    assert outside > 0.0                                                      # some taps leave the map (zero padding)
    assert_rounded_once(run_fused(value, shapes, lsi, ref, raw), want, dtype, FP32_TOL)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [1, 16])
def test_fused_msda_half_level_limits(L, dtype):
    value, shapes, lsi, ref, raw, _, want, outside = fused_case(L, 3, 5, 8, 16, 1, 1.0, dtype)
    assert outside > 0.0
    assert_rounded_once(run_fused(value, shapes, lsi, ref, raw), want, dtype, FP32_TOL)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_msda_half_refuses_seventeen_levels(dtype):
    MSDA = _msda()
    value = torch.zeros(1, 17 * 15, 8, 16, dtype=dtype, device="cuda")
    assert not MSDA.fused_half_supported(value, 17, 17 * 15, 4)
    assert MSDA.fused_half_supported(value[:, :16 * 15], 16, 16 * 15, 4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_msda_half_per_batch_reference_points_differ(dtype):
    """The batch stride of the reference points: batch element 1 gets points up to 0.4 cell off batch element 0's, and the
    oracle takes the per-batch points.  A kernel that ignored the stride would return the shared call's result, which differs
    from the oracle by more than the bar (asserted)."""
    value, shapes, lsi, ref, raw, rows, _, _ = named_case("L2_5x7_M8_D16_B2", 1.0, dtype)
    H, W = int(shapes[0, 0]), int(shapes[0, 1])
    g = torch.Generator().manual_seed(11)
    jitter = torch.zeros(2, *ref.shape[1:])
    jitter[1] = (torch.rand(ref.shape[1:], generator=g) * 2 - 1) * 0.4 / torch.tensor([W, H], dtype=torch.float32)
    ref_b = (ref.expand(2, -1, -1, -1) + jitter).contiguous()
    want, _ = fused_oracle(value, shapes, lsi, ref_b, raw, rows)
    out = run_fused(value, shapes, lsi, ref_b, raw)
    shared = run_fused(value, shapes, lsi, ref, raw)
    assert_rounded_once(out, want, dtype, FP32_TOL)
    assert torch.equal(out[0], shared[0])                                     # (no jitter there)
    gap = (shared[1].cpu().double() - want[1].double()).abs() - (ulp_of(dtype) * want[1].double().abs() + FP32_TOL)
    assert gap.max().item() > 0.0, gap.max().item()                           # the shared call's result would NOT pass


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_msda_half_padded_raw(dtype):
    """raw rows wider than M*L*12 (the query stride is the row's, the pad is never read: it holds NaN), and the refusal of a
    row stride that is no multiple of 4 elements (the kernel's 8-byte accesses)."""
    MSDA = _msda()
    value, shapes, lsi, ref, raw, _, want, _ = named_case("L2_5x7_M8_D16_B2", 1.0, dtype)
    B, S, n = raw.shape
    packed = run_fused(value, shapes, lsi, ref, raw)
    wide = torch.full((B, S, n + 8), float("nan"), dtype=dtype, device="cuda")
    wide[..., :n] = raw.cuda()
    args = [a.cuda() for a in (value, shapes, lsi, ref)]
    view = wide[..., :n]
    assert view.stride(1) == n + 8 and not view.is_contiguous()
    out = MSDA.ms_deform_attn_forward_fused_half(*args, view)
    assert MSDA.last_forward_kernel() == "msda_fwd_fused_half"
    assert torch.equal(out, packed)
    assert_rounded_once(out, want, dtype, FP32_TOL)
    odd = torch.full((B, S, n + 2), float("nan"), dtype=dtype, device="cuda")
    odd[..., :n] = raw.cuda()
    with pytest.raises(RuntimeError, match="hipError 801"):                   # hipErrorNotSupported: refused, not computed
        MSDA.ms_deform_attn_forward_fused_half(*args, odd[..., :n])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("broken", ["shapes", "level_start_index"])
def test_fused_msda_half_unequal_shapes_give_nan_everywhere(broken, dtype):
    """Level shapes are device data, so the host cannot refuse them: a call whose shapes / level_start_index are not L equal
    maps laid end to end returns NaN in every output element.  The kernel's early-return path reads spatial_shapes and
    level_start_index only (L entries each), writes B*S*M*D/2 NaN words into `out` and returns BEFORE it reads value,
    reference points or raw -- no address depends on the bad shapes.  S = 162 passes the host's S % L test."""
    MSDA = _msda()
    value, shapes, lsi, ref, raw, _, want, _ = named_case("L3_6x9_M4_D32", 1.0, dtype)
    B, S, M, D = value.shape
    if broken == "shapes":
        bad_shapes = torch.tensor([(6, 9), (9, 6), (6, 9)], dtype=torch.long)
        bad_lsi = torch.tensor([0, 54, 108], dtype=torch.long)
    else:
        bad_shapes, bad_lsi = shapes, torch.tensor([0, 53, 108], dtype=torch.long)
    assert int(bad_shapes.prod(1).sum()) == S == 162
    out = MSDA.ms_deform_attn_forward_fused_half(value.cuda(), bad_shapes.cuda(), bad_lsi.cuda(), ref.cuda(), raw.cuda())
    assert MSDA.last_forward_kernel() == "msda_fwd_fused_half"
    assert out.shape == (B, S, M * D) and out.dtype == dtype
    assert torch.isnan(out).all()
    good = run_fused(value, shapes, lsi, ref, raw)                            # the same inputs with the promised shapes
    assert torch.isfinite(good).all()
    assert_rounded_once(good, want, dtype, FP32_TOL)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_msda_half_softmax_subtracts_the_maximum(dtype):
    """Logits of whole levels shifted by 0, 200, -200 and 1000 (rolled by head): exp(1000) overflows fp32, so a softmax
    without the `- max` term gives inf / inf.  In bfloat16 the logits near 1000 tie exactly after rounding; the oracle sees
    the same rounded values."""
    value, shapes, lsi, ref, raw, _, want, _ = fused_case(7, 12, 20, 8, 16, 1, 1.0, dtype, (0, 200, -200, 1000))
    assert raw.float().max().item() > 900.0 and torch.isfinite(want).all()
    assert_rounded_once(run_fused(value, shapes, lsi, ref, raw), want, dtype, FP32_TOL)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_msda_half_non_finite_logits_stay_in_their_head(dtype):
    """-inf logits (a masked tap: weight exactly 0) on a tenth of the taps; one (query, head) with every logit -inf and one
    with a single +inf (what a 16-bit GEMM overflows to): fp32 softmax gives NaN for exactly these two heads, and the NaN
    must fill their own D channels of their own query and nothing else."""
    c = MSDA_CASES["L3_6x9_M4_D32"]
    value, shapes, lsi, ref, raw, rows, _, _ = named_case("L3_6x9_M4_D32", 1.0, dtype)
    off, logit = fused_plain(raw.float(), rows, c["M"], c["L"])
    logit = logit.clone()
    logit[torch.rand(logit.shape, generator=torch.Generator().manual_seed(12)) < 0.1] = float("-inf")
    logit[0, 5, 1] = float("-inf")
    logit[0, 17, 2, 1, 2] = float("inf")
    raw = repack(off, logit, rows).to(dtype)
    want, _ = fused_oracle(value, shapes, lsi, ref, raw, rows)
    bad = torch.zeros(1, value.shape[1], c["M"], c["D"], dtype=torch.bool)
    bad[0, 5, 1] = True
    bad[0, 17, 2] = True
    bad = bad.flatten(-2)
    assert torch.equal(torch.isnan(want), bad)                                # the oracle: those two heads, nothing else
    out = run_fused(value, shapes, lsi, ref, raw).cpu()
    assert torch.equal(torch.isnan(out), bad)
    assert_rounded_once(out.masked_fill(bad, 0.0), want.masked_fill(bad, 0.0), dtype, FP32_TOL)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_msda_half_non_finite_and_huge_offsets_add_zero(dtype):
    """2 % of the offset entries are +inf, -inf, NaN or the dtype's largest finite value: such a tap lies outside the map, adds
    zero (the kernel's `in ? y : 0.f`: no position is turned into an index unless it is inside) and its logit still takes
    part in the softmax.  The oracle, which casts positions to integers, gets 1e4 px in their place: finite, far outside."""
    c = MSDA_CASES["L2_5x7_M8_D16_B2"]
    value, shapes, lsi, ref, raw, rows, _, _ = named_case("L2_5x7_M8_D16_B2", 1.0, dtype)
    off, logit = fused_plain(raw.float(), rows, c["M"], c["L"])
    n = off.numel()
    k = int(round(0.02 * n)) // 4 * 4
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(13))[:k]
    bad, clean = off.clone().flatten(), off.clone().flatten()
    bad[idx] = torch.tensor([float("inf"), float("-inf"), float("nan"), torch.finfo(dtype).max]).repeat_interleave(k // 4)
    clean[idx] = 1e4
    want, loc = fused_oracle(value, shapes, lsi, ref, repack(clean.view(off.shape), logit, rows), rows)
    assert torch.isfinite(loc).all() and k >= 4
    raw_bad = repack(bad.view(off.shape), logit, rows).to(dtype)
    assert int((~torch.isfinite(raw_bad)).sum()) == 3 * (k // 4)
    out = run_fused(value, shapes, lsi, ref, raw_bad)
    assert torch.isfinite(out).all()
    assert_rounded_once(out, want, dtype, FP32_TOL)


# ---- 2. the converters, on every bit pattern --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def converter_case(dtype):
    """Two 64 x 64 levels, one head of 16 channels, one point: level 0 holds all 65,536 bit patterns (16 per token), level 1
    each pattern + 1 (the next value up in magnitude); NaN and inf patterns become 0 in both (a zero-weight corner on an inf
    neighbour would be NaN).  Query q samples its own texel in both levels.  -> value, shapes, lsi, loc, a, b, keep."""
    pat = torch.arange(65536, dtype=torch.int32)
    a = pat.to(torch.int16).view(dtype)
    b = (pat + 1).to(torch.int16).view(dtype)
    keep = torch.isfinite(a) & torch.isfinite(b)                              # the positions that are compared
    a = torch.where(torch.isfinite(a), a, torch.zeros((), dtype=dtype))
    b = torch.where(torch.isfinite(b), b, torch.zeros((), dtype=dtype))
    value = torch.cat([a.view(4096, 16), b.view(4096, 16)]).view(1, 8192, 1, 16).contiguous()
    shapes = torch.tensor([(64, 64), (64, 64)], dtype=torch.long)
    lsi = torch.tensor([0, 4096], dtype=torch.long)
    q = torch.arange(4096)
    xy = torch.stack([(q % 64).float() + 0.5, (q // 64).float() + 0.5], -1) / 64
    loc = xy.to(dtype)
    # exact in both types, so loc * 64 - 0.5 is the texel's integer index and the blend weights are exactly (1, 0, 0, 0)
    assert torch.equal(loc.float(), xy)
    px = loc.float() * 64 - 0.5
    assert torch.equal(px, torch.stack([q % 64, q // 64], -1).float())
    loc = loc.view(1, 4096, 1, 1, 1, 2).expand(1, 4096, 1, 2, 1, 2).contiguous()
    return value, shapes, lsi, loc, a, b, keep


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("aw", [(1.0, 0.0), (0.5, 0.5), (1.0, 1.0)], ids=["identity", "midpoint", "sum"])
def test_converters_round_every_pattern_to_nearest_even(aw, dtype):
    """F16 / BF16 (csrc/half_types.h, shared by every 16-bit kernel) through msda_fwd_gather_half, bit for bit: `up` then `down`
    is the identity on every finite pattern; the midpoint of two adjacent values is a tie on EVERY element (subnormals and the
    step across a binade included); a + b is a tie one binade up, and the top binade overflows to inf.  All three results are
    exact in fp32, so the expectation is one IEEE rounding (nearest even, subnormals kept) of the fp32 value: no tolerance."""
    MSDA = _msda()
    value, shapes, lsi, loc, a, b, keep = converter_case(dtype)
    w = torch.tensor(aw, dtype=dtype).view(1, 1, 1, 2, 1).expand(1, 4096, 1, 2, 1).contiguous()
    out = MSDA.ms_deform_attn_forward(value.cuda(), shapes.cuda(), lsi.cuda(), loc.cuda(), w.cuda(), 64)
    assert MSDA.last_forward_kernel() == "msda_fwd_gather_half"
    exact = 0.0 + (aw[0] * a.float() + aw[1] * b.float())                     # the accumulator starts at +0: (+0) + (-0) = +0
    exact64, fin = 0.0 + (aw[0] * a.double() + aw[1] * b.double()), torch.isfinite(exact)
    assert torch.equal(exact[fin].double(), exact64[fin])                     # (no rounding before the one under test;
    assert (exact64[~fin].abs() > torch.finfo(torch.float32).max).all()       # bfloat16's top binade leaves fp32 too: inf)
    want = exact.to(dtype).view(torch.int16)
    got = out.cpu().view(65536).view(torch.int16)
    wrong = (got != want) & keep
    first = int(wrong.nonzero()[0]) if wrong.any() else -1
    print(f"{dtype} {aw}: {int(wrong.sum())} of {int(keep.sum())} patterns differ; first {first:#06x}")
    assert keep.sum() == 65536 - (2 * (2 ** (10 if dtype == torch.float16 else 7)) + 2)  # NaN / inf patterns and the one before inf
    assert not wrong.any(), (first, hex(got[first].item() & 0xffff), hex(want[first].item() & 0xffff))
    if aw == (0.5, 0.5):                                                      # (every element IS a tie: the test is not vacuous)
        mid = exact[keep]
        assert ((mid != a.float()[keep]) & (mid != b.float()[keep])).all()
    if aw == (1.0, 1.0):
        assert torch.isinf(exact.to(dtype)[keep]).any()


# ---- 3. add + LayerNorm ---------------------------------------------------------------------------------------------------------
def make_norm(cols, dtype, g):
    norm = nn.LayerNorm(cols)
    with torch.no_grad():
        norm.weight.copy_(1.0 + 0.3 * torch.randn(cols, generator=g))
        norm.bias.copy_(0.3 * torch.randn(cols, generator=g))
    return norm.to(dtype).cuda()


def ln_oracle(x, res, norm):
    s = x.double() if res is None else x.double() + res.double()
    return torch.nn.functional.layer_norm(s, (x.shape[-1],), norm.weight.double().cpu(), norm.bias.double().cpu(), norm.eps)


def at_offset(t, elements):
    """A contiguous CUDA copy of `t` that starts `elements` elements into a larger (512-byte aligned) buffer."""
    if t is None:
        return None
    buf = torch.empty(t.numel() + 64, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[elements:elements + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + elements * t.element_size()
    return v


def ln_inputs(B, rows, cols, dtype, with_res, with_add, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, rows, cols, generator=g) * 3 + 0.7).to(dtype)
    res = (torch.randn(B, rows, cols, generator=g) * 0.5).to(dtype) if with_res else None
    pos = torch.randn(1, rows, cols, generator=g).to(dtype) if with_add else None     # rows of ONE batch element
    return x, res, pos, make_norm(cols, dtype, g)


def check_ln(got, want, pos, dtype, floor=LN_FP32_TOL):
    if pos is not None:
        got, got2 = got
        assert_rounded_once(got2, want + pos.double(), dtype, floor)         # from the UNROUNDED row: one rounding
    assert_rounded_once(got, want, dtype, floor)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", [64, 128, 256])
@pytest.mark.parametrize("with_res,with_add", [(True, True), (True, False), (False, True), (False, False)])
def test_add_layer_norm_half_without_16_byte_alignment(dtype, cols, with_res, with_add):
    """add_layernorm_rows_half<COLS, COLS / 64> (one row per wave): every input starts cols / 64 elements into its buffer --
    the C entry's minimum alignment, a lane's cols / 64 elements as one access, but not 16 bytes.  The reduction order is not
    the aligned instantiation's, so the comparison is with the oracle."""
    from mvdetr_amd.ops.add_layernorm import add_layer_norm, fused_add_layer_norm_available, last_kernel
    x, res, pos, norm = ln_inputs(2, 37, cols, dtype, with_res, with_add, 37 + cols)
    xo, ro, po = (at_offset(t, cols // 64) for t in (x, res, pos))
    for t in (xo, ro, po):                                                    # the condition that selects the instantiation
        assert t is None or (t.data_ptr() % 16 != 0 and t.data_ptr() % (cols // 64 * 2) == 0)
    with torch.no_grad():
        assert fused_add_layer_norm_available(xo, norm)
        got = add_layer_norm(xo, ro, norm, then_add=po)
    assert last_kernel() == f"add_layernorm_rows_half<{cols},{cols // 64}>"
    check_ln(got, ln_oracle(x, res, norm), pos, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", [128, 256])
def test_add_layer_norm_half_below_the_minimum_alignment_runs_torch_ops(dtype, cols):
    """Inputs one element (2 bytes) into their buffers: below the C entry's minimum alignment (hipErrorNotSupported there).
    add_layer_norm must not raise: it returns what the module's own torch ops return -- norm(x + residual), a rounding after
    every step, so against the fp64 oracle the bar is wider than the fused kernel's: the output's rounding, the rounding
    of y + then_add's first operand, and the rounding of the sum s = x + residual (|ds| <= ulp max|s| along the row) carried
    through the normalisation to first order: |dy| <= ulp max|s| rstd |gamma| (2 + |n|), n the normalised element -- its own
    and the mean's share, and the variance's share times n."""
    from mvdetr_amd.ops.add_layernorm import add_layer_norm
    x, res, pos, norm = ln_inputs(2, 37, cols, dtype, True, True, 41 + cols)
    xo, ro, po = (at_offset(t, 1) for t in (x, res, pos))
    assert xo.data_ptr() % (cols // 64 * 2) != 0
    with torch.no_grad():
        got, got2 = add_layer_norm(xo, ro, norm, then_add=po)
        y = norm(xo + ro)
        assert torch.equal(got, y) and torch.equal(got2, y + po)
    s = x.double() + res.double()
    want = ln_oracle(x, res, norm)
    ulp = ulp_of(dtype)
    rstd = (s.var(-1, unbiased=False, keepdim=True) + norm.eps).rsqrt()
    n = (s - s.mean(-1, keepdim=True)) * rstd
    carried = ulp * s.abs().amax(-1, keepdim=True) * rstd * norm.weight.double().cpu().abs() * (2 + n.abs())
    err = (got.cpu().double() - want).abs()
    assert (err <= ulp * want.abs() + carried + LN_FP32_TOL).all(), err.max().item()
    err2 = (got2.cpu().double() - (want + pos.double())).abs()
    assert (err2 <= ulp * (want + pos.double()).abs() + ulp * want.abs() + carried + LN_FP32_TOL).all(), err2.max().item()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", [64, 128, 256])
def test_add_layer_norm_half_grid_stride(dtype, cols):
    """More rows than 4096 workgroups hold (4 waves of 512 / cols rows each): the grid-stride loop of the aligned instantiation,
    and -- the same rows at an offset of cols / 64 elements, one row per wave -- of the unaligned one."""
    from mvdetr_amd.ops.add_layernorm import add_layer_norm, last_kernel
    rows = 4096 * 4 * (512 // cols) + 37
    assert -(-rows // (4 * (512 // cols))) > 4096 and -(-rows // 4) > 4096     # the launcher's block counts, both instantiations
    x, res, pos, norm = ln_inputs(1, rows, cols, dtype, True, True, 43 + cols)
    want = ln_oracle(x, res, norm)
    with torch.no_grad():
        aligned = add_layer_norm(x.cuda(), res.cuda(), norm, then_add=pos.cuda())
        assert last_kernel() == f"add_layernorm_rows_half<{cols},8>"
        check_ln(aligned, want, pos, dtype)
        del aligned
        check_ln(add_layer_norm(*(at_offset(t, cols // 64) for t in (x, res)), norm, then_add=at_offset(pos, cols // 64)),
                 want, pos, dtype)
        assert last_kernel() == f"add_layernorm_rows_half<{cols},{cols // 64}>"


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_layer_norm_half_constant_rows_give_beta(dtype):
    """Rows of one value each (x + residual constant along the row, a multiple of 1/16 below 32: every partial sum of the row is
    exact in fp32): the mean is exact, every centred element is exactly 0, and the output is beta, bit for bit."""
    from mvdetr_amd.ops.add_layernorm import add_layer_norm
    g = torch.Generator().manual_seed(44)
    rows, cols = 64, 128
    x = (torch.randn(1, rows, 1, generator=g) * 24).round().div(8).to(dtype).expand(1, rows, cols).contiguous()      # eighths
    res = (torch.randn(1, rows, 1, generator=g) * 8).round().div(16).to(dtype).expand(1, rows, cols).contiguous()   # sixteenths
    assert torch.equal(x.double() * 16, (x.double() * 16).round()) and x.abs().max() < 16 and x.abs().max() > 1
    norm = make_norm(cols, dtype, g)
    with torch.no_grad():
        for r in (None, res):
            got = add_layer_norm(x.cuda(), None if r is None else r.cuda(), norm)
            assert torch.equal(got.view(torch.int16), norm.bias.detach().expand(1, rows, cols).contiguous().view(torch.int16))


def test_add_layer_norm_half_sum_leaves_float16_range():
    """float16 rows with |x| and |residual| near 4e4 and equal signs: x + residual (up to ~9e4) is beyond float16's largest
    finite value (65504) but an ordinary fp32 number; a kernel that rounded the sum to storage would return inf / NaN."""
    from mvdetr_amd.ops.add_layernorm import add_layer_norm
    dtype, rows, cols = torch.float16, 64, 128
    g = torch.Generator().manual_seed(45)
    sign = torch.where(torch.rand(1, rows, cols, generator=g) < 0.5, -1.0, 1.0)
    x = (sign * (4e4 + 2e3 * torch.randn(1, rows, cols, generator=g))).to(dtype)
    res = (sign * (4e4 + 2e3 * torch.randn(1, rows, cols, generator=g))).to(dtype)
    pos = torch.randn(1, rows, cols, generator=g).to(dtype)
    norm = make_norm(cols, dtype, g)
    assert torch.isfinite(x).all() and torch.isfinite(res).all() and (x.float() + res.float()).abs().max() > 65504
    with torch.no_grad():
        got = add_layer_norm(x.cuda(), res.cuda(), norm, then_add=pos.cuda())
    check_ln(got, ln_oracle(x, res, norm), pos, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_layer_norm_half_large_mean(dtype):
    """Rows with mean 1000 and unit noise: the cancellation in v - mean amplifies fp32 rounding beyond the 5e-6 floor of the
    N(0.7, 3) rows, whatever the order of the sums.  The floor becomes 5e-6 + 2 |LN_fp32(upcast inputs) - ref64| elementwise:
    the fp32 composition's own distance from fp64 (torch's CPU layer_norm on the fp32 sum), doubled for another summation
    order.  Elementwise bar only.
    Measured on MI355X, worst err - bar of out / out2 (negative = inside the bar): float16 -6.6e-6 / -7.6e-6, bfloat16
    -7.6e-6 / -1.5e-5.  A kernel that forms v = x + residual in fp32 and centres v - sum(v) / COLS misses it by 6.5e-5 in
    float16 and 2.1e-5 in bfloat16 (the roundings of the total and of v scale with the mean, not the spread)."""
    from mvdetr_amd.ops.add_layernorm import add_layer_norm
    rows, cols = 64, 128
    g = torch.Generator().manual_seed(46)
    x = (1000.0 + torch.randn(1, rows, cols, generator=g)).to(dtype)
    res = (torch.randn(1, rows, cols, generator=g) * 0.5).to(dtype)
    pos = torch.randn(1, rows, cols, generator=g).to(dtype)
    norm = make_norm(cols, dtype, g)
    want = ln_oracle(x, res, norm)
    ref32 = torch.nn.functional.layer_norm(x.float() + res.float(), (cols,), norm.weight.float().cpu(), norm.bias.float().cpu(),
                                           norm.eps)
    extra = 2 * (ref32.double() - want).abs()
    with torch.no_grad():
        got, got2 = add_layer_norm(x.cuda(), res.cuda(), norm, then_add=pos.cuda())
    worst = []
    for o, w in ((got, want), (got2, want + pos.double())):
        err = (o.cpu().double() - w).abs()
        bar = ulp_of(dtype) * w.abs() + LN_FP32_TOL + extra
        worst.append((err - bar).max().item())
        print(f"large mean {dtype}: max |err| {err.max().item():.3e}, max (err - bar) {worst[-1]:.3e}, "
              f"max extra {extra.max().item():.3e}, row std min {(x.double() + res.double()).std(-1).min().item():.3f}")
    assert max(worst) <= 0.0, worst


# ---- 4. warp: channel counts and alignment ------------------------------------------------------------------------------------
def _warp():
    from mvdetr_amd.ops import warp
    return warp


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("channels", [8, 72, 200])
def test_warp_channel_last_chunk_counts(dtype, channels):
    """warp_fwd_cl_half at 1, 9 and 25 16-byte chunks per pixel: no power of two divides the 256 lanes' items evenly."""
    warp = _warp()
    src, M, _, _ = warp_case(dtype, channels, "bilinear")
    x = src.cuda().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        out = warp.warp_perspective(x, M, DST_HW, channels_last_out=True)
    assert warp.last_kernel() == "warp_fwd_cl_half"
    assert out.shape == (N_VIEWS, *DST_HW, channels)
    check_warp(out.permute(0, 3, 1, 2), dtype, channels)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cl_out", [True, False])
@pytest.mark.parametrize("channels,cl_src", [(65, False), (130, False), (12, True)])
def test_warp_generic_kernel_ragged_channel_groups(dtype, channels, cl_src, cl_out):
    """warp_fwd_half with a ragged last group of 64 channels (65: one channel in it; 130: two) from an NCHW source, and with a
    channel-last source of 24-byte pixels, which the 16-byte kernel does not take."""
    warp = _warp()
    src, M, _, _ = warp_case(dtype, channels, "bilinear")
    x = src.cuda().contiguous(memory_format=torch.channels_last) if cl_src else src.cuda()
    with torch.no_grad():
        out = warp.warp_perspective(x, M, DST_HW, channels_last_out=cl_out)
    assert warp.last_kernel() == "warp_fwd_half"
    check_warp(out.permute(0, 3, 1, 2) if cl_out else out, dtype, channels)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cl_out", [True, False])
def test_warp_misaligned_channel_last_source(dtype, cl_out):
    """A 64-channel channel-last source that starts 8 bytes into its buffer: not the 16-byte kernel's, so warp_fwd_half runs --
    with the values of the aligned call (the same fp32 blend of the same four texels, rounded once)."""
    warp = _warp()
    src, M, _, _ = warp_case(dtype, 64, "bilinear")
    n, c, h, w = src.shape
    buf = torch.empty(src.numel() + 8, dtype=dtype, device="cuda")
    x = buf[4:4 + src.numel()].view(n, h, w, c).permute(0, 3, 1, 2)
    x.copy_(src)
    assert x.data_ptr() % 16 == 8 and x.is_contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        out = warp.warp_perspective(x, M, DST_HW, channels_last_out=cl_out)
        assert warp.last_kernel() == "warp_fwd_half"
        aligned = warp.warp_perspective(src.cuda().contiguous(memory_format=torch.channels_last), M, DST_HW, channels_last_out=cl_out)
        assert warp.last_kernel() == ("warp_fwd_cl_half" if cl_out else "warp_fwd_half")
    check_warp(out.permute(0, 3, 1, 2) if cl_out else out, dtype, 64)
    assert torch.equal(out, aligned)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("channels,cl", [(64, True), (3, False)])
def test_warp_degenerate_sizes(dtype, channels, cl):
    """A 1 x 1 destination (destination pixel (0, 0) does not depend on the destination's size: the oracle's own pixel (0, 0)),
    a 1 x 1 source (kornia's corner-aligned normalisation divides by size - 1, 1e-14 in its place: under the identity,
    destination pixel (0, 0) lands on x = y = -0.5 and blends a quarter of the texel with the zero padding, every other
    pixel is far outside) and no views at all."""
    warp = _warp()
    src, M, ref64, ref32 = warp_case(dtype, channels, "bilinear")
    x = src.cuda().contiguous(memory_format=torch.channels_last) if cl else src.cuda()
    nchw = (lambda o: o.permute(0, 3, 1, 2)) if cl else (lambda o: o)
    with torch.no_grad():
        one = warp.warp_perspective(x, M, (1, 1), channels_last_out=cl)
        assert warp.last_kernel() == ("warp_fwd_cl_half" if cl else "warp_fwd_half")
        assert one.shape == ((N_VIEWS, 1, 1, channels) if cl else (N_VIEWS, channels, 1, 1))
        want = ref64[:, :, :1, :1]
        assert_rounded_once(nchw(one), want, dtype, FP32_TOL, extra=1.5 * (ref32[:, :, :1, :1].double() - want).abs())
        assert want[0].abs().max() > 0.1                                      # (the near-identity view samples the source there)

        texel = x[:2, :, 7:8, 9:10]                                           # a 1 x 1 source, two views
        eye_away = torch.stack([torch.eye(3), warp_mats()[2]])
        tiny = nchw(warp.warp_perspective(texel, eye_away, DST_HW, channels_last_out=cl))
        assert warp.last_kernel() == "warp_fwd_half"
        # (worked out by hand: through the 1e-14 the oracles' matrix inverses lose every digit of this position)
        want = torch.zeros(2, channels, *DST_HW, dtype=torch.float64)
        want[0, :, 0, 0] = 0.25 * src[0, :, 7, 9].double()
        assert tiny.shape == want.shape and want.abs().max() > 0.1
        assert torch.equal(tiny.cpu().double(), want.to(dtype).double())      # a quarter of a 16-bit value: exact in 16 bits

        none = warp.warp_perspective(x[:0], M[:0], DST_HW, channels_last_out=cl)
        assert none.shape == ((0, *DST_HW, channels) if cl else (0, channels, *DST_HW)) and none.dtype == dtype
