"""GPU parity tests of multi-scale deformable attention: HIP kernels (through the product API and
the C ABI) against the oracle, the golden vectors produced by the reference, and size-independent
properties at the full Wildtrack shape.  Tolerance for fp32: 1e-4 absolute on O(1) features
(BASELINE.json north_star); fp64: torch.allclose defaults like ops/test.py:40."""
import pytest
import torch

from conftest import load_golden, t
from helpers import encoder_msda_inputs, level_start_index, random_msda_inputs
from oracle import c_oracle, torch_oracle

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4


@pytest.fixture(scope="module")
def ops():
    import mvdetr_amd.ops  # noqa: F401
    from mvdetr_amd.ops.functions import MSDeformAttnFunction
    import MultiScaleDeformableAttention as MSDA
    return MSDeformAttnFunction, MSDA


def dev(*xs):
    return [x.cuda() for x in xs]


def run_fwd(ops, value, shapes, lsi, loc, aw, step=64):
    F, _ = ops
    return F.apply(*dev(value, shapes, lsi, loc, aw), step).cpu()


# ---- golden vectors ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_forward_testpy_golden(ops, tag):
    g = load_golden(f"msda_testpy_{tag}.npz")
    out = run_fwd(ops, t(g["value"]), t(g["shapes"]), t(g["level_start_index"]), t(g["loc"]), t(g["aw"]), 2)
    ref = t(g["out"])
    if tag == "f64":
        assert torch.allclose(out, ref)
        assert (out - ref).abs().max().item() < 1e-15
    else:
        assert torch.allclose(out, ref, rtol=1e-2, atol=1e-3)       # the reference's own bar (test.py:56)
        assert (out - ref).abs().max().item() < 1e-8                 # ours (values are ~0.01)


def test_forward_mini_golden(ops):
    g = load_golden("msda_mini.npz")
    args = [t(g[k]) for k in ("value", "shapes", "level_start_index", "loc", "aw")]
    out32 = run_fwd(ops, *args)
    assert (out32 - t(g["out_f32"])).abs().max().item() < FP32_TOL
    assert (out32.double() - t(g["out"])).abs().max().item() < FP32_TOL
    out64 = run_fwd(ops, args[0].double(), args[1], args[2], args[3].double(), args[4].double())
    assert (out64 - t(g["out"])).abs().max().item() < 1e-12


def test_forward_edges_golden(ops):
    g = load_golden("msda_edges.npz")
    args = [t(g[k]) for k in ("value", "shapes", "level_start_index", "loc", "aw")]
    assert (run_fwd(ops, *args) - t(g["out"])).abs().max().item() < 1e-12
    out32 = run_fwd(ops, args[0].float(), args[1], args[2], args[3].float(), args[4].float())
    assert (out32.double() - t(g["out"])).abs().max().item() < FP32_TOL


def test_backward_mini_golden(ops):
    _, MSDA = ops
    g = load_golden("msda_mini.npz")
    v, s, lsi, loc, aw, go = [t(g[k]) for k in ("value", "shapes", "level_start_index", "loc", "aw", "grad_out")]
    gv, gl, ga = [x.cpu() for x in MSDA.ms_deform_attn_backward(
        *dev(v.double(), s, lsi, loc.double(), aw.double(), go.double()), 64)]
    assert (gv - t(g["grad_value"])).abs().max().item() < 1e-11
    assert (gl - t(g["grad_loc"])).abs().max().item() < 1e-10
    assert (ga - t(g["grad_aw"])).abs().max().item() < 1e-11
    gv, gl, ga = [x.cpu().double() for x in MSDA.ms_deform_attn_backward(*dev(v, s, lsi, loc, aw, go), 64)]
    assert (gv - t(g["grad_value"])).abs().max().item() < 1e-4
    assert (ga - t(g["grad_aw"])).abs().max().item() < 1e-4
    # grad_loc carries a factor W (or H) and a D-term sum: relative bar
    ref = t(g["grad_loc"])
    assert ((gl - ref).abs() / (1 + ref.abs())).max().item() < 1e-4


# ---- random shapes against the oracle -----------------------------------------------------------------
SHAPES = [
    # B, levels, M, D, Lq, P
    (1, [(6, 4), (3, 2)], 2, 2, 2, 2),                       # ops/test.py
    (2, [(8, 8), (4, 4), (2, 2), (1, 1)], 8, 32, 37, 4),     # Deformable-DETR-like pyramid
    (1, [(5, 7)] * 3, 4, 16, 105, 4),                        # small MVDeTr-like (Lq == S)
    (3, [(9, 11), (3, 5)], 1, 1, 13, 1),                     # scalar channels, single head/point
    (2, [(7, 3)], 3, 30, 5, 3),                              # D not a multiple of 4
    (1, [(4, 4), (6, 2)], 2, 71, 9, 2),                      # odd D
    (1, [(3, 3)], 1, 1025, 3, 1),                            # D > 1024 (reference's multi-block path)
    (1, [(5, 9)] * 6, 8, 16, 270, 4),                        # MultiviewX-like
    (1, [(4, 6)] * 16, 8, 32, 384, 4),                       # 16 cameras, 256 channels
]


@pytest.mark.parametrize("B,lv,M,D,Lq,P", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_forward_vs_oracle(ops, B, lv, M, D, Lq, P, dtype):
    value, shapes, lsi, loc, aw = random_msda_inputs(B, lv, M, D, Lq, P, seed=B + D + Lq, dtype=dtype)
    out = run_fwd(ops, value, shapes, lsi, loc, aw, step=B)
    ref64 = c_oracle.msda_forward(value.double(), shapes, lsi, loc.double(), aw.double())
    tol = FP32_TOL if dtype == torch.float32 else 1e-12
    assert out.shape == (B, Lq, M * D)
    assert (out.double() - ref64).abs().max().item() < tol
    if dtype == torch.float32:          # and against the fp32 torch formulation the reference falls back to
        assert (out - torch_oracle.msda_core(value, shapes, loc, aw)).abs().max().item() < FP32_TOL


@pytest.mark.parametrize("B,lv,M,D,Lq,P", SHAPES)
def test_backward_vs_oracle(ops, B, lv, M, D, Lq, P):
    _, MSDA = ops
    value, shapes, lsi, loc, aw = random_msda_inputs(B, lv, M, D, Lq, P, seed=7 + D, dtype=torch.float64)
    go = torch.randn(B, Lq, M * D, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    ref = c_oracle.msda_backward(value, shapes, lsi, loc, aw, go)
    got = [x.cpu() for x in MSDA.ms_deform_attn_backward(*dev(value, shapes, lsi, loc, aw, go), B)]
    for a, b, name in zip(got, ref, ("grad_value", "grad_loc", "grad_aw")):
        assert a.shape == b.shape
        assert ((a - b).abs() / (1 + b.abs())).max().item() < 1e-10, name
    got32 = [x.cpu().double() for x in MSDA.ms_deform_attn_backward(
        *dev(value.float(), shapes, lsi, loc.float(), aw.float(), go.float()), B)]
    for a, b, name in zip(got32, ref, ("grad_value", "grad_loc", "grad_aw")):
        assert ((a - b).abs() / (1 + b.abs())).max().item() < 2e-4 * max(1.0, D / 64), name


@pytest.mark.parametrize("channels", [30, 32, 64, 71, 1025, 2048, 3096])
def test_gradcheck_channel_sweep(ops, channels):
    """ops/test.py:63-86: gradcheck in fp64 over the D values that select every backward variant."""
    F, _ = ops
    N, M, Lq, L, P = 1, 2, 2, 2, 2
    shapes = torch.as_tensor([(6, 4), (3, 2)], dtype=torch.long)
    S = int(shapes.prod(1).sum())
    torch.manual_seed(3)
    value = (torch.rand(N, S, M, channels) * 0.01).double().cuda().requires_grad_(True)
    loc = torch.rand(N, Lq, M, L, P, 2).double().cuda().requires_grad_(True)
    aw = torch.rand(N, Lq, M, L, P) + 1e-5
    aw = (aw / aw.sum((-1, -2), keepdim=True)).double().cuda().requires_grad_(True)
    assert torch.autograd.gradcheck(F.apply, (value, shapes.cuda(), level_start_index(shapes).cuda(), loc, aw, 2))


def test_autograd_through_function_matches_oracle_autograd(ops):
    F, _ = ops
    value, shapes, lsi, loc, aw = random_msda_inputs(2, [(6, 5), (3, 4)], 4, 16, 21, 4, seed=5, dtype=torch.float64)
    leaves = [x.clone().requires_grad_(True) for x in (value, loc, aw)]
    out_ref = torch_oracle.msda_core(leaves[0], shapes, leaves[1], leaves[2])
    go = torch.randn(out_ref.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    ref = torch.autograd.grad(out_ref, leaves, go)
    dl = [x.clone().cuda().requires_grad_(True) for x in (value, loc, aw)]
    out = F.apply(dl[0], shapes.cuda(), lsi.cuda(), dl[1], dl[2], 64)
    got = torch.autograd.grad(out, dl, go.cuda())
    for a, b in zip(got, ref):
        assert (a.cpu() - b).abs().max().item() < 1e-10


# ---- ragged / empty / misuse ----------------------------------------------------------------------------
def test_empty_queries_and_batch(ops):
    F, MSDA = ops
    value, shapes, lsi, loc, aw = random_msda_inputs(2, [(4, 4)], 2, 8, 0, 2)
    out = run_fwd(ops, value, shapes, lsi, loc, aw)
    assert out.shape == (2, 0, 16)
    gv, gl, ga = MSDA.ms_deform_attn_backward(*dev(value, shapes, lsi, loc, aw, out), 64)
    assert gv.shape == value.shape and float(gv.abs().sum()) == 0.0 and gl.numel() == 0 and ga.numel() == 0


def test_all_taps_outside_give_zero(ops):
    value, shapes, lsi, loc, aw = random_msda_inputs(1, [(4, 5), (2, 3)], 2, 16, 11, 4, lo=1.5, hi=3.0)
    assert float(run_fwd(ops, value, shapes, lsi, loc, aw).abs().max()) == 0.0
    value, shapes, lsi, loc, aw = random_msda_inputs(1, [(4, 5), (2, 3)], 2, 16, 11, 4, lo=-3.0, hi=-0.6)
    assert float(run_fwd(ops, value, shapes, lsi, loc, aw).abs().max()) == 0.0


def test_nan_locations_do_not_fault(ops):
    value, shapes, lsi, loc, aw = random_msda_inputs(1, [(4, 5)], 2, 16, 8, 2)
    loc[0, 3] = float("nan")
    out = run_fwd(ops, value, shapes, lsi, loc, aw)
    ref = torch_oracle.msda_core(value, shapes, loc, aw)
    keep = [i for i in range(8) if i != 3]
    assert (out[0, keep] - ref[0, keep]).abs().max().item() < FP32_TOL
    assert float(out[0, 3].abs().max()) == 0.0          # the > -1 / < size guard rejects NaN (cuh:288)


def test_misuse_raises_like_reference(ops):
    F, MSDA = ops
    value, shapes, lsi, loc, aw = dev(*random_msda_inputs(3, [(4, 4)], 2, 8, 5, 2))
    with pytest.raises(RuntimeError, match="must divide im2col_step"):
        MSDA.ms_deform_attn_forward(value, shapes, lsi, loc, aw, 2)
    with pytest.raises(RuntimeError, match="sampling_loc tensor has to be contiguous"):
        MSDA.ms_deform_attn_forward(value, shapes, lsi, loc.transpose(1, 2).contiguous().transpose(1, 2), aw, 3)
    with pytest.raises(RuntimeError, match="spatial_shapes must be a CUDA tensor"):
        MSDA.ms_deform_attn_forward(value, shapes.cpu(), lsi, loc, aw, 3)
    with pytest.raises(RuntimeError, match="not implemented for"):       # AT_DISPATCH_FLOATING_TYPES, cu:64 (the forward takes
        MSDA.ms_deform_attn_forward(value.to(torch.int32), shapes, lsi, loc, aw, 3)   # fp16/bf16 here: an extension, tested below)
    with pytest.raises(RuntimeError, match="same dtype"):
        MSDA.ms_deform_attn_forward(value.half(), shapes, lsi, loc, aw, 3)


def test_inputs_are_not_mutated_and_stream_is_respected(ops):
    F, _ = ops
    args = dev(*random_msda_inputs(1, [(6, 6)] * 2, 4, 16, 72, 4, seed=3))
    before = [a.clone() for a in args]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out_side = F.apply(*args, 64)
    side.synchronize()
    out_main = F.apply(*args, 64)
    torch.cuda.synchronize()
    assert torch.equal(out_side, out_main)
    for a, b in zip(args, before):
        assert torch.equal(a, b)


# ---- module level ------------------------------------------------------------------------------------------
def test_module_golden(ops):
    from mvdetr_amd.ops.modules import MSDeformAttn
    g = load_golden("msda_module.npz")
    d_model, L, M, P = (int(x) for x in g["dims"])
    mod = MSDeformAttn(d_model, L, M, P)
    mod.load_state_dict({k[2:]: t(v) for k, v in g.items() if k.startswith("p.")})
    mod = mod.cuda()
    shapes = t(g["shapes"]).cuda()
    out = mod(t(g["query"]).cuda(), t(g["ref"]).cuda(), t(g["src"]).cuda(), shapes, level_start_index(shapes))
    assert (out.cpu() - t(g["out"])).abs().max().item() < FP32_TOL
    # 4-D reference points are not part of MVDeTr's contract (ms_deform_attn.py:106 indexes 5-D)
    with pytest.raises(IndexError):
        mod(t(g["query"]).cuda(), t(g["ref"]).cuda()[:, :, :, 0], t(g["src"]).cuda(), shapes, level_start_index(shapes))


# ---- full Wildtrack shape ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wildtrack_inputs():
    return encoder_msda_inputs(7, 60, 180, seed=0)


def test_wildtrack_forward_vs_oracle(ops, wildtrack_inputs):
    value, shapes, lsi, loc, aw = wildtrack_inputs
    out = run_fwd(ops, value, shapes, lsi, loc, aw)
    ref = c_oracle.msda_forward(value, shapes, lsi, loc, aw)          # fp32 C oracle, all 75,600 queries
    assert (out - ref).abs().max().item() < FP32_TOL
    sub = slice(0, 75600, 97)                                         # fp64 truth on a strided subset
    ref64 = c_oracle.msda_forward(value.double(), shapes, lsi, loc[:, sub].double().contiguous(),
                                  aw[:, sub].double().contiguous())
    assert (out[:, sub].double() - ref64).abs().max().item() < FP32_TOL


def test_wildtrack_adversarial_uniform_locations(ops):
    value, shapes, lsi, loc, aw = random_msda_inputs(1, [(60, 180)] * 7, 8, 16, 75600, 4, seed=1, lo=0.0, hi=1.0)
    out = run_fwd(ops, value, shapes, lsi, loc, aw)
    ref = c_oracle.msda_forward(value, shapes, lsi, loc, aw)
    assert (out - ref).abs().max().item() < FP32_TOL


def test_wildtrack_linearity_and_weight_scaling(ops, wildtrack_inputs):
    """Size-independent properties: the op is linear in value and in the attention weights."""
    value, shapes, lsi, loc, aw = dev(*wildtrack_inputs)
    F, _ = ops
    v2 = torch.randn_like(value)
    a = F.apply(value, shapes, lsi, loc, aw, 64)
    b = F.apply(v2, shapes, lsi, loc, aw, 64)
    ab = F.apply(2 * value - 3 * v2, shapes, lsi, loc, 0.5 * aw, 64)
    assert (ab - 0.5 * (2 * a - 3 * b)).abs().max().item() < 2e-5
    # constant value field + weights that sum to 1 and taps well inside => output == the constant
    ones = torch.ones_like(value)
    inside = (loc * 0.5 + 0.25).contiguous()
    out = F.apply(ones, shapes, lsi, inside, aw, 64)
    assert (out - 1).abs().max().item() < 1e-5


def test_wildtrack_backward_checksums(ops, wildtrack_inputs):
    """sum(grad_value) == sum over taps of aw * in-bounds bilinear mass * grad_out, checked through
    the identity <grad_out, f(value)> == <grad_value, value> (adjoint test), at full size."""
    _, MSDA = ops
    F, _ = ops
    value, shapes, lsi, loc, aw = dev(*wildtrack_inputs)
    go = torch.randn(1, 75600, 128, device="cuda")
    gv, gl, ga = MSDA.ms_deform_attn_backward(value, shapes, lsi, loc, aw, go, 64)
    out = F.apply(value, shapes, lsi, loc, aw, 64)
    lhs = (go.double() * out.double()).sum().item()
    rhs = (gv.double() * value.double()).sum().item()
    # (grad_value comes from per-tile fixed-point windows whose step is ~1e-9 of the largest |grad_out|,
    # msda_backward_tile.hip: as tight as with fp32 atomics)
    assert abs(lhs - rhs) < 1e-6 * (abs(lhs) + 1e3)
    # <grad_aw, aw> == <grad_out, out> as well (out is linear in aw)
    rhs2 = (ga.double() * aw.double()).sum().item()
    assert abs(lhs - rhs2) < 1e-6 * (abs(lhs) + 1e3)
    # and a strided subset of grad_loc / grad_aw against the fp64 oracle
    sub = slice(0, 75600, 997)
    lo, awc, goc = [x[:, sub].cpu().double().contiguous() for x in (loc, aw, go)]
    _, rl, ra = c_oracle.msda_backward(value.cpu().double(), shapes.cpu(), lsi.cpu(), lo, awc, goc)
    # grad_loc = W * a * sum_c g_c * dv_c: |terms| sum to ~1e2 at W = 180, so fp32 rounding is ~1e-5..1e-4
    err = (gl[:, sub].cpu().double() - rl).abs()
    assert err.max().item() / rl.abs().max().item() < 1e-5
    assert (err / (50 + rl.abs())).max().item() < 1e-4
    # grad_aw is the un-weighted tap value dotted with grad_out: a 1.5e-5 px fp32 rounding of loc*W at
    # W = 180 times a slope of up to ~10 per px gives ~1e-4 absolute on values of magnitude ~10
    erra = (ga[:, sub].cpu().double() - ra).abs()
    assert erra.max().item() / ra.abs().max().item() < 1e-4
    assert (erra / (1 + ra.abs())).max().item() < 5e-4


# ---- the LDS-tiled encoder kernel vs the gather kernel vs the oracle ------------------------------------------
@pytest.fixture
def msda_impl(ops):
    _, MSDA = ops
    yield MSDA
    MSDA.set_forward_impl("auto")


def _fwd_impl(MSDA, impl, args):
    MSDA.set_forward_impl(impl)
    out = MSDA.ms_deform_attn_forward(*dev(*args), 64).cpu()
    return out, MSDA.last_forward_impl()


TILE_CASES = {
    "mvdetr_like_partial_tiles": lambda: encoder_msda_inputs(7, 21, 43, seed=2, noise_px=1.0),
    "multiviewx_like": lambda: encoder_msda_inputs(6, 20, 31, seed=3, noise_px=1.0),
    "wide_offsets_many_misses": lambda: encoder_msda_inputs(3, 24, 40, seed=4, noise_px=6.0),
    "batch2": lambda: encoder_msda_inputs(4, 17, 19, B=2, seed=5),
    "d32_16cams": lambda: encoder_msda_inputs(16, 9, 33, M=8, D=32, seed=6),
    "single_level": lambda: encoder_msda_inputs(1, 30, 50, seed=7),
    "m2": lambda: encoder_msda_inputs(5, 12, 18, M=2, D=16, seed=8),
}


@pytest.mark.parametrize("case", sorted(TILE_CASES))
def test_tile_kernel_vs_gather_and_oracle(msda_impl, case):
    args = TILE_CASES[case]()
    tile, used = _fwd_impl(msda_impl, "tile", args)
    assert used == "tile"
    gather, used = _fwd_impl(msda_impl, "gather", args)
    assert used == "gather"
    ref = c_oracle.msda_forward(*[a.double() if a.is_floating_point() else a for a in args])
    assert (tile.double() - ref).abs().max().item() < FP32_TOL
    assert (gather.double() - ref).abs().max().item() < FP32_TOL
    assert (tile - gather).abs().max().item() < 2e-5          # same taps, different summation order


def test_tile_kernel_unequal_levels(msda_impl):
    from helpers import pyramid_encoder_inputs
    args = pyramid_encoder_inputs([(24, 36), (12, 18), (6, 9), (3, 5)], M=8, D=32, seed=9)
    tile, used = _fwd_impl(msda_impl, "tile", args)
    assert used == "tile"
    ref = c_oracle.msda_forward(*[a.double() if a.is_floating_point() else a for a in args])
    assert (tile.double() - ref).abs().max().item() < FP32_TOL
    args = pyramid_encoder_inputs([(10, 37), (20, 11), (7, 7)], M=4, D=16, seed=10, noise_px=3.0)
    tile, used = _fwd_impl(msda_impl, "tile", args)
    assert used == "tile"
    ref = c_oracle.msda_forward(*[a.double() if a.is_floating_point() else a for a in args])
    assert (tile.double() - ref).abs().max().item() < FP32_TOL


def test_tile_kernel_adversarial_and_edge_locations(msda_impl):
    # uniform locations: nearly every tap leaves its window -> the deferred global path does the work
    args = random_msda_inputs(1, [(40, 64)] * 3, 8, 16, 3 * 40 * 64, 4, seed=11, lo=-0.1, hi=1.1)
    tile, used = _fwd_impl(msda_impl, "tile", args)
    assert used == "tile"
    ref = c_oracle.msda_forward(*[a.double() if a.is_floating_point() else a for a in args])
    assert (tile.double() - ref).abs().max().item() < FP32_TOL
    # NaN / inf / huge locations must take the guarded path, not index LDS
    value, shapes, lsi, loc, aw = encoder_msda_inputs(3, 16, 32, seed=12)
    loc[0, 5] = float("nan")
    loc[0, 6] = float("inf")
    loc[0, 7] = -1e30
    loc[0, 8, :, :, :, 0] = 1e30
    tile, _ = _fwd_impl(msda_impl, "tile", (value, shapes, lsi, loc, aw))
    ref = torch_oracle.msda_core(value, shapes, loc, aw)
    keep = torch.ones(loc.shape[1], dtype=torch.bool)
    keep[5:9] = False
    assert (tile[0, keep] - ref[0, keep]).abs().max().item() < FP32_TOL
    assert float(tile[0, 5:9].abs().max()) == 0.0


def test_auto_dispatch_rules(msda_impl):
    MSDA = msda_impl
    MSDA.set_forward_impl("auto")
    args = encoder_msda_inputs(7, 16, 24, seed=1)
    MSDA.ms_deform_attn_forward(*dev(*args), 64)
    assert MSDA.last_forward_impl() == "tile" and MSDA.last_forward_kernel().startswith("msda_fwd_group2")
    # decoder-style call (Lq != S), fp64, D = 30, P != 4: gather
    for a in (random_msda_inputs(1, [(8, 8)], 8, 16, 10, 4),
              [x.double() if x.is_floating_point() else x for x in args],
              random_msda_inputs(1, [(4, 4)], 2, 30, 16, 4),
              random_msda_inputs(1, [(4, 4)], 2, 16, 16, 3)):
        MSDA.ms_deform_attn_forward(*dev(*a), 64)
        assert MSDA.last_forward_impl() == "gather" and MSDA.last_forward_kernel().startswith("msda_fwd_gather")


@pytest.mark.parametrize("L,D", [(7, 16), (6, 32)])
def test_auto_stands_down_tile_by_tile(msda_impl, L, D):
    """Round 4: no probe kernel in front of the public-contract forward.  msda_fwd_group2 looks at every tile's own taps
    (the sample that also places its windows) and, in `auto`, a tile whose taps are mostly far from their cells computes its
    outputs in the gather formulation inside the same launch.  Mixed input: the left half of every camera's map samples near
    its cells, the right half anywhere -- both kinds of job in one launch, every query against the oracle; forced `tile`
    (windows everywhere, far taps one by one) must agree."""
    MSDA = msda_impl
    H, W, M = 20, 48, 128 // D
    value, shapes, lsi, loc, aw = encoder_msda_inputs(L, H, W, M, D, 4, seed=11, noise_px=1.0)
    g = torch.Generator().manual_seed(12)
    far = torch.rand(loc.shape, generator=g) * 1.2 - 0.1
    right = (torch.arange(H * W) % W >= W // 2).repeat(L)                       # per query: right half of its camera's map
    loc = torch.where(right[None, :, None, None, None, None], far, loc).contiguous()
    want = c_oracle.msda_forward(value.double(), shapes, lsi, loc.double(), aw.double())
    for impl in ("auto", "tile"):
        MSDA.set_forward_impl(impl)
        got = MSDA.ms_deform_attn_forward(*dev(value, shapes, lsi, loc, aw), 64)
        assert MSDA.last_forward_impl() == "tile" and MSDA.last_forward_kernel().startswith("msda_fwd_group2")
        assert (got.cpu().double() - want).abs().max().item() < FP32_TOL, impl
    MSDA.set_forward_impl("auto")


# ---- backward at encoder shapes (partial tiles, misses, batch, NaN) vs the oracle ------------------------------------
def _away_from_texel_centres(loc, shapes, eps=1e-4):
    """1.0 where a tap's pixel coordinates are both > eps away from an integer.  The bilinear blend is
    continuous there but its derivative w.r.t. the location is not (left and right slopes differ), so
    grad_sampling_loc of a tap that lands within fp32 rounding of a texel centre legitimately depends on
    which side the rounding falls; such taps (a handful per million) are excluded from grad_loc checks."""
    wh = torch.stack([shapes[:, 1], shapes[:, 0]], -1).double()               # [L,2] (W,H)
    px = loc.double() * wh[None, None, None, :, None, :] - 0.5
    d = (px - px.round()).abs()
    return (d.amin(-1) > eps).double()


BWD_TILE_CASES = {
    "mvdetr_like_partial_tiles": lambda: encoder_msda_inputs(7, 21, 43, seed=2, noise_px=1.0),
    "wide_offsets_many_misses": lambda: encoder_msda_inputs(3, 24, 40, seed=4, noise_px=6.0),
    "batch2": lambda: encoder_msda_inputs(4, 17, 19, B=2, seed=5),
    "single_level": lambda: encoder_msda_inputs(1, 30, 50, seed=7),
    "m2": lambda: encoder_msda_inputs(5, 12, 18, M=2, D=16, seed=8),
    "uniform_locations": lambda: random_msda_inputs(1, [(20, 33)] * 3, 4, 16, 3 * 20 * 33, 4, seed=9, lo=-0.1, hi=1.1),
}


@pytest.mark.parametrize("case", sorted(BWD_TILE_CASES))
def test_backward_encoder_shapes_vs_oracle(ops, case):
    _, MSDA = ops
    value, shapes, lsi, loc, aw = BWD_TILE_CASES[case]()
    go = torch.randn(value.shape[0], loc.shape[1], value.shape[2] * value.shape[3],
                     generator=torch.Generator().manual_seed(1))
    ref = c_oracle.msda_backward(value.double(), shapes, lsi, loc.double(), aw.double(), go.double())
    got = [x.cpu().double() for x in MSDA.ms_deform_attn_backward(*dev(value, shapes, lsi, loc, aw, go), 64)]
    W = float(shapes[:, 1].max())
    smooth = _away_from_texel_centres(loc, shapes)
    for a, b, name, scale in zip(got, ref, ("grad_value", "grad_loc", "grad_aw"), (1.0, W, 1.0)):
        assert a.shape == b.shape
        err = (a - b).abs() / (scale + b.abs())
        if name == "grad_loc":
            err = err * smooth[..., None]
        assert err.max().item() < 2e-4, name


def test_backward_unequal_levels_and_nan(ops):
    from helpers import pyramid_encoder_inputs
    _, MSDA = ops
    value, shapes, lsi, loc, aw = pyramid_encoder_inputs([(10, 37), (20, 11), (7, 7)], M=4, D=16, seed=10, noise_px=3.0)
    loc[0, 5] = float("nan")
    loc[0, 6] = 1e30
    go = torch.randn(1, loc.shape[1], 64, generator=torch.Generator().manual_seed(2))
    gv, gl, ga = [x.cpu() for x in MSDA.ms_deform_attn_backward(*dev(value, shapes, lsi, loc, aw, go), 64)]
    assert torch.isfinite(gv).all() and float(gl[0, 5:7].abs().max()) == 0.0 and float(ga[0, 5:7].abs().max()) == 0.0
    keep = torch.ones(loc.shape[1], dtype=torch.bool)
    keep[5:7] = False
    lo, awc, goc = [x[:, keep].double().contiguous() for x in (loc, aw, go)]
    rv, rl, ra = c_oracle.msda_backward(value.double(), shapes, lsi, lo, awc, goc)
    assert ((gv.double() - rv).abs() / (1 + rv.abs())).max().item() < 2e-4
    assert ((ga[:, keep].double() - ra).abs() / (1 + ra.abs())).max().item() < 2e-4


def test_training_through_the_function_matches_oracle_autograd(ops):
    F, MSDA = ops
    value, shapes, lsi, loc, aw = encoder_msda_inputs(3, 10, 18, M=4, D=16, seed=3)
    leaves = [x.clone().cuda().requires_grad_(True) for x in (value, loc, aw)]
    out = F.apply(leaves[0], shapes.cuda(), lsi.cuda(), leaves[1], leaves[2], 64)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(4))
    got = torch.autograd.grad(out, leaves, go.cuda())
    cl = [x.clone().double().requires_grad_(True) for x in (value, loc, aw)]
    ref = torch.autograd.grad(torch_oracle.msda_core(cl[0], shapes, cl[1], cl[2]), cl, go.double())
    for a, b, scale in zip(got, ref, (1.0, 18.0, 1.0)):
        assert ((a.cpu().double() - b).abs() / (scale + b.abs())).max().item() < 2e-4


# ---- fused inference path (softmax + sampling locations inside the kernel) --------------------------------
def _module_with_random_projections(d_model, L, M, P, seed):
    from mvdetr_amd.ops.modules import MSDeformAttn
    torch.manual_seed(seed)
    mod = MSDeformAttn(d_model, L, M, P)
    with torch.no_grad():
        mod.sampling_offsets.weight.normal_(0, 0.05)
        mod.attention_weights.weight.normal_(0, 0.3)
        mod.attention_weights.bias.normal_(0, 0.5)
    return mod


@pytest.mark.parametrize("L,H,W,B,d_model", [(7, 21, 43, 1, 128), (3, 16, 24, 2, 128), (16, 9, 17, 1, 256), (4, 40, 64, 1, 128),
                                             (6, 20, 31, 2, 128), (7, 13, 19, 1, 256), (7, 6, 16, 1, 128), (6, 61, 35, 1, 128)])
def test_fused_module_forward_vs_oracle_and_unfused(ops, L, H, W, B, d_model):
    _, MSDA = ops
    M, P = 8, 4
    mod = _module_with_random_projections(d_model, L, M, P, seed=L).cuda().eval()
    shapes = torch.tensor([[H, W]] * L)
    S = L * H * W
    g = torch.Generator().manual_seed(L + H)
    query = torch.randn(B, S, d_model, generator=g)
    src = torch.randn(B, S, d_model, generator=g)
    ys, xs = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
    ref = torch.stack([xs / W, ys / H], -1).reshape(-1, 1, 1, 2).repeat(L, L, P, 1)      # [S,L,P,2]
    ref = ref + 0.002 * torch.randn(ref.shape, generator=g)
    ref_b = ref.unsqueeze(0).expand(B, -1, -1, -1, -1)                                   # stride-0 batch
    with torch.no_grad():
        fused = mod(query.cuda(), ref_b.cuda(), src.cuda(), shapes.cuda(), level_start_index(shapes).cuda())
        assert MSDA.last_forward_impl() == "tile_fused"
        mod.fused_inference = False
        unfused = mod(query.cuda(), ref_b.cuda(), src.cuda(), shapes.cuda(), level_start_index(shapes).cuda())
        assert MSDA.last_forward_impl() == "tile"
    params = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    want = torch_oracle.msda_module(params, query, ref_b, src, shapes, M, P)
    assert (fused.cpu() - want).abs().max().item() < FP32_TOL
    assert (unfused.cpu() - want).abs().max().item() < FP32_TOL
    assert (fused - unfused).abs().max().item() < 2e-5
    # per-batch (non-expanded) reference points take the same path
    ref2 = ref_b.contiguous().cuda()
    mod.fused_inference = True
    with torch.no_grad():
        again = mod(query.cuda(), ref2, src.cuda(), shapes.cuda(), level_start_index(shapes).cuda())
    assert torch.equal(again, fused)


def test_fused_path_is_inference_only_and_training_still_matches(ops):
    """Three levels: outside MVDeTr's 6 / 7, where the fused TRAINING pair stopped until ABI 13.  With the pair switched off a
    call that needs gradients takes the reference's unfused arithmetic + MSDeformAttnFunction; with it on (the default) it takes
    the pair's general route (inference forward + statistics pass, one-pass backward) -- same output, same gradients."""
    _, MSDA = ops
    L, H, W, M, P, d_model = 3, 10, 18, 8, 4, 128
    mod = _module_with_random_projections(d_model, L, M, P, seed=1).cuda().train()
    shapes = torch.tensor([[H, W]] * L).cuda()
    S = L * H * W
    query = torch.randn(1, S, d_model, device="cuda", requires_grad=True)
    ys, xs = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
    ref = torch.stack([xs / W, ys / H], -1).reshape(-1, 1, 1, 2).repeat(L, L, P, 1)[None].cuda()
    mod.fused_training = False
    out = mod(query, ref, query, shapes, level_start_index(shapes))
    assert MSDA.last_forward_impl() == "tile"                      # grad mode, pair off: the differentiable path
    out.square().mean().backward()
    assert query.grad is not None and mod.sampling_offsets.weight.grad.abs().sum() > 0
    unfused = [query.grad.clone(), mod.sampling_offsets.weight.grad.clone(), mod.attention_weights.weight.grad.clone(),
               mod.value_proj.weight.grad.clone()]
    query.grad = None
    mod.zero_grad()
    mod.fused_training = True
    out_f = mod(query, ref, query, shapes, level_start_index(shapes))
    assert MSDA.last_forward_impl() == "tile_fused"                # grad mode, pair on: its general route
    out_f.square().mean().backward()
    assert (out_f - out).abs().max().item() < 2e-5
    fused = [query.grad, mod.sampling_offsets.weight.grad, mod.attention_weights.weight.grad, mod.value_proj.weight.grad]
    for a, b in zip(fused, unfused):
        assert (a - b).abs().max().item() < 2e-4 * (1.0 + b.abs().max().item())
    with torch.no_grad():
        out2 = mod(query, ref, query, shapes, level_start_index(shapes))
    assert MSDA.last_forward_impl() == "tile_fused"
    assert (out2 - out.detach()).abs().max().item() < 2e-5


def test_fused_seven_unequal_levels_take_the_tile_kernel(ops):
    """L = 7 selects the camera-grouped kernel on the host, but the shapes (device-side) are unequal: the
    grouped kernel must stand down and the tile kernel must do the work."""
    from helpers import pyramid_encoder_inputs
    _, MSDA = ops
    lv = [(12, 20), (6, 10), (12, 20), (3, 5), (8, 8), (12, 20), (5, 9)]
    value, shapes, lsi, _, _ = pyramid_encoder_inputs(lv, M=8, D=16, seed=3)
    S = value.shape[1]
    g = torch.Generator().manual_seed(5)
    off = torch.randn(1, S, 7, 8, 4, 2, generator=g) * 1.5            # level-major raw offsets (pixels)
    logit = torch.randn(1, S, 7, 8, 4, generator=g)
    refs = []
    for H, W in lv:
        ys, xs = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
        refs.append(torch.stack([xs / W, ys / H], -1).reshape(-1, 2))
    ref = torch.cat(refs, 0).view(1, S, 1, 1, 2).repeat(1, 1, 7, 4, 1)
    out = MSDA.ms_deform_attn_forward_fused(*dev(value, shapes, lsi, ref, off, logit), level_major=True).cpu()
    off_hm, logit_hm = off.permute(0, 1, 3, 2, 4, 5), logit.permute(0, 1, 3, 2, 4)
    loc = torch_oracle.msda_sampling_locations(ref, off_hm, shapes)
    aw = torch.softmax(logit_hm.flatten(3), -1).view(1, S, 8, 7, 4)
    want = torch_oracle.msda_core(value, shapes, loc, aw)
    assert (out - want).abs().max().item() < FP32_TOL


# ---- query levels: one rank's share of a query-sharded encoder layer ---------------
QL_CASES = {
    "wildtrack-like": ([(13, 21)] * 7, 8, 16, 1, [(0, 1), (3, 4), (6, 7), (2, 5), (0, 7)]),
    "two-per-rank": ([(9, 17)] * 6, 8, 16, 2, [(0, 2), (2, 4), (4, 6)]),
    "unequal": ([(12, 20), (6, 10), (12, 20), (3, 5), (8, 8)], 8, 16, 1, [(0, 1), (1, 3), (3, 5), (4, 5)]),
    "d32": ([(10, 18)] * 4, 8, 32, 1, [(1, 2), (2, 4)]),
}


@pytest.mark.parametrize("case", sorted(QL_CASES))
@pytest.mark.parametrize("level_major", [False, True])
def test_fused_query_levels_vs_full_call_and_oracle(ops, case, level_major):
    """Restricting the queries to the tokens of levels [l0, l1) returns exactly those rows of the full call."""
    from helpers import pyramid_encoder_inputs
    _, MSDA = ops
    lv, M, D, B, ranges = QL_CASES[case]
    L, P = len(lv), 4
    value, shapes, lsi, _, _ = pyramid_encoder_inputs(lv, M=M, D=D, B=B, seed=11)
    S = value.shape[1]
    g = torch.Generator().manual_seed(7)
    off = torch.randn(B, S, M, L, P, 2, generator=g) * 1.5
    logit = torch.randn(B, S, M, L, P, generator=g)
    refs = []
    for H, W in lv:
        ys, xs = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
        refs.append(torch.stack([xs / W, ys / H], -1).reshape(-1, 2))
    ref = torch.cat(refs, 0).view(1, S, 1, 1, 2).repeat(B, 1, L, P, 1) + 0.002 * torch.randn(B, S, L, P, 2, generator=g)
    loc = torch_oracle.msda_sampling_locations(ref, off, shapes)
    aw = torch.softmax(logit.flatten(3), -1).view(B, S, M, L, P)
    want = torch_oracle.msda_core(value, shapes, loc, aw)
    if level_major:
        off_k, logit_k = off.permute(0, 1, 3, 2, 4, 5).contiguous(), logit.permute(0, 1, 3, 2, 4).contiguous()
    else:
        off_k, logit_k = off, logit
    value_d, shapes_d, lsi_d = dev(value, shapes, lsi)
    full = MSDA.ms_deform_attn_forward_fused(value_d, shapes_d, lsi_d, *dev(ref, off_k, logit_k), level_major=level_major)
    assert (full.cpu() - want).abs().max().item() < FP32_TOL
    starts = lsi.tolist() + [S]
    for l0, l1 in ranges:
        q0, q1 = starts[l0], starts[l1]
        assert MSDA.fused_supported(value_d, L, q1 - q0, P, (l0, l1))
        part = MSDA.ms_deform_attn_forward_fused(
            value_d, shapes_d, lsi_d, *dev(ref[:, q0:q1].contiguous(), off_k[:, q0:q1].contiguous(),
                                           logit_k[:, q0:q1].contiguous()),
            level_major=level_major, query_levels=(l0, l1))
        assert MSDA.last_forward_impl() == "tile_fused"
        assert part.shape == (B, q1 - q0, M * D)
        assert (part.cpu() - want[:, q0:q1]).abs().max().item() < FP32_TOL, (l0, l1)
        if (l0, l1) != (0, L) or not (L in (6, 7) and len(set(lv)) == 1):
            # same kernel, same summation order as the rows of the full call (the grouped kernel, which serves
            # the full call for 6 or 7 equal cameras, sums in another order)
            assert (part - full[:, q0:q1]).abs().max().item() < 2e-5


def test_fused_query_levels_rejects_inconsistent_ranges(ops):
    _, MSDA = ops
    value = torch.randn(1, 4 * 6 * 8, 8, 16, device="cuda")
    assert MSDA.fused_supported(value, 4, 48, 4, (1, 2))
    assert not MSDA.fused_supported(value, 4, 48, 4, (2, 2))
    assert not MSDA.fused_supported(value, 4, 48, 4, (3, 5))
    assert not MSDA.fused_supported(value, 4, 4 * 48 + 1, 4, (0, 3))
    assert not MSDA.fused_supported(value, 4, 48, 4, None)            # all levels need Lq == S


# ---- grad_value through fixed-point LDS windows (msda_backward_tile.hip) ------------------------------------
@pytest.mark.parametrize("variant", ["plain", "tiny", "huge", "wild_weights", "d32", "mixed_magnitudes", "converging", "far_mix"])
def test_backward_fixed_point_windows_keep_fp32_accuracy(ops, variant):
    """The encoder-shaped backward accumulates grad_value in per-tile fixed-point windows whose scale follows
    the data: the error stays far below the 1e-4 bar relative to the gradient's own scale for tiny, huge,
    unnormalised / negative weights and strongly mixed magnitudes alike."""
    _, MSDA = ops
    M, D = (4, 32) if variant == "d32" else (8, 16)
    value, shapes, lsi, loc, aw = encoder_msda_inputs(7, 19, 37, M=M, D=D, seed=21, noise_px=1.5)
    go = torch.randn(1, loc.shape[1], M * D, generator=torch.Generator().manual_seed(5))
    if variant == "tiny":
        go = go * 1e-30
    elif variant == "huge":
        go = go * 1e25
    elif variant == "wild_weights":
        aw = (aw - 0.02) * 300.0                                   # negative and far from a softmax
    elif variant == "mixed_magnitudes":
        go = go * torch.logspace(-6, 3, go.shape[1]).view(1, -1, 1)        # 9 decades across the queries
    elif variant == "converging":
        # the mass bound's worst case (msda_bwd_value_tok: one atomic per tap + 2 x 2 dilation): every tap of every query of a
        # tile row lands on (almost) the same token, with weights far above a softmax's -- no accumulator may overflow
        H_, W_ = 19, 37
        target = torch.tensor([17.3 / W_, 9.6 / H_])
        loc = target.expand_as(loc).clone() + 1e-4 * torch.randn(loc.shape, generator=torch.Generator().manual_seed(9))
        aw = aw * 40.0
    elif variant == "far_mix":
        # a fifth of the taps far outside every window (direct fp32 atomics) among near ones, some outside the map
        far = torch.rand(loc.shape[:-1], generator=torch.Generator().manual_seed(10)) < 0.2
        loc = torch.where(far[..., None], torch.rand(loc.shape, generator=torch.Generator().manual_seed(11)) * 1.4 - 0.2, loc)
    ref = c_oracle.msda_backward(value.double(), shapes, lsi, loc.double(), aw.double(), go.double())[0]
    gv = MSDA.ms_deform_attn_backward(*dev(value, shapes, lsi, loc, aw, go), 64)[0].cpu().double()
    assert torch.isfinite(gv).all()
    # per job the quantisation step is <= 2^-20 of (largest |go| * sum|aw|) among the ~100 cells of its tile
    tile_scale = ref.abs().max().item() if variant != "mixed_magnitudes" else None
    if tile_scale is not None:
        assert (gv - ref).abs().max().item() < 2e-5 * tile_scale
    else:
        # magnitudes vary smoothly along the token axis: compare against a running local scale
        flat_ref, flat_gv = ref.flatten(2)[0], gv.flatten(2)[0]             # [S, M*D]
        local = torch.nn.functional.max_pool1d(flat_ref.abs().amax(1)[None, None], 1201, 1, 600)[0, 0]
        assert ((flat_gv - flat_ref).abs().amax(1) / (local + 1e-30)).max().item() < 1e-3


def test_backward_nonfinite_upstream_gradients_propagate_like_fp32_atomics(ops):
    _, MSDA = ops
    value, shapes, lsi, loc, aw = encoder_msda_inputs(7, 12, 20, M=8, D=16, seed=22)
    go = torch.randn(1, loc.shape[1], 128, generator=torch.Generator().manual_seed(6))
    go[0, 33, 5] = float("inf")
    go[0, 700, 17] = float("nan")
    gv = MSDA.ms_deform_attn_backward(*dev(value, shapes, lsi, loc, aw, go), 64)[0].cpu()
    ok = go.clone()
    ok[0, 33, 5] = 0
    ok[0, 700, 17] = 0
    ref = c_oracle.msda_backward(value.double(), shapes, lsi, loc.double(), aw.double(), ok.double())[0]
    gv4, ref4 = gv.view(1, -1, 8, 16), ref.view(1, -1, 8, 16)
    bad = ~torch.isfinite(gv4)
    assert bad[..., 0, 5].any() and bad[..., 1, 1].any()               # the poisoned channels show up ...
    clean = torch.ones(8, 16, dtype=torch.bool)
    clean[0, 5] = clean[1, 1] = False
    assert torch.isfinite(gv4[..., clean]).all()                       # ... and only they
    assert (gv4[..., clean].double() - ref4[..., clean]).abs().max().item() < 2e-4


# ---- many cameras (9..16 levels): the camera-split group kernel (4 lane groups on one window) ------------------
@pytest.mark.parametrize("L,D,M,H,W,B", [(9, 16, 8, 13, 21, 1), (12, 16, 4, 9, 33, 2), (16, 32, 8, 12, 20, 1), (13, 32, 2, 7, 18, 1)])
def test_many_camera_group_kernel_fused_and_unfused(ops, msda_impl, L, D, M, H, W, B):
    MSDA = msda_impl
    value, shapes, lsi, loc, aw = encoder_msda_inputs(L, H, W, M=M, D=D, B=B, seed=L, noise_px=1.5)
    want = torch_oracle.msda_core(value, shapes, loc, aw)
    got, used = _fwd_impl(MSDA, "tile", (value, shapes, lsi, loc, aw))
    assert used == "tile"
    assert (got - want).abs().max().item() < FP32_TOL
    # fused entry on the same problem: raw offsets (pixels) and logits whose softmax is `aw`
    S, P = value.shape[1], 4
    ys, xs = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
    ref = torch.stack([xs / W, ys / H], -1).reshape(1, H * W, 1, 1, 2).repeat(B, L, L, P, 1)
    off = (loc - ref[:, :, None]) * torch.tensor([W, H], dtype=torch.float32)
    logit = torch.log(aw.clamp_min(1e-30))
    out = MSDA.ms_deform_attn_forward_fused(*dev(value, shapes, lsi, ref, off, logit)).cpu()
    assert MSDA.last_forward_impl() == "tile_fused"
    assert (out - want).abs().max().item() < FP32_TOL


def test_many_unequal_levels_fall_back_inside_the_group_launch(ops, msda_impl):
    from helpers import pyramid_encoder_inputs
    MSDA = msda_impl
    lv = [(12, 20), (6, 10), (12, 20), (3, 5), (8, 8), (12, 20), (5, 9), (4, 4), (9, 14), (2, 7)]
    value, shapes, lsi, loc, aw = pyramid_encoder_inputs(lv, M=8, D=16, seed=4)
    want = torch_oracle.msda_core(value, shapes, loc, aw)
    got, used = _fwd_impl(MSDA, "tile", (value, shapes, lsi, loc, aw))
    assert used == "tile" and (got - want).abs().max().item() < FP32_TOL


# ---- one reference point per (query, level), [.., Lq, L, 2] (layout flag bit 1) ------------------------------------
@pytest.mark.parametrize("lv,D,B", [([(13, 21)] * 7, 16, 1), ([(9, 17)] * 3, 16, 2), ([(8, 12)] * 12, 32, 1),
                                     ([(12, 20), (6, 10), (12, 20), (3, 5), (8, 8)], 16, 1)])
@pytest.mark.parametrize("level_major", [False, True])
def test_fused_shared_reference_point_equals_the_expanded_call(ops, lv, D, B, level_major):
    from helpers import pyramid_encoder_inputs
    _, MSDA = ops
    M, P, L = 8, 4, len(lv)
    value, shapes, lsi, _, _ = pyramid_encoder_inputs(lv, M=M, D=D, B=B, seed=13)
    S = value.shape[1]
    g = torch.Generator().manual_seed(17)
    off = torch.randn(B, S, M, L, P, 2, generator=g) * 1.5
    logit = torch.randn(B, S, M, L, P, generator=g)
    refs = []
    for H, W in lv:
        ys, xs = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
        refs.append(torch.stack([xs / W, ys / H], -1).reshape(-1, 2))
    ref3 = torch.cat(refs, 0).view(1, S, 1, 2).repeat(1, 1, L, 1) + 0.003 * torch.randn(1, S, L, 2, generator=g)
    ref5 = ref3.unsqueeze(3).expand(1, S, L, P, 2).contiguous()
    if level_major:
        off_k, logit_k = off.permute(0, 1, 3, 2, 4, 5).contiguous(), logit.permute(0, 1, 3, 2, 4).contiguous()
    else:
        off_k, logit_k = off, logit
    args = dev(value, shapes, lsi)
    full = MSDA.ms_deform_attn_forward_fused(*args, *dev(ref5, off_k, logit_k), level_major=level_major)
    shared = MSDA.ms_deform_attn_forward_fused(*args, *dev(ref3, off_k, logit_k), level_major=level_major)
    assert torch.equal(full, shared)                               # same arithmetic, fewer bytes
    loc = torch_oracle.msda_sampling_locations(ref5.expand(B, -1, -1, -1, -1), off, shapes)
    aw = torch.softmax(logit.flatten(3), -1).view(B, S, M, L, P)
    assert (shared.cpu() - torch_oracle.msda_core(value, shapes, loc, aw)).abs().max().item() < FP32_TOL
    # one rank's query levels take the same reference layout
    starts = lsi.tolist() + [S]
    part = MSDA.ms_deform_attn_forward_fused(
        *args, *dev(ref3[:, starts[1]:starts[2]].contiguous(), off_k[:, starts[1]:starts[2]].contiguous(),
                    logit_k[:, starts[1]:starts[2]].contiguous()), level_major=level_major, query_levels=(1, 2))
    assert (part - full[:, starts[1]:starts[2]]).abs().max().item() < 2e-5


def test_module_detects_a_shared_reference_point(ops):
    _, MSDA = ops
    L, H, W, M, P, d_model = 7, 10, 18, 8, 4, 128
    mod = _module_with_random_projections(d_model, L, M, P, seed=2).cuda().eval()
    shapes = torch.tensor([[H, W]] * L).cuda()
    S = L * H * W
    query = torch.randn(1, S, d_model, device="cuda")
    ys, xs = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
    ref = torch.stack([xs / W, ys / H], -1).reshape(-1, 1, 1, 2).repeat(L, L, P, 1)[None].cuda()       # P equal copies
    with torch.no_grad():
        a = mod(query, ref, query, shapes, level_start_index(shapes))
        assert mod._shared_ref_cache[2] is True and mod._shared_reference(ref).shape == (1, L, S, 2)   # level-major
        ref2 = ref.clone()
        ref2[0, 5, 2, 1, 0] += 0.01                                # one point differs: the full tensor is used
        b = mod(query, ref2, query, shapes, level_start_index(shapes))
        assert mod._shared_ref_cache[2] is False
        mod.fused_inference = False
        c = mod(query, ref, query, shapes, level_start_index(shapes))
    assert (a - c).abs().max().item() < 2e-5 and (a - b).abs().max().item() > 0


def test_module_caches_survive_recycled_addresses_and_data_writes(ops):
    """(1) a NEW reference tensor that lands on a freed tensor's address must not inherit its verdict or
    its points; (2) parameter writes through .data (EMA swaps, constant_(w.data)) must reach the fused path."""
    _, MSDA = ops
    L, H, W, M, P, d_model = 3, 9, 14, 8, 4, 128
    mod = _module_with_random_projections(d_model, L, M, P, seed=4).cuda().eval()
    shapes = torch.tensor([[H, W]] * L).cuda()
    lsi = level_start_index(shapes)
    S = L * H * W
    query = torch.randn(1, S, d_model, device="cuda")
    ys, xs = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
    base = torch.stack([xs / W, ys / H], -1).reshape(-1, 1, 1, 2).repeat(L, L, P, 1)[None]
    with torch.no_grad():
        for k in range(6):                                         # same shape, allocated and freed over and over
            ref = (base + 0.01 * k).cuda()
            if k % 2:
                ref[0, :, :, 1:] += 0.02                           # odd rounds: the P points differ
            got = mod(query, ref, query, shapes, lsi)
            mod.fused_inference = False
            want = mod(query, ref, query, shapes, lsi)
            mod.fused_inference = True
            assert (got - want).abs().max().item() < 2e-5, k
            del ref
        ref = base.cuda()
        before = mod(query, ref, query, shapes, lsi)
        mod.sampling_offsets.weight.data.normal_(0, 0.05)          # no version bump
        mod.attention_weights.bias.data.add_(0.3 * torch.randn_like(mod.attention_weights.bias))
        after = mod(query, ref, query, shapes, lsi)
        mod.fused_inference = False
        want = mod(query, ref, query, shapes, lsi)
        assert (after - before).abs().max().item() > 1e-3 and (after - want).abs().max().item() < 2e-5
        # the opt-in cache is the owner's promise that parameters are frozen; re-arming it picks up changes
        mod.fused_inference = True
        mod.cache_fused_projection(True)
        c1 = mod(query, ref, query, shapes, lsi)
        assert (c1 - want).abs().max().item() < 2e-5
        mod.sampling_offsets.bias.data.add_(0.5)
        mod.cache_fused_projection(True)
        c2 = mod(query, ref, query, shapes, lsi)
        assert (c2 - c1).abs().max().item() > 1e-3


def test_module_fused_path_is_skipped_when_any_parameter_trains(ops):
    """frozen offsets + trainable attention weights must still get gradients (the fused kernel is not
    differentiable)."""
    L, H, W, M, P, d_model = 3, 7, 9, 8, 4, 128
    mod = _module_with_random_projections(d_model, L, M, P, seed=5).cuda()
    for prm in mod.parameters():
        prm.requires_grad_(False)
    mod.attention_weights.weight.requires_grad_(True)
    shapes = torch.tensor([[H, W]] * L).cuda()
    S = L * H * W
    query = torch.randn(1, S, d_model, device="cuda")
    ys, xs = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
    ref = torch.stack([xs / W, ys / H], -1).reshape(-1, 1, 1, 2).repeat(L, L, P, 1)[None].cuda()
    out = mod(query, ref, query, shapes, level_start_index(shapes))
    out.square().mean().backward()
    assert mod.attention_weights.weight.grad is not None and mod.attention_weights.weight.grad.abs().max().item() > 0


@pytest.mark.parametrize("lv,D,M,B,ql", [([(13, 21)] * 7, 16, 8, 1, None), ([(9, 17)] * 6, 32, 4, 2, None), ([(8, 12)] * 12, 32, 2, 1, None),
                                        ([(6, 9), (7, 11), (5, 8)], 16, 4, 1, None), ([(10, 14)] * 5, 16, 8, 1, (1, 3)),
                                        ([(11, 13)] * 4, 16, 2, 2, None)])
def test_fused_slice_interleaved_layout_equals_the_plain_layouts(ops, lv, D, M, B, ql):
    """ABI v7: ONE raw tensor, slice-interleaved (MSDA.slice_major_rows), with query-major or level-major shared
    reference points -- against the level-major two-tensor form and the oracle; group kernel, many-camera kernel,
    unequal levels (tile body inside the group launch) and a query-level range (tile kernel)."""
    _, MSDA = ops
    P, L = 4, len(lv)
    shapes = torch.tensor(lv)
    lsi = level_start_index(shapes)
    S = int(shapes.prod(1).sum())
    g = torch.Generator().manual_seed(L * 100 + D)
    value = torch.randn(B, S, M, D, generator=g)
    q0, q1 = (0, S) if ql is None else (int(lsi[ql[0]]), int(lsi[ql[1]]) if ql[1] < L else S)
    Lq = q1 - q0
    # one reference point per (query, level): the query's own cell centre in every level + jitter
    cells = torch.cat([torch.stack(torch.meshgrid(torch.arange(h) + 0.5, torch.arange(w) + 0.5, indexing="ij"), -1).reshape(-1, 2)
                       / torch.tensor([h, w]) for h, w in lv])[q0:q1].flip(-1)                     # (x, y) in [0,1]
    ref = (cells[None, :, None, :] + 0.01 * torch.randn(B, Lq, L, 2, generator=g)).contiguous()
    off = 2.5 * torch.randn(B, Lq, M, L, P, 2, generator=g)
    logit = torch.randn(B, Lq, M, L, P, generator=g)
    rows = torch.tensor(MSDA.slice_major_rows(M, L, P, D))
    raw = torch.cat([off.reshape(B, Lq, -1), logit.reshape(B, Lq, -1)], -1).index_select(-1, rows).contiguous()
    kw = {} if ql is None else {"query_levels": ql}
    dv = dev(value, shapes, lsi)
    plain = MSDA.ms_deform_attn_forward_fused(*dv, ref.cuda(), off.cuda(), logit.cuda(), **kw)
    a = MSDA.ms_deform_attn_forward_fused(*dv, ref.cuda(), None, None, raw=raw.cuda(), **kw)
    b = MSDA.ms_deform_attn_forward_fused(*dv, ref.transpose(1, 2).contiguous().cuda(), None, None, raw=raw.cuda(),
                                          ref_level_major=True, **kw)
    # a wider GEMM output whose leading columns are the raw tensor
    wide = torch.cat([raw, torch.randn(B, Lq, 8, generator=g)], -1).cuda()
    c = MSDA.ms_deform_attn_forward_fused(*dv, ref.cuda(), None, None, raw=wide, **kw)
    # the same runs with the level outermost, [.., Lq, L, M/g, run] (what the module produces since round 4)
    rows_lo = torch.tensor(MSDA.slice_major_rows(M, L, P, D, level_outer=True))
    raw_lo = torch.cat([off.reshape(B, Lq, -1), logit.reshape(B, Lq, -1)], -1).index_select(-1, rows_lo).contiguous()
    assert sorted(rows_lo.tolist()) == sorted(rows.tolist()) == list(range(M * L * P * 3))
    d = MSDA.ms_deform_attn_forward_fused(*dv, ref.transpose(1, 2).contiguous().cuda(), None, None, raw=raw_lo.cuda(),
                                          ref_level_major=True, raw_level_outer=True, **kw)
    for got in (a, b, c, d):
        assert (got - plain).abs().max().item() < 2e-5
    loc = torch_oracle.msda_sampling_locations(ref[:, :, :, None, :].expand(B, Lq, L, P, 2), off, shapes)
    want = torch_oracle.msda_core(value, shapes, loc, torch.softmax(logit.flatten(-2), -1).view_as(logit))
    assert (a.cpu() - want).abs().max().item() < FP32_TOL
    with pytest.raises(RuntimeError):
        MSDA.ms_deform_attn_forward_fused(*dv, ref.cuda(), off.cuda(), None, raw=raw.cuda(), **kw)


# ---- seeded sweep over encoder-shaped configurations: every dispatch route against the oracle -------------------
def _sweep_cases(n=28, seed=2024):
    import random
    rnd = random.Random(seed)
    cases = []
    for i in range(n):
        L = rnd.choice([1, 2, 3, 5, 6, 7, 8, 9, 11, 16])
        D = rnd.choice([16, 16, 32, 8])
        M = rnd.choice([1, 2, 3, 4, 8]) if D != 8 else 4
        H, W = rnd.randint(1, 26), rnd.randint(1, 40)
        B = rnd.choice([1, 1, 2])
        noise = rnd.choice([0.5, 1.5, 4.0, 9.0])
        cases.append((i, L, D, M, H, W, B, noise))
    return cases


@pytest.mark.parametrize("i,L,D,M,H,W,B,noise", _sweep_cases())
def test_encoder_shape_sweep_forward_and_backward(ops, i, L, D, M, H, W, B, noise):
    _, MSDA = ops
    value, shapes, lsi, loc, aw = encoder_msda_inputs(L, H, W, M=M, D=D, B=B, seed=100 + i, noise_px=noise)
    want = torch_oracle.msda_core(value.double(), shapes, loc.double(), aw.double())
    got = MSDA.ms_deform_attn_forward(*dev(value, shapes, lsi, loc, aw), 64).cpu().double()
    assert (got - want).abs().max().item() < FP32_TOL
    go = torch.randn(B, loc.shape[1], M * D, generator=torch.Generator().manual_seed(i))
    ref = c_oracle.msda_backward(value.double(), shapes, lsi, loc.double(), aw.double(), go.double())
    grads = [x.cpu().double() for x in MSDA.ms_deform_attn_backward(*dev(value, shapes, lsi, loc, aw, go), 64)]
    smooth = _away_from_texel_centres(loc, shapes)
    for a, b, name, scale in zip(grads, ref, ("grad_value", "grad_loc", "grad_aw"), (1.0, float(W), 1.0)):
        err = (a - b).abs() / (scale + b.abs())
        if name == "grad_loc":
            err = err * smooth[..., None]
        assert err.max().item() < 2e-4, (name, MSDA.last_forward_impl())
    if MSDA.fused_supported(value.cuda(), L, value.shape[1], 4):
        ys, xs = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
        r3 = torch.stack([xs / W, ys / H], -1).reshape(1, H * W, 1, 2).repeat(B, L, L, 1)
        off = (loc - r3[:, :, None, :, None, :]) * torch.tensor([W, H], dtype=torch.float32)
        logit = torch.log(aw.clamp_min(1e-30))
        fused = MSDA.ms_deform_attn_forward_fused(*dev(value, shapes, lsi, r3, off, logit)).cpu().double()
        assert (fused - want).abs().max().item() < FP32_TOL


# ---- 16-bit storage forward (an extension: the reference is float/double only, ms_deform_attn_cuda.cu:64) ---------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("case", [
    (2, [(6, 4), (3, 2)], 2, 2, 2, 2),        # ops/test.py's shape
    (1, [(30, 45)] * 3, 8, 32, 700, 4),       # D = 32: 16-byte accesses
    (2, [(7, 9), (5, 3)], 4, 12, 33, 3),      # D % 8 != 0: 8-byte accesses
    (1, [(5, 5)], 3, 5, 9, 2),                # odd D: scalar accesses
])
def test_forward_half_matches_fp32_oracle(ops, dtype, case):
    """fp16 / bf16 tensors in, fp32 arithmetic, one rounding on the way out: against the fp32 oracle on the SAME
    (already rounded) inputs the only differences are accumulation order and that last rounding -- half an ulp of the
    storage type (2^-11 / 2^-8 relative) plus the fp32 bar."""
    _, MSDA = ops
    B, hw, M, D, Lq, P = case
    v, s, lsi, loc, aw = random_msda_inputs(B, hw, M, D, Lq, P, seed=11)
    v, loc, aw = v.to(dtype), loc.to(dtype), aw.to(dtype)
    out = MSDA.ms_deform_attn_forward(*dev(v, s, lsi, loc, aw), 64).cpu()
    assert out.dtype == dtype and out.shape == (B, Lq, M * D)
    ref = c_oracle.msda_forward(v.float(), s, lsi, loc.float(), aw.float())
    ulp = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    err = (out.float() - ref).abs()
    assert (err <= ulp * ref.abs() + FP32_TOL).all(), err.max().item()
    # and the rounding is to nearest: the result equals the oracle's output rounded the same way almost everywhere
    same = (out == ref.to(dtype)).float().mean().item()
    assert same > 0.99, same


def test_half_backward_is_refused(ops):
    _, MSDA = ops
    v, s, lsi, loc, aw = random_msda_inputs(1, [(4, 4)], 2, 4, 3, 2, seed=1)
    args = dev(v.half(), s, lsi, loc.half(), aw.half())
    go = torch.zeros(1, 3, 8, dtype=torch.float16, device="cuda")
    with pytest.raises(RuntimeError, match="not implemented"):
        MSDA.ms_deform_attn_backward(*args, go, 64)
    with pytest.raises(RuntimeError, match="not implemented"):        # the host path is float/double only
        MSDA.ms_deform_attn_forward(v.half(), s, lsi, loc.half(), aw.half(), 64)


# ---- windows that follow the taps (round 3) ------------------------------------------------------------------------------
def _window_shift_case(scale):
    """Fused module forward on offsets = scale x the reference's bias grid (rays of up to 4 * scale px) + learned noise:
    with scale 1.5 the far points of every ray sit at the edge of a +-6 px window."""
    L, H, W, d_model, M, P = 7, 24, 40, 128, 8, 4
    mod = _module_with_random_projections(d_model, L, M, P, seed=3).eval()
    with torch.no_grad():
        mod.sampling_offsets.bias.mul_(scale)
    shapes = torch.tensor([[H, W]] * L)
    S = L * H * W
    g = torch.Generator().manual_seed(17)
    query, src = torch.randn(1, S, d_model, generator=g), torch.randn(1, S, d_model, generator=g)
    ys, xs = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
    ref = torch.stack([xs / W, ys / H], -1).reshape(-1, 1, 1, 2).repeat(L, L, P, 1)[None]
    return mod, query, ref, src, shapes


@pytest.mark.parametrize("scale", [1.0, 1.5, 2.5])
def test_window_shift_gives_the_same_results_as_centred_windows(ops, scale):
    """The forward kernels centre their LDS windows on where the tile's taps lie (msda_forward_group.hip, msda_tile_body.h).
    Any shift must give the oracle's result -- taps outside the window are gathered from memory -- and the same result as
    MVDETR_MSDA_WINDOW_SHIFT=0 (read once per process: the centred run is a child process)."""
    import os
    import subprocess
    import sys
    import tempfile
    mod, query, ref, src, shapes = _window_shift_case(scale)
    md = mod.cuda()
    with torch.no_grad():
        got = md(query.cuda(), ref.cuda(), src.cuda(), shapes.cuda(), level_start_index(shapes).cuda()).cpu()
        md.fused_inference = False
        unfused = md(query.cuda(), ref.cuda(), src.cuda(), shapes.cuda(), level_start_index(shapes).cuda()).cpu()
    params = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    want = torch_oracle.msda_module(params, query, ref, src, shapes, 8, 4)
    assert (got - want).abs().max().item() < FP32_TOL and (unfused - want).abs().max().item() < FP32_TOL
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "centred.pt")
        code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
                "from test_msda_gpu import _window_shift_case, level_start_index\n"
                "mod, query, ref, src, shapes = _window_shift_case(%r)\n"
                "md = mod.cuda()\n"
                "with torch.no_grad():\n"
                "    y = md(query.cuda(), ref.cuda(), src.cuda(), shapes.cuda(), level_start_index(shapes).cuda()).cpu()\n"
                "torch.save(y, %r)\n") % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                          os.path.dirname(os.path.abspath(__file__)), scale, out)
        env = dict(os.environ, MVDETR_MSDA_WINDOW_SHIFT="0")
        subprocess.run([sys.executable, "-c", code], env=env, check=True, timeout=300)
        centred = torch.load(out)
    assert (centred - want).abs().max().item() < FP32_TOL
    assert (centred - got).abs().max().item() < 2e-5
