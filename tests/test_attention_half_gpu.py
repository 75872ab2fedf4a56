"""attn_fwd_mfma_half (csrc/attention_half.hip) on the MI355X: ops.attention, ops.MultiheadAttention, the ``trans`` aggregator
and the converted model in float16 / bfloat16.

The kernel's bar, on EVERY element:  |out - ref| <= u |ref| + fp32_bar(q, k, v),  u = 2^-11 (fp16) / 2^-8 (bf16) -- one
rounding on the way out of what the fp32 kernel may compute -- with ref = attention_oracle.attention in fp64 on the inputs
rounded to the dtype; and out == rn16(ref) on >= 99 % of the elements, pooled over all cases per (dtype, seed) (an Sq = 1
case has 64 elements: one legitimately flipped rounding would sink it).  tests/test_attention_half.py shows on the CPU that
this bar passes the two-term P V product and refuses P rounded to 16 bits once."""
import ctypes
import importlib

import pytest
import torch

import attention_cases as ac
import attention_oracle as ao
from helpers import smooth_features
from test_attention_half import CASES, DTYPES, bar_ratio_and_equal, rounded_case

pytestmark = pytest.mark.gpu

ROUTE = "attn_fwd_mfma_half"
FP32_ROUTES = ("attn_fwd_mfma", "attn_fwd_generic")


@pytest.fixture
def A():
    mod = importlib.import_module("mvdetr_amd.ops.attention")
    yield mod
    mod.set_half_query_tile(0)


def run_case(A, case, dtype, seed):
    """The case's operands in its own layout on the GPU, rounded to ``dtype`` -> (out dense on the CPU, route)."""
    x = ac.lay_out(case, "cuda", dtype=dtype, seed=seed)
    with torch.no_grad():
        out = A.attention(x.q, x.k, x.v)
    return out.cpu().contiguous(), A.last_kernel()


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("seed", ac.SEEDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_against_the_fp64_oracle(A, dtype, seed, tile):
    """Every tile edge of both workgroup sizes (64 and 128 queries; 64-key pairs, 32-key halves), Sq = 1, Sk = 1, both head
    dimensions, dense / seq-first packed / batch-first operands, and logits of magnitude 80."""
    A.set_half_query_tile(tile)
    same = total = 0
    for case in CASES:
        out, route = run_case(A, case, dtype, seed)
        assert route == ROUTE, (case.name, route)
        _, ref, fbar = rounded_case(case, dtype, seed)
        r, e, n = bar_ratio_and_equal(out, ref, fbar, dtype)
        print(f"ATBAR {ROUTE}/{str(dtype)[6:]}/tq{tile} {case.name} out {r:.3f}")
        assert r <= 1.0, (case.name, r)
        same, total = same + e, total + n
    print(f"rounded-equal {dtype} seed {seed} tile {tile}: {same / total:.5f} of {total}")
    assert same / total >= 0.99, same / total


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_runs_and_both_tiles_give_the_same_bits(A, dtype):
    case = ac.by_name("m16_129x129_packed")
    first, _ = run_case(A, case, dtype, 0)
    again, _ = run_case(A, case, dtype, 0)
    assert torch.equal(first, again)
    A.set_half_query_tile(128)
    wide, _ = run_case(A, case, dtype, 0)
    assert torch.equal(first, wide)              # the workgroup size moves no query's arithmetic


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["m16_33x97_seq", "m32_64x64_packed_bf", "m16_129x129_packed"])
def test_strided_views_are_read_in_place(A, dtype, name):
    """Head-split views of one packed projection reach the kernel as they are (the route is the 16-bit kernel's, which takes
    only what it can address by strides) and give, bit for bit, what dense copies give; out lies in memory like q."""
    case = ac.by_name(name)
    x = ac.lay_out(case, "cuda", dtype=dtype)
    assert not x.q.is_contiguous() and not x.v.is_contiguous()
    with torch.no_grad():
        out = A.attention(x.q, x.k, x.v)
        assert A.last_kernel() == ROUTE
        dense = A.attention(x.q.contiguous(), x.k.contiguous(), x.v.contiguous())
    assert torch.equal(out, dense)
    back = (2, 0, 1, 3) if case.layout == "seq_first" else (0, 2, 1, 3)
    assert out.permute(back).is_contiguous() and dense.is_contiguous()


@pytest.mark.parametrize("dtype", DTYPES)
def test_what_the_kernel_does_not_take_runs_fp32_on_the_upcast(A, dtype):
    # a head dimension of 20
    case = ac.by_name("g20_9x65_gout_zero_rows")
    out, route = run_case(A, case, dtype, 0)
    _, ref, fbar = rounded_case(case, dtype, 0)
    r, _, _ = bar_ratio_and_equal(out, ref, fbar, dtype)
    print(f"ATBAR fallback/{route} {case.name} out {r:.3f}")
    assert route in FP32_ROUTES and r <= 1.0
    # rows that start 2 bytes off a 16-byte boundary
    case = ac.by_name("m16_33x97_seq")
    (q, k, v), ref, fbar = rounded_case(case, dtype, 0)
    pads = [torch.zeros(*t.shape[:3], t.shape[3] + 8, dtype=dtype, device="cuda") for t in (q, k, v)]
    views = []
    for pad, t in zip(pads, (q, k, v)):
        pad[..., 1:t.shape[3] + 1] = t.cuda()
        views.append(pad[..., 1:t.shape[3] + 1])
    assert views[0].data_ptr() % 16 == 2 and views[0].stride(2) % 8 == 0
    with torch.no_grad():
        out = A.attention(*views)
    r, _, _ = bar_ratio_and_equal(out.cpu(), ref, fbar, dtype)
    print(f"ATBAR fallback/{A.last_kernel()} {case.name}_off2 out {r:.3f}")
    assert A.last_kernel() in FP32_ROUTES and r <= 1.0 and out.dtype == dtype


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals(A, dtype):
    from mvdetr_amd import _lib
    q = torch.randn(1, 2, 8, 16, device="cuda").to(dtype)
    with pytest.raises(RuntimeError, match="forward-only"):
        A.attention(q.clone().requires_grad_(True), q, q)
    with pytest.raises(ValueError):
        A.attention(q, q, q, dropout_p=0.25)
    with torch.no_grad():
        assert A.attention(q.clone().requires_grad_(True), q, q).dtype == dtype      # nothing to differentiate: served
    # the C entry itself: D = 20 is refused with hipErrorNotSupported before anything is launched
    x = torch.zeros(1, 1, 8, 20, device="cuda", dtype=dtype)
    strides = (ctypes.c_int64 * 12)(*([160, 160, 20] * 4))
    fn = getattr(_lib.lib(), f"mvdetr_attn_forward_{_lib.suffix(dtype, half_ok=True)}")
    out = torch.full_like(x, 7.0)
    assert fn(_lib.current_stream_ptr(x.device), x.data_ptr(), x.data_ptr(), x.data_ptr(), strides, 1, 1, 8, 8, 20,
              out.data_ptr()) == 801
    assert (out == 7.0).all()


def _identity_projections(mha):
    with torch.no_grad():
        E = mha.embed_dim
        mha.in_proj_weight.copy_(torch.eye(E).repeat(3, 1))
        mha.in_proj_bias.zero_()
        mha.out_proj.weight.copy_(torch.eye(E))
        mha.out_proj.bias.zero_()
    return mha


@pytest.mark.parametrize("dtype", DTYPES)
def test_multihead_attention_in_16_bits(A, dtype):
    """In / out projections = identity, zero bias (exact in 16 bits): the module's output is its core's, rounded once."""
    E, H, S, B = 64, 4, 70, 2
    mha = _identity_projections(A.MultiheadAttention(E, H)).cuda().to(dtype).eval()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(S, B, E, generator=g).to(dtype)
    heads = x.unflatten(-1, (H, E // H)).permute(1, 2, 0, 3)                 # [B, H, S, D]
    ref, fbar = ao.attention(heads, heads, heads), ao.fp32_bar(heads, heads, heads)
    with torch.no_grad():
        out, w = mha(x.cuda(), x.cuda(), x.cuda(), need_weights=False)
    assert w is None and A.last_kernel() == ROUTE
    got = out.cpu().unflatten(-1, (H, E // H)).permute(1, 2, 0, 3)
    r, e, n = bar_ratio_and_equal(got, ref, fbar, dtype)
    print(f"ATBAR {ROUTE}/module out {r:.3f} rounded-equal {e / n:.4f}")
    assert r <= 1.0 and e / n >= 0.99
    # a call that needs a gradient, or a module in training mode, is torch's implementation: our route does not move
    with torch.no_grad():
        A.attention(heads.float().cuda(), heads.float().cuda(), heads.float().cuda())
    sentinel = A.last_kernel()
    assert sentinel in FP32_ROUTES
    mha(x.cuda().requires_grad_(True), x.cuda(), x.cuda(), need_weights=False)[0].sum().backward()
    assert A.last_kernel() == sentinel
    mha.train()
    with torch.no_grad():
        mha(x.cuda(), x.cuda(), x.cuda(), need_weights=False)
    assert A.last_kernel() == sentinel


def _trans_model(dtype):
    """The mini geometry with a 128-channel bottleneck: 8 heads of 16 channels, the head size of the Wildtrack model."""
    from mvdetr_amd.model import build_model
    return build_model("mini", seed=0, world_feat_arch="trans", bottleneck_dim=128).cuda().to_inference(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_trans_world_feat_error_is_not_above_the_torch_compositions(A, dtype, monkeypatch):
    """TransformerWorldFeat in 16 bits: RMS error against the same module in fp32 (the rounded parameters and input, upcast)
    of the HIP path (attn_fwd_mfma_half, fused add + LayerNorm tails: one rounding per op) and of the 16-bit torch
    composition (nn.MultiheadAttention's own path, torch's add then LayerNorm).  Bar: HIP <= 1.25 x composition -- the quarter
    is allowance for one seed's luck over ~10^4 elements (test_encoder_error_is_not_above_the_torch_compositions)."""
    import copy
    import mvdetr_amd.world_feat as world_feat
    model = _trans_model(dtype)
    wf = model.world_feat
    H, W = model.Rworld_shape
    x = smooth_features(model.num_cam, 128, H, W, seed=9).to(dtype).cuda()[None]           # [1, N, C, H, W]
    ref_wf = copy.deepcopy(wf).float()
    with torch.no_grad():
        want = ref_wf(x.float()).cpu()
        hip = wf(x)
        assert A.last_kernel() == ROUTE
        monkeypatch.setattr(A.MultiheadAttention, "_fused_ok", lambda *a, **k: False)
        monkeypatch.setattr(world_feat, "fused_add_layer_norm_available", lambda *a, **k: False)
        A.attention(*(torch.zeros(1, 1, 2, 16, device="cuda"),) * 3)                        # sentinel: an fp32 route
        comp = wf(x)
        assert A.last_kernel() in FP32_ROUTES                                               # (torch's path: ours did not run)
    assert hip.dtype == comp.dtype == dtype and hip.shape == want.shape
    rms_hip = (hip.float().cpu() - want).pow(2).mean().sqrt().item()
    rms_comp = (comp.float().cpu() - want).pow(2).mean().sqrt().item()
    print(f"trans aggregator RMS error vs fp32 ({dtype}): HIP {rms_hip:.3e}, torch composition {rms_comp:.3e}, "
          f"output RMS {want.pow(2).mean().sqrt().item():.3e}")
    assert rms_hip <= 1.25 * rms_comp, (rms_hip, rms_comp)


@pytest.mark.parametrize("dtype", DTYPES)
def test_trans_model_forward_and_detect_in_16_bits(A, dtype):
    from mvdetr_amd.ops import warp
    model = _trans_model(dtype)
    imgs = torch.rand(1, model.num_cam, 3, *model.geom.img_shape, generator=torch.Generator().manual_seed(2)).cuda()
    M = torch.eye(3).repeat(1, model.num_cam, 1, 1)
    with torch.no_grad():
        (hm, off), (ihm, ioff, iwh) = model(imgs, M)
    assert warp.last_kernel() == "warp_fwd_half" and A.last_kernel() == ROUTE
    H, W = model.Rworld_shape
    assert hm.shape == (1, 1, H, W) and off.shape == (1, 2, H, W)
    assert ihm.shape[0] == model.num_cam and ihm.shape[1] == 1 and ioff.shape[1] == 2 and iwh.shape[1] == 2
    for t_ in (hm, off, ihm, ioff, iwh):
        assert t_.dtype == dtype and torch.isfinite(t_).all()
    det = model.detect(imgs, M, cls_thres=0.05)
    assert type(det).__name__ == "Detections"
    assert det[0].dtype == torch.float32 and det[0].shape[0] == 1 and det[0].shape[-1] == 2
    assert det[1].dtype == torch.float32 and torch.isfinite(det[0]).all() and int(det[3][0]) >= 0
