"""16-bit inference on the GPU: the three 16-bit-storage kernels (warp, fused deformable attention, add + LayerNorm) against
oracles that run on the SAME, already rounded inputs, upcast -- so what is left is accumulation order and the one rounding
on the way out: half an ulp of the storage type (2^-11 relative for float16, 2^-8 for bfloat16) plus the fp32 bar of the
op's own fp32 test -- then the encoder and the whole model.  No element is excluded from any comparison."""
import functools

import pytest
import torch
from torch import nn

from helpers import assert_rounded_once, fused_plain, fused_train_inputs, smooth_features, ulp_of
from oracle import c_oracle, torch_oracle

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
FP32_TOL = 1e-4                                           # tests/test_msda_gpu.py, tests/test_warp_gpu.py
LN_FP32_TOL = 5e-6                                        # tests/test_layernorm_gpu.py


# ---- warp ------------------------------------------------------------------------------------------------------------------
N_VIEWS, SRC_HW, DST_HW = 3, (15, 20), (13, 21)           # the destination is no multiple of the kernels' 8 x 8 tile


def warp_mats():
    """One matrix per view (destination pixel <- source pixel), fp32 as the op takes them: near the identity; a perspective
    whose horizon (the destination line that maps to infinity) runs between destination rows 6 and 7 -- the rows below it
    sample the source, magnified more and more towards it, the rows above map behind the camera --; and one that maps every
    destination pixel far outside the source."""
    near = torch.tensor([[1.04, 0.02, 0.3], [-0.015, 0.86, 0.2], [0.0, 0.0, 1.0]], dtype=torch.float64)
    inv = torch.tensor([[0.5, 0.02, 0.5], [0.01, 0.2, 0.3], [0.002, 0.1, -0.65]], dtype=torch.float64)
    away = torch.tensor([[1.0, 0.0, 1000.0], [0.0, 1.0, 1000.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    return torch.stack([near, torch.linalg.inv(inv), away]).float()


@functools.lru_cache(maxsize=None)
def warp_case(dtype, channels, mode):
    """Rounded source [N, C, h, w] and the oracle's fp64 / fp32 results on it [N, C, H, W] (computed once per case)."""
    src = smooth_features(N_VIEWS, channels, *SRC_HW, seed=channels).to(dtype)
    M = warp_mats()
    ref64 = torch_oracle.warp_perspective(src.double(), M.double(), DST_HW, mode=mode)
    ref32 = torch_oracle.warp_perspective(src.float(), M, DST_HW, mode=mode)
    return src, M, ref64, ref32


def check_warp(out_nchw, dtype, channels, mode="bilinear"):
    _, _, ref64, ref32 = warp_case(dtype, channels, mode)
    assert_rounded_once(out_nchw, ref64, dtype, FP32_TOL, extra=1.5 * (ref32.double() - ref64).abs())
    assert (ref64[2] == 0).all() and (out_nchw[2] == 0).all()                # the view that maps outside: exactly zero
    assert ref64[0].abs().max() > 0.1 and ref64[1].abs().max() > 0.1         # (the other two do sample the source)


def last_warp_kernel():
    from mvdetr_amd.ops import warp
    return warp.last_kernel()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("channels", [64, 128])
@pytest.mark.parametrize("cl_out", [True, False])
def test_warp_channel_last_source(dtype, channels, cl_out):
    from mvdetr_amd.ops import warp_perspective
    src, M, _, _ = warp_case(dtype, channels, "bilinear")
    x = src.cuda().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        out = warp_perspective(x, M, DST_HW, channels_last_out=cl_out)
    assert last_warp_kernel() == ("warp_fwd_cl_half" if cl_out else "warp_fwd_half")
    assert out.shape == ((N_VIEWS, *DST_HW, channels) if cl_out else (N_VIEWS, channels, *DST_HW))
    check_warp(out.permute(0, 3, 1, 2) if cl_out else out, dtype, channels)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cl_out", [True, False])
def test_warp_nchw_source_three_channels(dtype, cl_out):
    from mvdetr_amd.ops import warp_perspective
    src, M, _, _ = warp_case(dtype, 3, "bilinear")
    with torch.no_grad():
        out = warp_perspective(src.cuda(), M.cuda(), DST_HW, channels_last_out=cl_out)
    assert last_warp_kernel() == "warp_fwd_half"                             # the generic route, 2-byte accesses
    check_warp(out.permute(0, 3, 1, 2) if cl_out else out, dtype, 3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_warp_nearest(dtype):
    from mvdetr_amd.ops import warp_perspective
    src, M, ref64, _ = warp_case(dtype, 64, "nearest")
    x = src.cuda().contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        out = warp_perspective(x, M, DST_HW, mode="nearest", channels_last_out=True)
        out3 = warp_perspective(src[:, :3].cuda().contiguous(), M, DST_HW, mode="nearest")
    assert last_warp_kernel() == "warp_fwd_half"
    check_warp(out.permute(0, 3, 1, 2), dtype, 64, "nearest")
    assert torch.equal(out.permute(0, 3, 1, 2).cpu().double(), ref64)        # a copy of source texels: no rounding at all
    assert torch.equal(out3.cpu().double(), ref64[:, :3])


@pytest.mark.parametrize("dtype", DTYPES)
def test_warp_half_is_forward_only(dtype):
    from mvdetr_amd.ops import warp_perspective
    src, M, _, _ = warp_case(dtype, 64, "bilinear")
    x = src.cuda().requires_grad_()
    with pytest.raises(RuntimeError, match="forward-only"):
        warp_perspective(x, M, DST_HW)
    with torch.no_grad():                                                    # (nothing to differentiate: served)
        assert warp_perspective(x, M, DST_HW).dtype == dtype


# ---- fused deformable attention ---------------------------------------------------------------------------------------------
MSDA_CASES = {
    "L2_5x7_M8_D16_B2": dict(L=2, H=5, W=7, M=8, D=16, B=2),                 # odd sizes, batch stride
    "L7_12x20_M8_D16": dict(L=7, H=12, W=20, M=8, D=16, B=1),
    "L3_6x9_M4_D32": dict(L=3, H=6, W=9, M=4, D=32, B=1),
}


@functools.lru_cache(maxsize=None)
def msda_case(name, noise_px, dtype):
    """Rounded inputs of the fused call and the fp32 oracle of the module arithmetic on them (softmax, loc = ref + off / (W, H),
    then the C oracle's core)."""
    c = MSDA_CASES[name]
    value, shapes, lsi, ref, raw, rows = fused_train_inputs(c["L"], c["H"], c["W"], M=c["M"], D=c["D"], B=c["B"], seed=3,
                                                            noise_px=noise_px)
    value, raw = value.to(dtype), raw.to(dtype)
    off, logit = fused_plain(raw.float(), rows, c["M"], c["L"])
    wh = torch.tensor([c["W"], c["H"]], dtype=torch.float32)
    ref_ql = ref[0].transpose(0, 1)                                          # [Lq, L, 2]
    loc = (ref_ql[None, :, None, :, None, :] + off / wh).contiguous()
    B, Lq = logit.shape[:2]
    aw = torch.softmax(logit.flatten(-2), -1).view(B, Lq, c["M"], c["L"], 4).contiguous()
    want = c_oracle.msda_forward(value.float(), shapes, lsi, loc, aw)
    outside = ((loc < 0) | (loc > 1)).any(-1).float().mean().item()
    return value, shapes, lsi, ref, raw, want, outside


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("noise_px", [1.0, 6.0])
@pytest.mark.parametrize("name", sorted(MSDA_CASES))
def test_fused_msda_half_matches_fp32_oracle(name, noise_px, dtype):
    from mvdetr_amd.ops import MultiScaleDeformableAttention as MSDA
    value, shapes, lsi, ref, raw, want, outside = msda_case(name, noise_px, dtype)
    assert outside > 0.0                                                      # some taps leave the map (zero padding)
    args = [a.cuda() for a in (value, shapes, lsi, ref, raw)]
    assert MSDA.fused_half_supported(args[0], shapes.shape[0], value.shape[1], 4)
    out = MSDA.ms_deform_attn_forward_fused_half(*args)
    assert MSDA.last_forward_kernel() == "msda_fwd_fused_half"
    res = MSDA.last_forward_resources()
    assert res is not None and res["scratch_bytes_per_lane"] == 0
    assert_rounded_once(out, want, dtype, FP32_TOL)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_msda_half_batch_shared_and_per_batch_reference_agree(dtype):
    from mvdetr_amd.ops import MultiScaleDeformableAttention as MSDA
    value, shapes, lsi, ref, raw, _, _ = msda_case("L2_5x7_M8_D16_B2", 1.0, dtype)
    args = [a.cuda() for a in (value, shapes, lsi, ref, raw)]
    a = MSDA.ms_deform_attn_forward_fused_half(*args)
    args[3] = args[3].expand(2, -1, -1, -1).contiguous()
    assert torch.equal(a, MSDA.ms_deform_attn_forward_fused_half(*args))


def _identity_projections(mod):
    with torch.no_grad():
        for lin in (mod.value_proj, mod.output_proj):
            lin.weight.copy_(torch.eye(lin.weight.shape[0]))
            lin.bias.zero_()
        mod.sampling_offsets.weight.normal_(0.0, 0.05)
        mod.attention_weights.weight.normal_(0.0, 0.3)
    return mod


def _module_case(n_points, dtype, shapes_hw):
    """An MSDeformAttn whose value / output projections are the identity (exact in 16 bits), so that the module's result is
    its core's, rounded once.  -> module, query, 5-D fp32 reference points, src, shapes, lsi (on the GPU)."""
    from mvdetr_amd.ops.modules import MSDeformAttn
    torch.manual_seed(5)
    L, M, C = len(shapes_hw), 8, 128
    mod = _identity_projections(MSDeformAttn(C, L, M, n_points)).cuda().to(dtype).eval()
    shapes = torch.tensor(shapes_hw, dtype=torch.long)
    lsi = torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
    cells = []
    for H, W in shapes_hw:
        ys, xs = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
        cells.append(torch.stack([xs / W, ys / H], -1).reshape(-1, 2))
    cells = torch.cat(cells)                                                 # [S, 2]
    S = cells.shape[0]
    ref = cells[None, :, None, None, :].expand(1, S, L, n_points, 2).contiguous()
    g = torch.Generator().manual_seed(6)
    query, src = torch.randn(1, S, C, generator=g).to(dtype), torch.randn(1, S, C, generator=g).to(dtype)
    return mod, query.cuda(), ref.cuda(), src.cuda(), shapes.cuda(), lsi.cuda()


def _module_oracle(mod, query, ref, src, shapes, lsi, fused):
    """fp32 arithmetic of the module on the offsets / logits its own (16-bit) Linears produce -- the two Linears of the
    unfused path, or (``fused``) the one permuted GEMM of the fused path: the very call the module makes."""
    M, L, P = mod.n_heads, mod.n_levels, mod.n_points
    with torch.no_grad():
        if fused:
            raw = torch.nn.functional.linear(query, *mod._fused_projection()).float().cpu()
            off, logit = fused_plain(raw, mod._fused_rows.cpu(), M, L, P)
            logit = logit.reshape(1, -1, M, L * P)
        else:
            off = mod.sampling_offsets(query).float().cpu().view(1, -1, M, L, P, 2)
            logit = mod.attention_weights(query).float().cpu().view(1, -1, M, L * P)
    wh = torch.stack([shapes[:, 1], shapes[:, 0]], -1).float().cpu()
    loc = (ref.cpu()[:, :, None, :, :, :] + off / wh[None, None, None, :, None, :]).contiguous()
    aw = torch.softmax(logit, -1).view(1, -1, M, L, P).contiguous()
    value = src.float().cpu().view(1, -1, M, mod.d_model // M).contiguous()
    return c_oracle.msda_forward(value, shapes.cpu(), lsi.cpu(), loc, aw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["two_points", "unequal_levels", "fused"])
def test_module_in_16_bits(dtype, case):
    """Calls the 16-bit fused kernel does not take (P = 2; levels of different shapes) WORK: the core runs in fp32 on the
    upcast value, fp32 locations and weights, and the result is cast back -- within the same bar as the fused kernel, which
    the third case runs through the module."""
    from mvdetr_amd.ops import MultiScaleDeformableAttention as MSDA
    P, hw = {"two_points": (2, [(6, 9)] * 3), "unequal_levels": (4, [(6, 9), (4, 5), (3, 7)]), "fused": (4, [(6, 9)] * 3)}[case]
    mod, query, ref, src, shapes, lsi = _module_case(P, dtype, hw)
    with torch.no_grad():
        out = mod(query, ref, src, shapes, lsi)
    assert (MSDA.last_forward_kernel() == "msda_fwd_fused_half") == (case == "fused")
    want = _module_oracle(mod, query, ref, src, shapes, lsi, case == "fused")
    assert_rounded_once(out, want, dtype, FP32_TOL)


# ---- add + LayerNorm ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 37, 1000])
@pytest.mark.parametrize("cols", [64, 128, 256])
@pytest.mark.parametrize("with_res,with_add", [(True, True), (True, False), (False, True), (False, False)])
def test_add_layer_norm_half(dtype, rows, cols, with_res, with_add):
    from mvdetr_amd.ops.add_layernorm import add_layer_norm, fused_add_layer_norm_available
    B = 2
    g = torch.Generator().manual_seed(rows + cols)
    x = (torch.randn(B, rows, cols, generator=g) * 3 + 0.7).to(dtype)
    res = (torch.randn(B, rows, cols, generator=g) * 0.5).to(dtype) if with_res else None
    pos = torch.randn(1, rows, cols, generator=g).to(dtype) if with_add else None     # add2_rows = rows of ONE batch element
    norm = nn.LayerNorm(cols)
    with torch.no_grad():
        norm.weight.copy_(1.0 + 0.3 * torch.randn(cols, generator=g))
        norm.bias.copy_(0.3 * torch.randn(cols, generator=g))
    norm = norm.to(dtype).cuda()
    s = x.double() if res is None else x.double() + res.double()
    want = torch.nn.functional.layer_norm(s, (cols,), norm.weight.double().cpu(), norm.bias.double().cpu(), norm.eps)
    with torch.no_grad():
        assert fused_add_layer_norm_available(x.cuda(), norm)
        got = add_layer_norm(x.cuda(), None if res is None else res.cuda(), norm, then_add=None if pos is None else pos.cuda())
    if with_add:
        got, got2 = got
        assert_rounded_once(got2, want + pos.double(), dtype, LN_FP32_TOL)   # from the UNROUNDED row: one rounding
    assert_rounded_once(got, want, dtype, LN_FP32_TOL)


def test_add_layer_norm_half_refuses_other_widths_and_mixed_dtypes():
    from mvdetr_amd import _lib
    from mvdetr_amd.ops.add_layernorm import fused_add_layer_norm_available
    buf = torch.zeros(96, device="cuda", dtype=torch.bfloat16)
    assert _lib.lib().mvdetr_add_layernorm_add_bf16(0, buf.data_ptr(), 0, 0, 0, 0, 0, 1, 96, 1e-5, buf.data_ptr(), 0) == 801
    norm32 = nn.LayerNorm(128).cuda()
    x = torch.randn(4, 128, device="cuda").bfloat16()
    with torch.no_grad():
        assert not fused_add_layer_norm_available(x, norm32)                 # an unconverted norm: torch's ops
        assert fused_add_layer_norm_available(x, norm32.bfloat16())
        assert not fused_add_layer_norm_available(x.cpu(), norm32)


# ---- encoder and model ------------------------------------------------------------------------------------------------------
def _mini(dtype, **kw):
    """The mini geometry with a 128-channel bottleneck: 8 heads of 16 channels, the head size of the Wildtrack model (the mini
    default, 32 channels, gives 4-channel heads, which no fused kernel -- fp32 or 16-bit -- takes)."""
    from mvdetr_amd.model import build_model
    return build_model("mini", seed=0, bottleneck_dim=128, **kw).cuda().to_inference(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_encoder_error_is_not_above_the_torch_compositions(dtype, monkeypatch):
    """DeformTransWorldFeat in 16 bits: RMS error against the fp32 oracle (same rounded parameters and input) of the HIP path
    (16-bit fused attention, 16-bit add + LayerNorm: one rounding per op) and of the 16-bit torch composition of the same
    layers (fused_inference = False, torch's add and LayerNorm: a rounding after every step).  Bar: HIP <= 1.25 x
    composition -- the quarter is allowance for one seed's luck over ~10^4 elements.  Both values are printed."""
    from mvdetr_amd.ops import MultiScaleDeformableAttention as MSDA
    import mvdetr_amd.world_feat as world_feat
    from mvdetr_amd.ops.modules import MSDeformAttn
    model = _mini(dtype)
    wf = model.world_feat
    H, W = model.Rworld_shape
    x = smooth_features(model.num_cam, 128, H, W, seed=9).to(dtype)          # [N, C, H, W]
    p = {k: v.float().cpu() for k, v in wf.state_dict().items()}
    pos = wf.pos_embedding.float().cpu()                                     # (a buffer: the oracle gets the rounded one too)
    monkeypatch.setattr(torch_oracle, "create_pos_embedding", lambda *a, **k: pos)
    want = torch_oracle.deform_trans_world_feat(p, x.float()[None], wf.encoder.reference_points.cpu())
    xin = x.cuda().permute(0, 2, 3, 1).contiguous()[None]                    # channel-last [1, N, H, W, C], as the warp hands it over
    with torch.no_grad():
        hip = wf(xin)
        assert MSDA.last_forward_kernel() == "msda_fwd_fused_half"
        monkeypatch.setattr(world_feat, "fused_add_layer_norm_available", lambda *a, **k: False)
        for m in wf.modules():
            if isinstance(m, MSDeformAttn):
                monkeypatch.setattr(m, "fused_inference", False)
        comp = wf(xin)
        assert MSDA.last_forward_kernel() != "msda_fwd_fused_half"              # (the fp32 core on upcast tensors)
    assert hip.dtype == comp.dtype == dtype and hip.shape == want.shape
    rms_hip = (hip.float().cpu() - want).pow(2).mean().sqrt().item()
    rms_comp = (comp.float().cpu() - want).pow(2).mean().sqrt().item()
    print(f"encoder RMS error vs fp32 oracle ({dtype}): HIP {rms_hip:.3e}, torch composition {rms_comp:.3e}, "
          f"output RMS {want.pow(2).mean().sqrt().item():.3e}")
    assert rms_hip <= 1.25 * rms_comp, (rms_hip, rms_comp)


@pytest.mark.parametrize("dtype", DTYPES)
def test_model_forward_and_detect_in_16_bits(dtype):
    from mvdetr_amd.ops import MultiScaleDeformableAttention as MSDA
    model = _mini(dtype)
    g = torch.Generator().manual_seed(2)
    imgs = torch.rand(1, model.num_cam, 3, *model.geom.img_shape, generator=g).cuda()          # fp32 images: features() casts
    M = torch.eye(3).repeat(1, model.num_cam, 1, 1)
    with torch.no_grad():
        (hm, off), (ihm, ioff, iwh) = model(imgs, M)
    assert last_warp_kernel() == "warp_fwd_cl_half" and MSDA.last_forward_kernel() == "msda_fwd_fused_half"
    H, W = model.Rworld_shape
    assert hm.shape == (1, 1, H, W) and off.shape == (1, 2, H, W)
    assert ihm.shape[0] == model.num_cam and ihm.shape[1] == 1 and ioff.shape[1] == 2 and iwh.shape[1] == 2
    for t_ in (hm, off, ihm, ioff, iwh):
        assert t_.dtype == dtype and torch.isfinite(t_).all()
    det = model.detect(imgs, M, cls_thres=0.05)
    assert type(det).__name__ == "Detections"
    assert det[0].dtype == torch.float32 and det[0].shape[0] == 1 and det[0].shape[-1] == 2      # fp32 ground-plane coordinates
    assert det[1].dtype == torch.float32 and torch.isfinite(det[0]).all() and int(det[3][0]) >= 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_model_runs_in_16_bits(dtype):
    from mvdetr_amd.model import build_model
    model = build_model("mini", seed=0, world_feat_arch="conv").cuda().to_inference(dtype)
    imgs = torch.rand(1, model.num_cam, 3, *model.geom.img_shape, generator=torch.Generator().manual_seed(2)).cuda()
    with torch.no_grad():
        (hm, off), _ = model(imgs, torch.eye(3).repeat(1, model.num_cam, 1, 1))
    assert last_warp_kernel() == "warp_fwd_half"                             # channel-last features -> NCHW world grid
    assert hm.dtype == off.dtype == dtype and torch.isfinite(hm).all() and torch.isfinite(off).all()
