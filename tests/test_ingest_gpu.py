"""ops.ingest_frames on the device (csrc/ingest.hip): every case of tests/test_ingest.py in float32 / float16 / bfloat16 and
both layouts against the fp64 oracle, every route pinned by the library's own kernel name, one Wildtrack-sized call for the grid
limits, and MVDeTr.ingest / detect_frames on the mini scene.

Bars (ingest_oracle.bar): 32 u 255 a_c + 2 u |ref| per element, + ulp |ref| for a 16-bit result (2^-11 float16, 2^-8 bfloat16);
no element excluded.  The device result also lies within the fp32 bar of the host path's float32 result (a 16-bit result: plus its
own rounding, ulp |host|)."""
import pytest
import torch

import ingest_cases as cases
import ingest_oracle as oracle
from mvdetr_amd import geometry
from mvdetr_amd.model import MVDeTr
from mvdetr_amd.ops import ingest_frames
from mvdetr_amd.ops.ingest import last_kernel

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DEV = "cuda"


def check(out, ref64, dtype, host32=None, what=""):
    w = oracle.worst(out, ref64, dtype)
    print(f"{what} {dtype} err/bar {w:.3f} [{last_kernel()}]")
    assert out.dtype == dtype and w <= 1.0, (what, dtype, w)
    if host32 is not None:
        # the fp32 bar between the two implementations; a 16-bit result is the device's fp32 value rounded once more
        h = host32.double().reshape(ref64.shape)
        wh = float(((out.double().cpu().reshape(ref64.shape) - h).abs() / (oracle.bar(ref64, torch.float32) + oracle.ULP[dtype] * h.abs())).max())
        assert wh <= 1.0, (what, dtype, "against the host path", wh)


@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("src,dst", cases.IDENTITY_SHAPES)
def test_identity_matches_oracle_and_host(src, dst, dtype, channels_last):
    for K in (1, 3):
        fr = cases.frames(K, *src)
        out = ingest_frames(fr.to(DEV), None, dst, dtype=dtype, channels_last=channels_last)
        assert out.shape == (K, 3) + dst
        assert out.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        assert last_kernel().startswith("ingest_identity")
        host = ingest_frames(fr, None, dst, channels_last=channels_last)
        check(out, cases.identity_ref(K, src, dst), dtype, host, f"identity {src}->{dst} K={K}")
    five = ingest_frames(fr.to(DEV).view(1, 3, *src, 3), None, dst, dtype=dtype, channels_last=channels_last)
    assert five.shape == (1, 3, 3) + dst and torch.equal(five.view(3, 3, *dst), out)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_cases(dtype):
    """equal size, a constant image, an integer translation, the reference's hflip: within the general bar of the oracle, and in
    float32 within 2 u 255 a_c of the normalised pixel itself (tests/test_ingest.py derives that bar)"""
    a = 1.0 / (255.0 * torch.tensor(oracle.STD, dtype=torch.float64).view(1, 3, 1, 1))
    exact_bar = 2 * oracle.U * 255 * a

    def pixels(fr):
        x = fr.permute(0, 3, 1, 2).double() / 255.0
        return (x - torch.tensor(oracle.MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(oracle.STD, dtype=torch.float64).view(1, 3, 1, 1)

    Hs, Ws = 12, 20
    fr = cases.frames(2, Hs, Ws)
    shifted = torch.full((2, Hs, Ws, 3), 128, dtype=torch.uint8)
    shifted[:, : Hs - 2, 3:] = fr[:, 2:, : Ws - 3]
    flipped = torch.full((2, Hs, Ws, 3), 128, dtype=torch.uint8)
    flipped[:, :, 1:] = fr.flip(2)[:, :, : Ws - 1]
    const = torch.full((2, 20, 31, 3), 37, dtype=torch.uint8)
    for what, f, M, dst, want in (("equal size", cases.frames(3, 8, 8), None, (8, 8), pixels(cases.frames(3, 8, 8))),
                                  ("constant", const, None, (33, 47), pixels(const)[:, :, :1, :1].expand(2, 3, 33, 47)),
                                  ("translation", fr, cases.translation_matrix(3, -2), (Hs, Ws), pixels(shifted)),
                                  ("hflip", fr, cases.hflip_matrix(Ws), (Hs, Ws), pixels(flipped))):
        Ms = None if M is None else M[None].repeat(f.shape[0], 1, 1)
        for cl in (True, False):
            out = ingest_frames(f.to(DEV), Ms, dst, dtype=dtype, channels_last=cl)
            check(out, oracle.ingest_oracle(f, Ms, dst), dtype, ingest_frames(f, Ms, dst), what)
            if dtype == torch.float32:
                assert bool(((out.double().cpu() - want).abs() <= exact_bar).all()), what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(cases.GENERAL_WARPS))
def test_general_warps_match_oracle_and_host(name, dtype):
    assert 0.05 <= cases.border_fraction(name) <= 0.60
    src, dst = cases.WARP_SHAPE
    fr = cases.frames(2, *src)
    M = cases.GENERAL_WARPS[name][None].repeat(2, 1, 1)
    for cl in (True, False):
        for mats in (M, M.to(DEV), M.float()):                                  # host fp64, device, host fp32 matrices
            out = ingest_frames(fr.to(DEV), mats, dst, dtype=dtype, channels_last=cl)
            assert last_kernel() == "ingest_warp"
            ref = cases.warp_ref(name) if mats.dtype == torch.float64 else oracle.ingest_oracle(fr, mats, dst)
            check(out, ref, dtype, ingest_frames(fr, mats.cpu(), dst, channels_last=cl), f"warp {name}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_cropped_view_and_copied_layouts(dtype):
    fr = cases.frames(3, 37, 53).to(DEV)
    view = fr[:, 2:-3, 5:-7]
    for M in (None, cases.GENERAL_WARPS["scale0.8_hflip"][None].repeat(3, 1, 1)):
        a = ingest_frames(view, M, (24, 35), dtype=dtype)
        assert torch.equal(a, ingest_frames(view.contiguous(), M, (24, 35), dtype=dtype))
        check(a, oracle.ingest_oracle(view.cpu(), M, (24, 35)), dtype, None, "cropped view")
    planar = fr.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert torch.equal(ingest_frames(planar, None, (24, 35), dtype=dtype), ingest_frames(fr, None, (24, 35), dtype=dtype))


@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_load_routes_wide_and_narrow_agree(dtype, channels_last):
    """Ws * 3 = 192 bytes per row and an aligned base take the 16-byte loads; the same bytes one byte further on take the byte
    loads; the values are identical"""
    src, dst = (32, 64), (16, 48)
    fr = cases.frames(2, *src)
    n = fr.numel()
    buf = torch.empty(n + 16, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    aligned = buf[:n].view(fr.shape).copy_(fr)
    wide = ingest_frames(aligned, None, dst, dtype=dtype, channels_last=channels_last)
    assert last_kernel() == "ingest_identity_wide"
    wide = wide.clone()
    shifted = buf[1:n + 1].view(fr.shape).copy_(fr)
    assert shifted.data_ptr() % 16 == 1
    narrow = ingest_frames(shifted, None, dst, dtype=dtype, channels_last=channels_last)
    assert last_kernel() == "ingest_identity_narrow"
    assert torch.equal(wide, narrow)
    check(wide, oracle.ingest_oracle(fr, None, dst), dtype, ingest_frames(fr, None, dst), "wide / narrow loads")
    # rows 16-byte aligned but the last chunk of a row reaches past its end: Ws * 3 = 150 bytes in a 160-byte pitch
    parent = torch.zeros(2, 32, 160, dtype=torch.uint8, device=DEV)
    crop = parent[:, :, :150].view(2, 32, 50, 3)
    crop.copy_(cases.frames(2, 32, 50))
    out = ingest_frames(crop, None, (16, 40), dtype=dtype, channels_last=channels_last)
    assert last_kernel() == "ingest_identity_wide"
    check(out, oracle.ingest_oracle(cases.frames(2, 32, 50), None, (16, 40)), dtype, None, "wide loads, short last chunk")


@pytest.mark.parametrize("channels_last", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_store_routes_and_ragged_tiles(dtype, channels_last):
    """an output pointer off 16-byte alignment gives the same values as an aligned one; Wo = 203 is no multiple of the pixels per
    lane (element stores), 204 / 200 are (16-byte stores) but not of the 128-column tile; Ho = 27 is ragged against the tile rows"""
    src = (40, 300)
    fr = cases.frames(2, *src)
    dfr = fr.to(DEV)
    for M in (None, cases.translation_matrix(4.5, 1.25)[None].repeat(2, 1, 1)):
        for dst in ((27, 203), (27, 204), (27, 200)):
            ref = oracle.ingest_oracle(fr, M, dst)
            out = ingest_frames(dfr, M, dst, dtype=dtype, channels_last=channels_last)
            check(out, ref, dtype, ingest_frames(fr, M, dst), f"ragged {dst}")
            n = out.numel()
            flat = torch.full((n + 8,), float("nan"), dtype=dtype, device=DEV)
            off = flat[1:n + 1]
            assert off.data_ptr() % 16 != 0
            strides = (dst[0] * dst[1] * 3, 1, dst[1] * 3, 3) if channels_last else (3 * dst[0] * dst[1], dst[0] * dst[1], dst[1], 1)
            view = off.as_strided((2, 3) + dst, strides)
            got = ingest_frames(dfr, M, dst, dtype=dtype, channels_last=channels_last, out=view)
            assert got.data_ptr() == view.data_ptr() and torch.equal(got, out)
            assert bool(torch.isnan(flat[:1]).all()) and bool(torch.isnan(flat[n + 1:]).all())        # nothing written around it


@pytest.mark.parametrize("dtype", DTYPES)
def test_direct_route_for_large_downscales(dtype):
    """8x down: the band of a tile (59 rows x 3 KiB) does not fit the LDS, the taps are read from global memory"""
    src, dst = (240, 1040), (30, 130)
    fr = cases.frames(1, *src)
    out = ingest_frames(fr.to(DEV), None, dst, dtype=dtype)
    assert last_kernel() == "ingest_identity_direct"
    check(out, oracle.ingest_oracle(fr, None, dst), dtype, ingest_frames(fr, None, dst), "direct")


def test_identity_matrix_takes_the_warp_kernel_and_agrees():
    src, dst = cases.WARP_SHAPE
    fr = cases.frames(2, *src).to(DEV)
    plain = ingest_frames(fr, None, dst)
    assert last_kernel() == "ingest_identity_wide"
    eye = ingest_frames(fr, torch.eye(3)[None].repeat(2, 1, 1), dst)
    assert last_kernel() == "ingest_warp"
    ref = cases.identity_ref(2, src, dst)
    check(eye, ref, torch.float32, plain.cpu(), "eye(3)")


@pytest.fixture(scope="module")
def wildtrack():
    """seven 1080 x 1920 frames (smooth ramps + noise, so that neighbouring pixels differ) and their fp64 oracles, one camera at a
    time to keep the oracle's temporaries small"""
    g = torch.Generator().manual_seed(5)
    K, Hs, Ws = 7, 1080, 1920
    fr = torch.randint(0, 256, (K, Hs, Ws, 3), dtype=torch.uint8, generator=g)
    mats = torch.stack([cases._affine((Hs, Ws), 0.7 + 0.1 * k, k % 2 == 1, 31.5 * (k - 3), -20.25 * (k - 2)) for k in range(K)])
    dst = (720, 1280)
    ident = torch.cat([oracle.ingest_oracle(fr[k:k + 1], None, dst) for k in range(K)])
    warped = torch.cat([oracle.ingest_oracle(fr[k:k + 1], mats[k:k + 1], dst) for k in range(K)])
    return fr, mats, dst, ident, warped


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_wildtrack_size(wildtrack, dtype):
    fr, mats, dst, ident, warped = wildtrack
    dfr = fr.to(DEV)
    out = ingest_frames(dfr, None, dst, dtype=dtype)
    assert last_kernel() == "ingest_identity_wide" and out.shape == (7, 3) + dst
    check(out, ident, dtype, None, "wildtrack identity")
    out = ingest_frames(dfr.view(1, 7, 1080, 1920, 3), mats.view(1, 7, 3, 3), dst, dtype=dtype)
    assert last_kernel() == "ingest_warp" and out.shape == (1, 7, 3) + dst
    check(out, warped, dtype, None, "wildtrack, one matrix per camera")


@pytest.fixture(scope="module")
def mini():
    geom = geometry.MINI
    Ks, Rts = geometry.synthetic_rig(geom, seed=0)
    torch.manual_seed(0)
    model = MVDeTr(geom, Ks, Rts).to(DEV).eval()
    g = torch.Generator().manual_seed(3)
    frames = torch.randint(0, 256, (1, geom.num_cam) + tuple(geom.img_shape) + (3,), dtype=torch.uint8, generator=g)
    M = torch.stack([cases._affine(geom.img_shape, 0.9 + 0.1 * k, k == 1, 6.5 * k, -3.25) for k in range(geom.num_cam)])[None].float()
    return model, frames, M


def test_model_ingest_feeds_the_trunk_without_a_copy(mini):
    model, frames, M = mini
    H, W = model.geom.input_img_shape
    imgs = model.ingest(frames.to(DEV))
    assert imgs.shape == (1, model.num_cam, 3, H, W) and imgs.dtype == torch.float32
    assert imgs.view(-1, 3, H, W).is_contiguous(memory_format=torch.channels_last)
    check(imgs, oracle.ingest_oracle(frames, None, (H, W)), torch.float32, None, "model.ingest")
    seen = []
    hook = model.base.register_forward_pre_hook(lambda mod, inp: seen.append((inp[0].data_ptr(), inp[0].shape)))
    with torch.no_grad():
        model.features(imgs)
    hook.remove()
    assert seen == [(imgs.data_ptr(), (model.num_cam, 3, H, W))]
    one = model.ingest(frames[0].to(DEV))                                       # [N, Hs, Ws, 3]: one frame
    assert torch.equal(one, imgs)


def test_detect_frames_is_detect_of_ingest(mini):
    """detect_frames(frames, M) is detect(model.ingest(frames, M), M or identity), bit for bit in every part that is a function of
    its input: hooks on the model show that the forward inside detect_frames is fed exactly ingest's images (same bits, same
    memory format) and exactly M, and that the detections are those of detect's extraction on that very forward's maps.  The
    trunk in between is MIOpen's: two forwards of one model on the same input need not agree to the last bit on the device
    (tests/test_detect_gpu.py), so the two calls' detections are not compared across two forwards."""
    from mvdetr_amd.ops.detect import bev_detect
    model, frames, M = mini
    dfr = frames.to(DEV)
    kw = dict(cls_thres=0.05)
    for mats in (None, M):
        want_imgs = model.ingest(dfr, mats)
        want_M = torch.eye(3).repeat(1, model.num_cam, 1, 1) if mats is None else mats
        fed, maps = [], []
        hooks = [model.register_forward_pre_hook(lambda mod, args: fed.append(args)),
                 model.register_forward_hook(lambda mod, args, out: maps.append(out[0]))]
        try:
            a = model.detect_frames(dfr, mats, **kw)
        finally:
            for h in hooks:
                h.remove()
        assert len(fed) == 1 and len(maps) == 1
        imgs, m_in = fed[0]
        assert imgs.shape == want_imgs.shape and imgs.stride() == want_imgs.stride() and torch.equal(imgs, want_imgs)
        assert torch.equal(m_in.cpu().float(), want_M)
        b = bev_detect(maps[0][0], maps[0][1], world_reduce=model.geom.world_reduce, **kw)
        assert int(a.count.sum()) > 0
        for x, y in zip((a.xy, a.score, a.cell, a.count), (b.xy, b.score, b.cell, b.count)):
            assert torch.equal(x, y)


def test_model_ingest_in_bfloat16(mini):
    import copy
    model, frames, M = mini
    half = copy.deepcopy(model).to_inference(torch.bfloat16)
    H, W = half.geom.input_img_shape
    imgs = half.ingest(frames.to(DEV), M)
    assert imgs.dtype == torch.bfloat16 and imgs.view(-1, 3, H, W).is_contiguous(memory_format=torch.channels_last)
    check(imgs, oracle.ingest_oracle(frames, M.view(-1, 3, 3), (H, W)), torch.bfloat16, None, "bfloat16 model.ingest")
    seen = []
    hook = half.base.register_forward_pre_hook(lambda mod, inp: seen.append(inp[0].data_ptr()))
    with torch.no_grad():
        half.features(imgs)
    hook.remove()
    assert seen == [imgs.data_ptr()]
