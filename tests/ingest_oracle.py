"""fp64 oracle of ops.ingest_frames and the error bars of its tests.

The oracle is literally the reference's order (datasets/frameDataset.py:66-67,199-206 + utils/image_utils.py:43): warp the
frame by M at its own size (cv2.warpPerspective's convention: destination <- source, integer pixel centres, bilinear, constant
border; kept in float, the one documented difference from cv2), ``/255``, normalise, then ``F.interpolate`` on the double
tensor.  ``align_corners`` / ``antialias`` / ``border`` / a wrong matrix can be passed on purpose: the tests use those to show
that they would notice a wrong contract.
"""
import torch
import torch.nn.functional as F

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
U = 2.0 ** -24
ULP = {torch.float32: 0.0, torch.float64: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def warp_frames(A, M, border):
    """A [K, 3, H, W] float64 grey levels -> the same size, warped by M [K, 3, 3] (destination <- source)."""
    K, _, H, W = A.shape
    inv = torch.linalg.inv_ex(M.double())[0]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    pts = torch.stack([xs, ys, torch.ones_like(xs)], 0).reshape(3, -1)                 # [3, H W]
    uvw = inv @ pts                                                                     # [K, 3, H W]
    w = uvw[:, 2]
    px, py = uvw[:, 0] / w, uvw[:, 1] / w
    bad = ~(w > 0) | ~torch.isfinite(px) | ~torch.isfinite(py) | ~torch.isfinite(inv).all(-1).all(-1)[:, None]
    px, py = torch.where(bad, torch.full_like(px, -5.0), px), torch.where(bad, torch.full_like(py, -5.0), py)
    px, py = px.clamp(-5.0, W + 5.0), py.clamp(-5.0, H + 5.0)                           # (far outside is all border anyway)
    fx, fy = px.floor(), py.floor()
    lx, ly = (px - fx)[:, None], (py - fy)[:, None]
    flat = A.reshape(K, 3, H * W)

    def tap(yy, xx):
        ok = ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W))[:, None]
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long()[:, None].expand(K, 3, H * W)
        return torch.where(ok, flat.gather(2, idx), torch.full_like(flat, float(border)))

    top = tap(fy, fx) * (1 - lx) + tap(fy, fx + 1) * lx
    bot = tap(fy + 1, fx) * (1 - lx) + tap(fy + 1, fx + 1) * lx
    return (top * (1 - ly) + bot * ly).reshape(K, 3, H, W)


def ingest_oracle(frames, M, out_hw, mean=MEAN, std=STD, border=128, align_corners=False, antialias=False):
    """frames uint8 [K, Hs, Ws, 3] -> float64 [K, 3, Ho, Wo]"""
    A = frames.reshape((-1,) + tuple(frames.shape[-3:])).permute(0, 3, 1, 2).double()
    if M is not None:
        A = warp_frames(A, M.reshape(-1, 3, 3), border)
    A = A / 255.0
    A = (A - torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    return F.interpolate(A, size=tuple(out_hw), mode="bilinear", align_corners=align_corners, antialias=antialias)


def torch_fp32_composition(frames, out_hw, mean=MEAN, std=STD):
    """What a user would write in torch: the same order in float32 (positions formed in float32 by F.interpolate)."""
    A = frames.permute(0, 3, 1, 2).float() / 255.0
    A = (A - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)
    return F.interpolate(A, size=tuple(out_hw), mode="bilinear", align_corners=False, antialias=False)


def bar(ref64, dtype=torch.float32, std=STD):
    """Per-element bar: 32 u 255 a_c + 2 u |ref| (+ ulp |ref| for a 16-bit result), u = 2^-24, a_c = 1 / (255 std_c): up to 16
    taps with four one-ulp weight factors each on partial sums <= 255 grey levels, and one FMA."""
    a = 1.0 / (255.0 * torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1))
    return 32 * U * 255 * a + (2 * U + ULP[dtype]) * ref64.abs()


def worst(out, ref64, dtype=None, std=STD):
    """max over every element of err / bar"""
    dtype = out.dtype if dtype is None else dtype
    out = out.reshape(ref64.shape)
    return float(((out.double().cpu() - ref64).abs() / bar(ref64, dtype, std)).max())
