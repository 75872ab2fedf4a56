"""fp64 torch restatement of torchvision's deform_conv2d (v1) contract, for the deformable-convolution tests.

Explicit bilinear corner gathers with per-corner validity; gradients come from autograd (the floor is held fixed, so the
offset gradient is the derivative of the bilinear weights -- one-sided at integer coordinates).  Imports nothing from
mvdetr_amd.

Contract: tap (i, j) of output pixel (h, w), offset group g, samples input channel c of group g at
  y = h * stride_h - pad_h + i * dil_h + offset[:, 2 * (g * kh * kw + i * kw + j)],  x likewise with the next channel,
in pixel units; the sample is 0 when y <= -1, y >= H, x <= -1 or x >= W, else bilinear over the corners
(floor(y) or floor(y) + 1, floor(x) or floor(x) + 1) where corners outside the image contribute 0.
out[b, o] = bias[o] + sum_{c, i, j} weight[o, c, i, j] * sample(c, i, j).
"""
import torch


def _pair(v):
    return (int(v), int(v)) if not isinstance(v, (tuple, list)) else (int(v[0]), int(v[1]))


def columns(input, offset, kh, kw, stride=1, padding=0, dilation=1):
    """The sampled columns [B, C, kh * kw, H_out, W_out] in fp64 (differentiable w.r.t. input and offset)."""
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    x = input.double()
    off = offset.double()
    B, C, H, W = x.shape
    T = kh * kw
    G = off.shape[1] // (2 * T)
    Cg = C // G
    Ho, Wo = off.shape[2], off.shape[3]
    base_y = (torch.arange(Ho, dtype=torch.float64) * sh - ph)[:, None]
    base_x = (torch.arange(Wo, dtype=torch.float64) * sw - pw)[None, :]
    flat = x.reshape(B, C, H * W)
    per_group = []
    for g in range(G):
        xg = flat[:, g * Cg:(g + 1) * Cg]
        taps = []
        for t in range(T):
            i, j = divmod(t, kw)
            y = base_y + i * dh + off[:, 2 * (g * T + t)]                   # [B, Ho, Wo]
            xx = base_x + j * dw + off[:, 2 * (g * T + t) + 1]
            inside = (y > -1) & (y < H) & (xx > -1) & (xx < W)
            y0, x0 = torch.floor(y).detach(), torch.floor(xx).detach()
            ly, lx = y - y0, xx - x0
            acc = torch.zeros(B, Cg, Ho, Wo, dtype=torch.float64)
            for cy, cx, wgt in ((y0, x0, (1 - ly) * (1 - lx)), (y0, x0 + 1, (1 - ly) * lx),
                                (y0 + 1, x0, ly * (1 - lx)), (y0 + 1, x0 + 1, ly * lx)):
                valid = inside & (cy >= 0) & (cy <= H - 1) & (cx >= 0) & (cx <= W - 1)
                idx = (cy.clamp(0, H - 1) * W + cx.clamp(0, W - 1)).long().reshape(B, 1, Ho * Wo)
                vals = torch.gather(xg, 2, idx.expand(B, Cg, Ho * Wo)).reshape(B, Cg, Ho, Wo)
                acc = acc + torch.where(valid[:, None], wgt[:, None] * vals, torch.zeros((), dtype=torch.float64))
            taps.append(acc)
        per_group.append(torch.stack(taps, 2))                               # [B, Cg, T, Ho, Wo]
    return torch.cat(per_group, 1)


def deform_conv2d(input, offset, weight, bias=None, stride=1, padding=0, dilation=1):
    """fp64 [B, C_out, H_out, W_out]."""
    Co, C, kh, kw = weight.shape
    col = columns(input, offset, kh, kw, stride, padding, dilation)          # [B, C, T, Ho, Wo]
    out = torch.einsum("okt,bkthw->bohw", weight.double().reshape(Co, C, kh * kw), col)
    if bias is not None:
        out = out + bias.double()[None, :, None, None]
    return out


def with_grads(input, offset, weight, bias, grad_out, **kw):
    """(out, grad_input, grad_offset, grad_weight, grad_bias) of the fp64 restatement for the upstream gradient grad_out."""
    leaves = [t.detach().double().requires_grad_(True) if t is not None else None for t in (input, offset, weight, bias)]
    out = deform_conv2d(*leaves, **kw)
    out.backward(grad_out.double())
    return (out.detach(),) + tuple(t.grad if t is not None else None for t in leaves)


def positions(offset, kh, kw, stride=1, padding=0, dilation=1):
    """Sampling positions (y, x), each [B, G * kh * kw, H_out, W_out], fp64."""
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    off = offset.double()
    B, _, Ho, Wo = off.shape
    T = kh * kw
    G = off.shape[1] // (2 * T)
    t = torch.arange(G * T) % T
    iy, jx = (t // kw).double(), (t % kw).double()
    y = (torch.arange(Ho, dtype=torch.float64) * sh - ph)[None, None, :, None] + (iy * dh)[None, :, None, None] + off[:, 0::2]
    x = (torch.arange(Wo, dtype=torch.float64) * sw - pw)[None, None, None, :] + (jx * dw)[None, :, None, None] + off[:, 1::2]
    return y, x
