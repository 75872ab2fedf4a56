"""Shared cases, per-element fp32 bars and mutants for the deformable-convolution tests (CPU and GPU).  Everything here is
built from tests/deform_conv_oracle.py in fp64; nothing is imported from mvdetr_amd.

Geometry matrix.  MFMA_CASES puts every geometry on the MFMA route (C in {16, 32, 48, 160}, C_out in {32, 64, 160, 256});
GENERIC_CASES are their twins with odd channel counts or two offset groups.  A case is
(name, kh, kw, stride, padding, dilation, C, C_out, H, W, B, offset_groups).

Bars (eps = 2^-24; |.| operands throughout, so every bar is a sum of non-negative terms over exactly the terms of the
quantity it bounds).  With v_k the four corner values of a tap, w_k = wy_k * wx_k its bilinear weights, (ly, lx) the
fractions and (y, x) the sampling position:
  cola  = sum_k w_k |v_k|                                         the sample of |x|
  sy    = (1 - lx) |v2 - v0| + lx |v3 - v1|   (sx likewise)       |d sample / d y|
  cross = |v3 - v1 - v2 + v0|                                     |d^2 sample / dy dx|
  pe    = |y| sy + |x| sx                                         the sample's move when y and x are rounded once (eps |y| px)
  gcola = sum_o |w[o, c, t]| |gout[o, p]|                         bound of |g_col|
  out[o, p]          : eps ((K + 8) (|bias[o]| + sum_ct |w| cola) + sum_ct |w| pe),    K = C kh kw
  grad_weight[o,c,t] : eps ((P + 8) sum_p |gout| cola + sum_p |gout| pe),              P = B Ho Wo
  grad_offset_y[t,p] : eps ((Cg + C_out + 8) sum_c gcola sy + |x| sum_c gcola cross),  Cg = C / offset_groups (x likewise)
  grad_input[c, q]   : eps ((C_out + 8 + N_q) sum w_k gcola + sum (|y| wx_k + |x| wy_k) gcola) over the N_q corner
                       contributions that land on pixel q
  grad_bias[o]       : eps min((ceil(log2 P) + 8) sum_p |gout|, P max|gout|)        one tree sum (torch.sum)
The chain lengths are those of a sum taken in any order (K products, P pixels, N_q atomics, C_out for g_col); + 8 covers
the roundings inside one bilinear sample.  The offset gradient has no y term for d/dy: rounding y moves only ly, and
d sample / d y does not depend on ly while the floor holds (tests mask taps within 1e-4 px of a floor change or use
dyadic offsets, where every position is exact in fp32).

Mutants are what a subtly wrong implementation would return, made from the oracle alone by altering its inputs or
parameters; tests/test_deform_conv.py asserts that each one exceeds every bar it touches on every case it applies to.
"""
import functools
import math
from typing import NamedTuple, Tuple

import torch

from deform_conv_oracle import positions, with_grads

EPS32 = 2.0 ** -24
NAMES = ("out", "grad_input", "grad_offset", "grad_weight", "grad_bias")


class Case(NamedTuple):
    name: str
    kh: int
    kw: int
    stride: Tuple[int, int]
    padding: Tuple[int, int]
    dilation: Tuple[int, int]
    C: int
    C_out: int
    H: int
    W: int
    B: int
    offset_groups: int

    @property
    def conf(self):
        return dict(stride=self.stride, padding=self.padding, dilation=self.dilation)

    @property
    def out_hw(self):
        eh = self.H + 2 * self.padding[0] - self.dilation[0] * (self.kh - 1) - 1
        ew = self.W + 2 * self.padding[1] - self.dilation[1] * (self.kw - 1) - 1
        return eh // self.stride[0] + 1, ew // self.stride[1] + 1


MFMA_CASES = [
    #    name              kh kw  stride  padding dilation   C  C_out  H   W  B  G
    Case("k3_default",      3, 3, (1, 1), (1, 1), (1, 1),  32,   64,  9, 14, 2, 1),    # 126 px per item
    Case("k1x1_pad0",       1, 1, (1, 1), (0, 0), (1, 1),  32,   32,  9, 13, 2, 1),    # 117
    Case("k1x3",            1, 3, (1, 1), (0, 1), (1, 1),  16,   64,  7, 11, 2, 1),    # 77
    Case("k3x1",            3, 1, (1, 1), (1, 0), (1, 1),  48,   32, 10,  9, 2, 1),    # 90
    Case("k2x2_pad0",       2, 2, (1, 1), (0, 0), (1, 1),  32,   64,  8, 12, 3, 1),    # 7 x 11 = 77
    Case("k5x5",            5, 5, (1, 1), (2, 2), (1, 1),  16,   32,  9, 10, 2, 1),    # 90
    Case("k5x3_aniso",      5, 3, (2, 3), (3, 0), (2, 1),  32,  160, 14, 17, 2, 1),    # 6 x 5 = 30, remainders 1 and 2
    Case("k3_s2_rem_c16",   3, 3, (2, 2), (1, 1), (1, 1),  16,   64, 12, 15, 3, 1),    # 6 x 8 = 48, remainder 1 in h
    Case("k3_s2_co256",     3, 3, (2, 2), (1, 1), (1, 1),  48,  256, 11, 13, 2, 1),    # 6 x 7 = 42, no remainder
    Case("k3_d2_c160",      3, 3, (1, 1), (2, 2), (2, 2), 160,  160,  9, 11, 2, 1),    # 99
    Case("k3_pad4",         3, 3, (1, 1), (4, 4), (1, 1),  32,   32,  6,  9, 2, 1),    # 12 x 15 = 180 > H W
    Case("k3_s2_tiny",      3, 3, (2, 2), (1, 1), (1, 1),  32,   32,  8, 12, 1, 1),    # 4 x 6 = 24 <= 32 px in all
]


def _twin(case, C, C_out, G):
    return case._replace(name=case.name + f"_generic_c{C}g{G}", C=C, C_out=C_out, offset_groups=G)


# odd channels (G = 1) or two offset groups; C_out = 7 throughout
GENERIC_CASES = [_twin(c, *cg) for c, cg in zip(MFMA_CASES, [(5, 7, 1), (6, 7, 2), (5, 7, 1), (6, 7, 2), (5, 7, 1), (3, 7, 1),
                                                            (6, 7, 2), (5, 7, 1), (6, 7, 2), (5, 7, 1), (6, 7, 2), (5, 7, 1)])]
MATRIX = MFMA_CASES + GENERIC_CASES
# the shape of the first case of test_gradients_mfma_route, where a per-tensor grad_weight bar lets mutants 7 - 9 through:
# bars and mutants only
BAR_ONLY_CASES = [Case("k3_c128_18x40", 3, 3, (1, 1), (1, 1), (1, 1), 128, 128, 18, 40, 1, 1)]
DYADIC_CASES = [c for c in MATRIX if c.name.startswith(("k3_default", "k5x3_aniso"))]


def by_name(name):
    return next(c for c in MATRIX + BAR_ONLY_CASES if c.name == name)


def make_inputs(case, seed, offsets="random"):
    """(x, off, w, b, gout) in fp32 (callers take .double() for the same values in fp64).  offsets: "random" (+-3 px) or
    "dyadic" (multiples of 1/4 in [-4, 4]: every sampling position is exact in fp32)."""
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = case.out_hw
    T = case.kh * case.kw
    x = torch.randn(case.B, case.C, case.H, case.W, generator=g)
    w = torch.randn(case.C_out, case.C, case.kh, case.kw, generator=g) / (case.C * T) ** 0.5
    b = torch.randn(case.C_out, generator=g) * 0.1
    shape = (case.B, 2 * case.offset_groups * T, Ho, Wo)
    if offsets == "dyadic":
        off = torch.randint(-16, 17, shape, generator=g).float() / 4
    else:
        off = (torch.rand(shape, generator=g) - 0.5) * 6
    gout = torch.randn(case.B, case.C_out, Ho, Wo, generator=g)
    return x, off, w, b, gout


BAD_VALUES = (float("nan"), float("inf"), float("-inf"), 1e9, -1e9)


def poison(case, off, seed, n=20):
    """(bad, finite, taps): `bad` is off with n taps given a NaN, +-inf or +-1e9 in dy or dx (every value lands in both);
    `finite` has the same taps moved to a finite position far outside instead (what the result must equal: such a tap
    samples 0); `taps` is the [B, G T, Ho, Wo] map of those taps."""
    g = torch.Generator().manual_seed(seed)
    B, ch, Ho, Wo = off.shape
    bad, finite = off.clone(), off.clone()
    taps = torch.zeros(B, ch // 2, Ho, Wo, dtype=torch.bool)
    for k in range(n):
        b, t, h, w = (int(torch.randint(0, m, (1,), generator=g)) for m in (B, ch // 2, Ho, Wo))
        bad[b, 2 * t + (k // len(BAD_VALUES)) % 2, h, w] = BAD_VALUES[k % len(BAD_VALUES)]
        finite[b, 2 * t, h, w], finite[b, 2 * t + 1, h, w] = -1e4, 0.0
        taps[b, t, h, w] = True
    return bad, finite, taps


def tap_classes(case, off):
    """Boolean [B, G T, Ho, Wo] maps: the tap's four corners all inside the image; sampled with a partial footprint;
    outside (samples 0)."""
    y, x = positions(off, case.kh, case.kw, **case.conf)
    H, W = case.H, case.W
    outside = ~((y > -1) & (y < H) & (x > -1) & (x < W))
    full = (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
    return full, ~outside & ~full, outside


def smooth_mask(case, off, tol=1e-4):
    """[B, G T, Ho, Wo] True where the tap's y and x are more than tol px from an integer and from the -1 / H edges."""
    y, x = positions(off, case.kh, case.kw, **case.conf)

    def ok(v, n):
        frac = v - torch.floor(v)
        return (frac > tol) & (frac < 1 - tol) & ((v + 1).abs() > tol) & ((v - n).abs() > tol)
    return ok(y, case.H) & ok(x, case.W)


def on_grid(case, off):
    """Counts of taps exactly on an integer coordinate strictly inside, exactly on -1, and exactly on H or W."""
    y, x = positions(off, case.kh, case.kw, **case.conf)
    integer = ((y == torch.floor(y)) & (y > -1) & (y < case.H)) | ((x == torch.floor(x)) & (x > -1) & (x < case.W))
    return int(integer.sum()), int(((y == -1) | (x == -1)).sum()), int(((y == case.H) | (x == case.W)).sum())


# ---- bars ----------------------------------------------------------------------------------------------------------------

def _footprint(case, x, off):
    """Per-channel corner data, each [B, C, T, Ho, Wo] fp64: corner values v[4] (0 where the corner does not count), weight
    factors wy[4], wx[4] (0 likewise), flat pixel indices idx[4], and ly, lx, |y|, |x|, inside."""
    B, C, H, W = x.shape
    T, G = case.kh * case.kw, case.offset_groups
    Cg = C // G
    Ho, Wo = case.out_hw
    y, xx = positions(off, case.kh, case.kw, **case.conf)                    # [B, G T, Ho, Wo]
    inside = (y > -1) & (y < H) & (xx > -1) & (xx < W)
    y0, x0 = torch.floor(y), torch.floor(xx)
    ly, lx = y - y0, xx - x0

    def lift(a):
        return a.reshape(B, G, 1, T, Ho, Wo).expand(B, G, Cg, T, Ho, Wo).reshape(B, C, T, Ho, Wo)
    flat = x.double().reshape(B, G, Cg, H * W)
    v, wy, wx, idx = [], [], [], []
    for cy, fy, cx, fx in ((y0, 1 - ly, x0, 1 - lx), (y0, 1 - ly, x0 + 1, lx), (y0 + 1, ly, x0, 1 - lx), (y0 + 1, ly, x0 + 1, lx)):
        valid = inside & (cy >= 0) & (cy <= H - 1) & (cx >= 0) & (cx <= W - 1)
        i = (cy.clamp(0, H - 1) * W + cx.clamp(0, W - 1)).long()
        gi = i.reshape(B, G, 1, T * Ho * Wo).expand(B, G, Cg, T * Ho * Wo)
        vals = torch.gather(flat, 3, gi).reshape(B, C, T, Ho, Wo)
        m = lift(valid).double()
        v.append(vals * m)
        wy.append(lift(fy) * m)
        wx.append(lift(fx) * m)
        idx.append(lift(i))
    ins = lift(inside).double()
    return dict(v=v, wy=wy, wx=wx, idx=idx, ly=lift(ly) * ins, lx=lift(lx) * ins, ay=lift(y.abs()) * ins, ax=lift(xx.abs()) * ins,
                inside=ins)


def _scatter(vals, idx, HW):
    """sum of vals[k] ([B, C, T, Ho, Wo]) onto the pixels idx[k] -> [B, C, HW]"""
    B, C = vals[0].shape[:2]
    out = torch.zeros(B, C, HW, dtype=torch.float64)
    for val, i in zip(vals, idx):
        out.scatter_add_(2, i.reshape(B, C, -1), val.reshape(B, C, -1))
    return out


def bars(case, x, off, w, b, gout):
    """dict of the per-element fp32 bars (module docstring) for out, grad_input, grad_offset, grad_weight, grad_bias."""
    B, C, H, W = x.shape
    Co, T, G = case.C_out, case.kh * case.kw, case.offset_groups
    Cg, K = C // G, C * T
    Ho, Wo = case.out_hw
    P = B * Ho * Wo
    f = _footprint(case, x, off)
    v, ly, lx = [t.abs() for t in f["v"]], f["ly"], f["lx"]
    d = f["v"]
    cola = sum(wy * wx * a for wy, wx, a in zip(f["wy"], f["wx"], v))
    sy = ((1 - lx) * (d[2] - d[0]).abs() + lx * (d[3] - d[1]).abs()) * f["inside"]
    sx = ((1 - ly) * (d[1] - d[0]).abs() + ly * (d[3] - d[2]).abs()) * f["inside"]
    cross = (d[3] - d[1] - d[2] + d[0]).abs() * f["inside"]
    pe = f["ay"] * sy + f["ax"] * sx
    wa = w.double().abs().reshape(Co, C, T)
    ga = gout.double().abs()
    out_bar = EPS32 * torch.einsum("oct,bcthw->bohw", wa, (K + 8) * cola + pe)
    if b is not None:
        out_bar = out_bar + EPS32 * (K + 8) * b.double().abs()[None, :, None, None]
    gw_bar = EPS32 * torch.einsum("bohw,bcthw->oct", ga, (P + 8) * cola + pe).reshape(Co, C, case.kh, case.kw)
    gcola = torch.einsum("oct,bohw->bcthw", wa, ga)

    def per_group(a):                                                        # sum over the group's channels -> [B, G T, Ho, Wo]
        return a.reshape(B, G, Cg, T, Ho, Wo).sum(2).reshape(B, G * T, Ho, Wo)
    go_bar = torch.zeros(B, 2 * G * T, Ho, Wo, dtype=torch.float64)
    go_bar[:, 0::2] = EPS32 * ((Cg + Co + 8) * per_group(gcola * sy) + per_group(f["ax"] * gcola * cross))
    go_bar[:, 1::2] = EPS32 * ((Cg + Co + 8) * per_group(gcola * sx) + per_group(f["ay"] * gcola * cross))
    count = _scatter([(wy * wx > 0).double() for wy, wx in zip(f["wy"], f["wx"])], f["idx"], H * W)
    chain = _scatter([wy * wx * gcola for wy, wx in zip(f["wy"], f["wx"])], f["idx"], H * W)
    pos = _scatter([(f["ay"] * wx + f["ax"] * wy) * gcola for wy, wx in zip(f["wy"], f["wx"])], f["idx"], H * W)
    gi_bar = (EPS32 * ((Co + 8 + count) * chain + pos)).reshape(B, C, H, W)
    # one fp32 sum of P terms, taken as a tree (torch.sum): ceil(log2 P) levels (+ 8 for the vector lanes' partial sums);
    # never above the per-tensor bound P max|gout| that the gradient tests held before
    depth = math.ceil(math.log2(max(P, 2))) + 8
    gb_bar = EPS32 * torch.minimum(depth * ga.sum((0, 2, 3)), P * ga.max())
    return dict(out=out_bar, grad_input=gi_bar, grad_offset=go_bar, grad_weight=gw_bar, grad_bias=gb_bar)


def tap_mask_to_channels(mask):
    """[B, G T, Ho, Wo] tap mask -> [B, 2 G T, Ho, Wo] offset-channel mask (dy and dx of a tap share it)."""
    return mask.repeat_interleave(2, dim=1)


def ratios(got, want, bar, mask=None, positive_bar_only=False):
    """{tensor name: largest err / bar}; got and want are 5-tuples in NAMES order, mask an offset-channel mask applied to
    grad_offset only.  err == 0 counts as 0 whatever the bar; err > 0 where the bar is 0 gives inf, unless
    positive_bar_only leaves those elements out (the mutant test: a mutant must exceed a bar that is not 0)."""
    res = {}
    for name, g, t in zip(NAMES, got, want):
        err = (g.detach().cpu().double() - t).abs()
        r = err / bar[name]
        r[err == 0] = 0.0
        r[torch.isnan(r)] = float("inf")
        if positive_bar_only:
            r[bar[name] == 0] = 0.0
        if name == "grad_offset" and mask is not None:
            r = r[mask]
        res[name] = float(r.max()) if r.numel() else 0.0
    return res


def run(op, x, off, w, b, gout, case):
    """(out, grad_input, grad_offset, grad_weight, grad_bias) of op (the library's deform_conv2d) on the given tensors."""
    leaves = [t.detach().requires_grad_(True) for t in (x, off, w, b)]
    out = op(*leaves, **case.conf)
    out.backward(gout)
    return (out.detach(),) + tuple(t.grad for t in leaves)


# ---- mutants -------------------------------------------------------------------------------------------------------------
# fn(case, x, off, w, b, gout) -> the 5-tuple a wrong implementation would return, or None where it equals the truth by
# construction.  FORWARD_MUTANTS touch out and the input / offset / weight gradients; GRADIENT_MUTANTS every gradient.

def _swap_stride(case, x, off, w, b, gout):
    if case.stride[0] == case.stride[1]:
        return None
    return with_grads(x, off, w, b, gout, stride=case.stride[::-1], padding=case.padding, dilation=case.dilation)


def _no_dilation(case, x, off, w, b, gout):
    if case.dilation == (1, 1):
        return None
    return with_grads(x, off, w, b, gout, stride=case.stride, padding=case.padding, dilation=1)


def _padding_off_by_one(case, x, off, w, b, gout):
    pad = (case.padding[0] + 1, case.padding[1] + 1)
    return with_grads(x, off, w, b, gout, stride=case.stride, padding=pad, dilation=case.dilation)


def _tap_index_transposed(case, x, off, w, b, gout):
    """tap -> (tap % kh, tap / kh) instead of (tap / kw, tap % kw): a shift of each tap's base position"""
    kh, kw, T = case.kh, case.kw, case.kh * case.kw
    t = torch.arange(T)
    di = ((t % kh) - (t // kw)) * case.dilation[0]
    dj = ((t // kh) - (t % kw)) * case.dilation[1]
    if not (di.any() or dj.any()):
        return None
    shift = torch.stack([di, dj], 1).reshape(-1).repeat(case.offset_groups).double()
    return with_grads(x, off.double() + shift[None, :, None, None], w, b, gout, **case.conf)


def _swap_dy_dx(case, x, off, w, b, gout):
    swapped = torch.stack([off[:, 1::2], off[:, 0::2]], 2).reshape(off.shape)
    res = list(with_grads(x, swapped, w, b, gout, **case.conf))
    res[2] = torch.stack([res[2][:, 1::2], res[2][:, 0::2]], 2).reshape(off.shape)
    return tuple(res)


def _drop_partial_footprints(case, x, off, w, b, gout):
    _, partial, _ = tap_classes(case, off)
    moved = off.double().clone()
    moved[:, 0::2][partial] = -1e4
    return with_grads(x, moved, w, b, gout, **case.conf)


def _shift_positions(case, x, off, w, b, gout):
    return with_grads(x, off.double() + 2.0 ** -10, w, b, gout, **case.conf)


def _drop_one_grad_out(case, x, off, w, b, gout):
    g = gout.double().clone()                                                # an element in the middle, not the largest
    g[0, case.C_out // 2, g.shape[2] // 2, g.shape[3] // 2] = 0
    return with_grads(x, off, w, b, g, **case.conf)


def _drop_last_32_pixels(case, x, off, w, b, gout):
    B, Co, Ho, Wo = gout.shape
    g = gout.double().permute(1, 0, 2, 3).reshape(Co, -1).clone()           # [C_out, B Ho Wo]
    g[:, -32:] = 0
    res = list(with_grads(x, off, w, b, g.reshape(Co, B, Ho, Wo).permute(1, 0, 2, 3), **case.conf))
    res[0] = None                                                            # the forward is not touched
    return tuple(res)


FORWARD_MUTANTS = {"1_stride_swapped": _swap_stride, "2_dilation_ignored": _no_dilation, "3_padding_off_by_one": _padding_off_by_one,
                   "4_tap_index_transposed": _tap_index_transposed, "5_dy_dx_swapped": _swap_dy_dx,
                   "6_partial_footprints_dropped": _drop_partial_footprints, "7_positions_shifted_2^-10": _shift_positions}
GRADIENT_MUTANTS = {"8_one_grad_out_dropped": _drop_one_grad_out, "9_last_32_pixels_dropped": _drop_last_32_pixels}
MUTANT_TOUCHES = {**{m: ("out", "grad_input", "grad_offset", "grad_weight") for m in FORWARD_MUTANTS},
                  **{m: ("grad_input", "grad_offset", "grad_weight", "grad_bias") for m in GRADIENT_MUTANTS}}
MUTANTS = {**FORWARD_MUTANTS, **GRADIENT_MUTANTS}


# ---- references and checks shared by the host and the device tests --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matrix_reference(name, kind):
    """(inputs, oracle results, bars) of one matrix case; kind is "random" or "dyadic".  Shared with the GPU tests."""
    case = by_name(name)
    seed = 100 + [c.name for c in MATRIX + BAR_ONLY_CASES].index(name) + (50 if kind == "dyadic" else 0)
    inputs = make_inputs(case, seed, kind)
    x, off, w, b, gout = inputs
    return inputs, with_grads(x, off, w, b, gout, **case.conf), bars(case, x, off, w, b, gout)


def check_against_oracle(label, got, want, bar, dtype, mask=None):
    """fp64: every tensor within 1e-10 (1 + max|want|); fp32: every element inside its bar.  Prints the figures first."""
    if dtype == torch.float64:
        for name, g, t in zip(NAMES, got, want):
            err = (g.detach().cpu() - t).abs()
            if name == "grad_offset" and mask is not None:
                err = err[mask]
            err = err.max().item() if err.numel() else 0.0
            print(f"DCERR64 {label} {name} {err:.3e}")
            assert err <= 1e-10 * (1 + t.abs().max().item()), (label, name, err)
    else:
        r = ratios(got, want, bar, mask)
        print(f"DCBAR {label} " + " ".join(f"{k}={v:.4f}" for k, v in r.items()))
        for name, v in r.items():
            assert v <= 1.0, (label, name, v)
    for name, g, t in zip(NAMES, got, want):
        assert g.shape == t.shape and t.abs().max().item() > 0, (label, name)


NONFINITE_IDS = ["k3_default", "k5x3_aniso", "k3_default_generic_c5g1", "k5x3_aniso_generic_c6g2"]


@functools.lru_cache(maxsize=None)
def nonfinite_reference(name):
    """(inputs with NaN / inf / 1e9 offsets, the poisoned taps, oracle results and bars with those taps far outside)."""
    case = by_name(name)
    x, off, w, b, gout = matrix_reference(name, "random")[0]
    bad, finite, taps = poison(case, off, 7)
    return ((x, bad, w, b, gout), taps, with_grads(x, finite, w, b, gout, **case.conf), bars(case, x, finite, w, b, gout),
            tap_mask_to_channels(smooth_mask(case, finite)))


def check_nonfinite(label, got, name, dtype):
    inputs, taps, want, bar, mask = nonfinite_reference(name)
    for g in got:
        assert torch.isfinite(g).all(), label
    assert (got[2].cpu()[tap_mask_to_channels(taps)] == 0).all(), label
    check_against_oracle(label, got, want, bar, dtype, mask)
