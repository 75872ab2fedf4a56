"""Shared by tests/test_layernorm.py (CPU) and tests/test_layernorm_edges_gpu.py / test_layernorm_gpu.py (GPU): the data
families, the fp64 oracle, the elementwise bar and a numpy emulation of the fp32 add + LayerNorm kernels' operation order
(csrc/add_layernorm.hip).

The bar.  With s = x + residual in exact arithmetic, mean / rstd its exact row statistics (biased variance, eps inside the
root), n = (s - mean) rstd, y = gamma n + beta and u = 2^-24:

    bar = K1 u max_row|s| rstd |gamma| (2 + |n|)  +  K2 u (|gamma n| + |y|)          (+ u |y + then_add| for the 2nd output)

The first term is the fp32 rounding of the sum s and of the row total (each at most u max|s| per element), carried through the
normalisation to first order: an element's own error and the mean's (the 2) and the variance's share (the |n|).  The second
covers the roundings of the output arithmetic (the centred element, the product with rstd, rstd itself, the affine step).
K1 = 2, K2 = 4: torch's CPU fp32 layer_norm on the fp32 sum and the emulation of the kernels' order both stay inside it on every
family below (tests/test_layernorm.py asserts that and prints the ratios), and each wrong algorithm listed there leaves it.
The constants may only rise if the CPU fp32 reference needs it -- never because a kernel exceeds the bar."""
import numpy as np
import torch

K1, K2 = 2.0, 4.0
U = 2.0 ** -24
COLS = (64, 128, 256)
FP32_KERNELS = {64: "add_layernorm_rows<1>", 128: "add_layernorm_rows128x2", 256: "add_layernorm_rows<4>"}     # 16-byte aligned

# name -> (mean of x, spread of x, spread of the residual, eps)
FAMILIES = {
    "a": (0.7, 3.0, 0.5, 1e-5),          # the data of tests/test_layernorm_gpu.py
    "b": (1000.0, 1.0, 0.5, 1e-5),       # mean 1000, unit spread: cancellation in s - mean
    "c": (0.3, 0.01, 0.01, 1e-5),        # variance 2e-4 with the residual: eps is 5 % of it
    "d": (0.0, 0.05, 0.01, 1e-3),        # a non-default eps that is a third of the variance
    "e": (0.0, 1.0, 0.5, 1e-12),         # eps far below fp32 resolution of the variance
}


def family(name, B, n, cols, seed=0, batch_pos=False):
    """(x [B, n, cols], residual, then_add [1 or B, n, cols], weight, bias, eps), fp32 CPU tensors, seeded by every argument."""
    mean, spread, rspread, eps = FAMILIES[name]
    g = torch.Generator().manual_seed(1000 * seed + 131 * ord(name) + 7 * cols + B * n)
    x = mean + spread * torch.randn(B, n, cols, generator=g)
    res = rspread * torch.randn(B, n, cols, generator=g)
    pos = torch.randn(B if batch_pos else 1, n, cols, generator=g)
    w = 1.0 + 0.3 * torch.randn(cols, generator=g)
    b = 0.3 * torch.randn(cols, generator=g)
    return x, res, pos, w, b, eps


def make_norm(cols, w, b, eps, device="cuda"):
    """nn.LayerNorm with these parameters (w is None: not affine)."""
    norm = torch.nn.LayerNorm(cols, eps=eps, elementwise_affine=w is not None)
    if w is not None:
        with torch.no_grad():
            norm.weight.copy_(w)
            norm.bias.copy_(b)
    return norm.to(device)


def oracle(x, res, w, b, eps, pos=None):
    """fp64 layer_norm on the fp64 sum, and the elementwise bars: (y, bar, y2, bar2) -- y2 / bar2 None without ``pos``.
    On the arguments' device (all on one)."""
    cols = x.shape[-1]
    s = x.double() if res is None else x.double() + res.double()
    gamma = torch.ones(cols, dtype=torch.float64, device=x.device) if w is None else w.double()
    beta = torch.zeros(cols, dtype=torch.float64, device=x.device) if b is None else b.double()
    y = torch.nn.functional.layer_norm(s, (cols,), gamma, beta, eps)
    rstd = (s.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
    n = (s - s.mean(-1, keepdim=True)) * rstd
    bar = K1 * U * s.abs().amax(-1, keepdim=True) * rstd * gamma.abs() * (2 + n.abs()) + K2 * U * ((gamma * n).abs() + y.abs())
    if pos is None:
        return y, bar, None, None
    y2 = y + pos.double()
    return y, bar, y2, bar + U * y2.abs()


def ratio(got, want, bar):
    """max |got - want| / bar; inf if a got element is not finite where want is."""
    err = (got.detach().to(want.device).double() - want).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return (err / bar).max().item()


def reference32(x, res, w, b, eps, pos=None):
    """The reference arithmetic in fp32 on the CPU: torch's layer_norm on the fp32 sum (and the fp32 second add)."""
    s = x if res is None else x + res
    y = torch.nn.functional.layer_norm(s, (x.shape[-1],), w, b, eps)
    return y, (None if pos is None else y + pos)


# ---- the kernels' operation order in numpy fp32 ---------------------------------------------------------------------------------
_LANE = np.arange(64)
_XOR = {o: _LANE ^ o for o in (1, 2, 4, 8, 16, 32)}
_HALF_MIRROR = (_LANE & ~7) | (7 - (_LANE & 7))          # DPP row_half_mirror
_MIRROR = (_LANE & ~15) | (15 - (_LANE & 15))            # DPP row_mirror


def _wave_sum_rows(p):
    """add_layernorm_rows<VEC>: p [rows, 64] per-lane partials; xor-shuffle butterfly 32, 16, ..., 1."""
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[:, _XOR[o]]
    return p


def _wave_sum_128x2(p):
    """ln_sum32: p [waves, 64], a row per half wave; lane ^ 1, lane ^ 2, row_half_mirror, row_mirror, lane ^ 16."""
    for idx in (_XOR[1], _XOR[2], _HALF_MIRROR, _MIRROR, _XOR[16]):
        p = p + p[:, idx]
    return p


def emulate(x, res, w, b, eps, pos=None, two_rows=False, mutation=None):
    """The fp32 kernels' arithmetic in their order of operations (plain fp32 operations; the compiler's fused multiply-adds
    and the hardware's reciprocal square root, both within an ulp of what is computed here, are not modelled): the generic
    one-row-per-wave kernel, or with ``two_rows`` add_layernorm_rows128x2.  ``mutation`` plants one wrong algorithm:
    "one_pass" (variance as E[s^2] - mean^2), "no_eps", "eps_1e-5", "unbiased" (cols - 1), "rows_swapped" (rows 0 and 1 of
    the output exchanged), "wrong_batch" (then_add read one batch element further on).  Returns (y, y2) as fp32 tensors."""
    f = np.float32
    shape, cols = x.shape, x.shape[-1]
    rows = x.numel() // cols
    s = x.reshape(rows, cols).numpy().astype(f)
    if res is not None:
        s = s + res.reshape(rows, cols).numpy().astype(f)
    if two_rows:
        assert cols == 128
        pad = rows % 2                                    # an odd count: the idle half wave repeats the last row
        v = np.concatenate([s, s[-1:]] if pad else [s]).reshape(-1, 64, 4)        # [waves, lane, 4]: lane = 32 * (row & 1) + hl
        wave_sum, per_lane = _wave_sum_128x2, lambda t: (t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3])
    else:
        pad = 0
        v = s.reshape(rows, 64, cols // 64)
        wave_sum = _wave_sum_rows

        def per_lane(t):
            acc = np.zeros(t.shape[:-1], f)
            for i in range(t.shape[-1]):
                acc = acc + t[..., i]
            return acc
    inv = f(1.0 / cols)
    mean = (wave_sum(per_lane(v)) * inv)[..., None]
    d = v - mean
    if mutation == "one_pass":
        var = wave_sum(per_lane(v * v)) * inv - mean[..., 0] * mean[..., 0]
    elif mutation == "unbiased":
        var = wave_sum(per_lane(d * d)) * f(1.0 / (cols - 1))
    else:
        var = wave_sum(per_lane(d * d)) * inv
    e = f({"no_eps": 0.0, "eps_1e-5": 1e-5}.get(mutation, eps))
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = (1.0 / np.sqrt((var + e).astype(np.float64))).astype(f)[..., None]
    y = (d * rstd).reshape(-1, cols)[:rows]
    if w is not None:
        y = y * w.numpy().astype(f) + b.numpy().astype(f)
    if mutation == "rows_swapped" and rows > 1:
        y[[0, 1]] = y[[1, 0]]
    y2 = None
    if pos is not None:
        p = pos.reshape(-1, cols).numpy().astype(f)
        shift = shape[-2] if mutation == "wrong_batch" else 0
        y2 = torch.from_numpy(y + p[(np.arange(rows) + shift) % p.shape[0]]).view(shape)
    return torch.from_numpy(y).view(shape), y2
