"""Shared cases, layouts and mutants for the attention tests (CPU: test_attention.py, MI355X: test_attention_gpu.py).
Everything here is built from tests/attention_oracle.py in fp64; nothing is imported from mvdetr_amd except the keep mask
of a dropout case (``mvdetr_amd.ops.attention.dropout_keep_mask``, the library's statement of which elements it drops).

A case is (name, B, H, Sq, Sk, D, dtype, layout, dropout, amp, gout, fwd, bwd): the smallest shapes that reach each edge
of the kernels' tiling (attn_fwd_mfma: 128 queries per workgroup, 64-key tile pairs split in two 32-key halves;
attn_bwd_*_mfma: 128 rows per workgroup, 32 per wave, 32-row tiles of the other axis; generic: four rows per block, 64
scores at a time, channels lane + 64 c), with the route each call must take (last_kernel() without the "attn_" prefix).

layout: how q, k, v reach ``attention``, as ops.MultiheadAttention hands them over --
  dense          three contiguous [B, H, S, D] tensors;
  seq_first      head-split views of ONE [S, B, 3E] projection when Sq = Sk (packed), else of [Sq, B, E] and [Sk, B, 2E];
  batch_first    the same of [B, S, 3E], or [B, Sq, E] and [B, Sk, 2E].
gout: the gradient of the output as the backward receives it --
  proj           a head-split view of a dense [Sq, B, E] ([B, Sq, E] for batch_first) tensor, what the out-projection's
                 backward delivers; for the dense layout a contiguous [B, H, Sq, D] tensor;
  expanded       one number expanded to the output's shape (``out.sum().backward()``);
  misaligned     rows that start 4 bytes off a 16-byte boundary (token stride D + 4): the MFMA backward cannot take it;
  zero_rows      ``proj`` with the last query's row and channel 0 of every row zeroed: grad_q's last row and grad_v's
                 channel 0 are exactly 0 with a zero bar.
amp: q and k are scaled by sqrt(amp), so the logits have magnitude ~ amp.

Mutants are what a subtly wrong backward would return, made from the oracle alone; tests/test_attention.py asserts that
each exceeds the per-element bar of every gradient tensor it changes, on every case where it changes anything.
"""
import functools
import math
from typing import NamedTuple

import torch

import attention_oracle as ao

SEEDS = (0, 1, 2)
DROP_P, DROP_SEED = 0.25, 2 ** 63 + 12345


class Case(NamedTuple):
    name: str
    B: int
    H: int
    Sq: int
    Sk: int
    D: int
    dtype: torch.dtype = torch.float32
    layout: str = "dense"
    dropout: float = 0.0
    amp: float = 1.0
    gout: str = "proj"
    fwd: str = "fwd_mfma"
    bwd: str = "bwd_mfma"

    @property
    def size(self):
        return self.B, self.H, self.Sq, self.Sk, self.D


def _generic(name, *size, **kw):
    return Case(name, *size, fwd="fwd_generic", bwd="bwd_generic", **kw)


F64 = torch.float64

# Sq and Sk from {1, 31, 32, 33, 64, 96, 97, 127, 128, 129, 257} on each axis; Sq = 1 and Sk = 1 for both D
MFMA_EDGES = [
    Case("m16_1x129", 2, 2, 1, 129, 16),
    Case("m32_1x33_seq", 1, 2, 1, 33, 32, layout="seq_first"),
    Case("m32_129x1", 2, 2, 129, 1, 32),
    Case("m16_97x1_bf", 1, 3, 97, 1, 16, layout="batch_first"),
    Case("m16_33x97_seq", 2, 2, 33, 97, 16, layout="seq_first"),
    Case("m32_97x33", 1, 2, 97, 33, 32),
    Case("m16_32x32_packed", 2, 2, 32, 32, 16, layout="seq_first"),
    Case("m32_31x128", 2, 1, 31, 128, 32),
    Case("m16_128x31_bf", 1, 2, 128, 31, 16, layout="batch_first"),
    Case("m32_257x96_seq", 1, 2, 257, 96, 32, layout="seq_first"),
    Case("m16_96x257", 1, 2, 96, 257, 16),
    Case("m32_127x129", 2, 2, 127, 129, 32),
    Case("m32_64x64_packed_bf", 1, 2, 64, 64, 32, layout="batch_first"),
    Case("m16_129x129_packed", 1, 2, 129, 129, 16, layout="seq_first"),
    Case("m16_64x127", 1, 2, 64, 127, 16),
]
GOUT_FORMS = [
    Case("m16_33x97_gout_expanded", 2, 2, 33, 97, 16, gout="expanded"),
    Case("m16_33x97_gout_misaligned", 2, 2, 33, 97, 16, gout="misaligned", bwd="bwd_generic"),
    Case("m16_33x70_gout_zero_rows", 1, 2, 33, 70, 16, gout="zero_rows"),
    _generic("g20_9x65_gout_zero_rows", 1, 2, 9, 65, 20, gout="zero_rows"),
]
# channels lane + 64 c, c >= 1; B H Sq and B H Sk are no multiples of 4 in w200, w256 and w65_packed (the clamped rows)
WIDE = [
    _generic("w65_5x70", 1, 2, 5, 70, 65),
    _generic("w128_9x65_seq", 2, 2, 9, 65, 128, layout="seq_first"),
    _generic("w200_66x3", 1, 1, 66, 3, 200),
    _generic("w256_7x70", 1, 1, 7, 70, 256),
    _generic("w65_67x67_packed", 1, 1, 67, 67, 65, layout="seq_first"),
]
FP64 = [c._replace(name=c.name + "_f64", dtype=F64) for c in WIDE[:4]] + [_generic("g20_12x63_f64", 2, 3, 12, 63, 20, dtype=F64)]
DROPOUT = [
    Case("m16_33x97_drop", 2, 2, 33, 97, 16, dropout=DROP_P),
    Case("m32_129x33_drop_seq", 1, 2, 129, 33, 32, layout="seq_first", dropout=DROP_P),
    _generic("w65_5x70_drop", 1, 2, 5, 70, 65, dropout=DROP_P),
]
LARGE_LOGITS = [
    Case("m32_65x130_amp80", 1, 2, 65, 130, 32, amp=80.0),
    _generic("g4_130x63_amp80", 1, 2, 130, 63, 4, amp=80.0),
]
TABLE = MFMA_EDGES + GOUT_FORMS + WIDE + FP64 + DROPOUT + LARGE_LOGITS
assert len({c.name for c in TABLE}) == len(TABLE)


def by_name(name):
    return next(c for c in TABLE if c.name == name)


@functools.lru_cache(maxsize=None)
def make_inputs(case, seed=0):
    """(q, k, v, gout): dense fp32 [B, H, S, D] CPU tensors (fp64 cases take .double() of the same values)."""
    B, H, Sq, Sk, D = case.size
    g = torch.Generator().manual_seed(seed * 1000 + 7 * Sq + Sk + D)
    q, k, v = (torch.randn(B, H, S, D, generator=g) for S in (Sq, Sk, Sk))
    gout = torch.randn(B, H, Sq, D, generator=g)
    if case.amp != 1.0:
        q, k = q * math.sqrt(case.amp), k * math.sqrt(case.amp)
    if case.gout == "expanded":
        gout = torch.full_like(gout, 0.75)
    elif case.gout == "zero_rows":
        gout[:, :, -1] = 0.0
        gout[..., 0] = 0.0
    return q, k, v, gout


@functools.lru_cache(maxsize=None)
def keep_mask(case):
    if not case.dropout:
        return None
    from mvdetr_amd.ops.attention import dropout_keep_mask
    return dropout_keep_mask(DROP_SEED, case.dropout, *case.size[:4])


class Oracle(NamedTuple):
    out: torch.Tensor
    out_bar: torch.Tensor
    grads: tuple            # (grad_q, grad_k, grad_v) fp64
    bars: tuple             # per element
    tensor_bars: tuple      # one number per tensor, scaled by 1 / (1 - p)


@functools.lru_cache(maxsize=None)
def oracle(case, seed=0):
    """The fp64 results and every bar of a case, computed once per process."""
    q, k, v, gout = make_inputs(case, seed)
    keep, p = keep_mask(case), case.dropout
    res = ao.with_grads(q, k, v, gout, keep, p)
    return Oracle(res[0], ao.fp32_bar(q, k, v) / (1.0 - p), res[1:], ao.grad_bars_elementwise(q, k, v, gout, keep, p),
                  tuple(b / (1.0 - p) for b in ao.grad_bars(q, k, v, gout)))


# ---- layouts --------------------------------------------------------------------------------------------------------------

_PERM = {"seq_first": ((1, 2, 0, 3), (2, 0, 1, 3)), "batch_first": ((0, 2, 1, 3), (0, 2, 1, 3))}     # to [B,H,S,D]; back


def _tokens(x, layout):
    """dense [B, H, S, D] -> [S, B, E] (seq_first) or [B, S, E] (batch_first)"""
    return x.permute(_PERM[layout][1]).flatten(2)


def _heads(t, H, layout):
    """[S, B, E] or [B, S, E] -> the head-split [B, H, S, D] view"""
    return t.unflatten(-1, (H, t.shape[-1] // H)).permute(_PERM[layout][0])


class Operands(NamedTuple):
    leaves: list            # the tensors that require grad (dense q, k, v, or the packed projection(s))
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    gout: torch.Tensor
    layout: str

    def grads(self, case):
        """(grad_q, grad_k, grad_v) as dense [B, H, S, D] CPU tensors, read back from the leaves' .grad"""
        E, layout = case.H * case.D, self.layout
        if layout == "dense":
            parts = [x.grad for x in self.leaves]
        else:
            parts = [_heads(t, case.H, layout) for x in self.leaves for t in x.grad.split(E, dim=-1)]
        return [x.detach().cpu().contiguous() for x in parts]


def lay_out(case, device="cpu", dtype=None, layout=None, gout=None, seed=0):
    """The case's operands on ``device`` in ``layout`` with gout in the form ``gout`` (defaults: the case's)."""
    dtype = dtype or case.dtype
    layout = layout or case.layout
    form = gout or case.gout                   # (the values are the case's either way)
    q, k, v, gout = (x.to(device=device, dtype=dtype, copy=True) for x in make_inputs(case, seed))
    B, H, Sq, Sk, D = case.size
    if layout == "dense":
        leaves = [x.contiguous().requires_grad_(True) for x in (q, k, v)]
        views = leaves
    else:
        tq, tk, tv = (_tokens(x, layout) for x in (q, k, v))
        groups = [(tq, tk, tv)] if Sq == Sk else [(tq,), (tk, tv)]
        leaves = [torch.cat(g, -1).contiguous().requires_grad_(True) for g in groups]
        views = [_heads(t, H, layout) for x in leaves for t in x.split(H * D, dim=-1)]
    if form == "expanded":
        g = gout.flatten()[0].expand(gout.shape)
    elif form == "misaligned":
        pad = torch.zeros(B, H, Sq, D + 4, dtype=dtype, device=device)
        pad[..., 1:D + 1] = gout
        g = pad[..., 1:D + 1]
        assert g.data_ptr() % 16 == g.element_size() and g.stride(2) % 4 == 0
    elif layout == "dense":
        g = gout.contiguous()
    else:
        g = _heads(_tokens(gout, layout).contiguous(), H, layout)
    return Operands(leaves, *views, g, layout)


def run(op, case, device="cpu", dtype=None, layout=None, gout=None, seed=0):
    """Forward and backward of ``op`` (the module mvdetr_amd.ops.attention) on the case: (out, [grad_q, grad_k, grad_v]) as
    dense CPU tensors and the routes taken (None on the CPU)."""
    x = lay_out(case, device, dtype, layout, gout, seed)
    kw = dict(dropout_p=case.dropout, seed=DROP_SEED) if case.dropout else {}
    out = op.attention(x.q, x.k, x.v, **kw)
    fwd = None if device == "cpu" else op.last_kernel()
    out.backward(x.gout)
    bwd = None if device == "cpu" else op.last_kernel()
    return out.detach().cpu().contiguous(), x.grads(case), fwd, bwd


def ratio(got, want, bar):
    """max |got - want| / bar over the elements with a bar; where the bar is 0 the value is exactly 0 and must be returned so."""
    zero = bar == 0
    assert (want[zero] == 0).all() and (got[zero] == 0).all(), "an exactly-zero gradient was not returned as 0"
    err = (got.double() - want).abs()
    return (err[~zero] / bar[~zero]).max().item() if (~zero).any() else 0.0


def check_out(case, out, route, seed=0):
    o = oracle(case, seed)
    assert torch.isfinite(out).all()
    r = ratio(out, o.out, o.out_bar)
    print(f"ATBAR {route} {case.name} out {r:.3f}")
    assert r <= 1.0, (case.name, r)


def check_grads(case, grads, route, seed=0):
    """fp32 gradients within the per-element bars AND the per-tensor ones; prints ``ATBAR route case tensor err/bar``."""
    o = oracle(case, seed)
    for name, got, want, bar, tbar in zip("qkv", grads, o.grads, o.bars, o.tensor_bars):
        assert got.shape == want.shape and torch.isfinite(got).all(), name
        r = ratio(got, want, bar)
        print(f"ATBAR {route} {case.name} grad_{name} {r:.3f}")
        assert r <= 1.0, (case.name, name, r)
        assert (got.double() - want).abs().max().item() <= tbar, (case.name, name)


def check_fp64(case, out, grads, seed=0):
    """fp64 results at the host path's bars: 1e-12 for out, 1e-11 for the gradients."""
    o = oracle(case, seed)
    assert out.dtype == torch.float64 and torch.allclose(out, o.out, atol=1e-12, rtol=1e-12), case.name
    for name, got, want in zip("qkv", grads, o.grads):
        assert got.dtype == torch.float64 and torch.allclose(got, want, atol=1e-11, rtol=1e-11), (case.name, name)


# ---- mutants --------------------------------------------------------------------------------------------------------------

def _without_keys(q, k, v, gout, keep, p, idx):
    """the gradients of a backward that never visits the keys outside ``idx`` (their dk and dv stay 0)"""
    sub = ao.grads_explicit(q, k[:, :, idx], v[:, :, idx], gout, None if keep is None else keep[..., idx], p)
    dk, dv = torch.zeros(k.shape, dtype=torch.float64), torch.zeros(v.shape, dtype=torch.float64)
    dk[:, :, idx], dv[:, :, idx] = sub[1], sub[2]
    return sub[0], dk, dv


def _transpose_in_tiles(keep, tile=32):
    """keep[i, j] read at the transposed position within its 32 x 32 tile (where that position exists)"""
    Sq, Sk = keep.shape[-2:]
    i, j = torch.meshgrid(torch.arange(Sq), torch.arange(Sk), indexing="ij")
    ti, tj = i - i % tile + j % tile, j - j % tile + i % tile
    ok = (ti < Sq) & (tj < Sk)
    return keep[..., torch.where(ok, ti, i), torch.where(ok, tj, j)]


def changed(mut, want, tensor_bar):
    """A mutant changes a tensor when some element moves by more than 1e-6 of the per-tensor bar: two fp64 evaluations of
    the same gradient (autograd and the explicit formulas) differ by ~ 1e-9 of it, which is no change."""
    return (mut - want).abs().max().item() > 1e-6 * tensor_bar


def mutants(case, seed=0):
    """name -> (grad_q, grad_k, grad_v) fp64 of each wrong backward that applies to the case."""
    q, k, v, gout = make_inputs(case, seed)
    keep, p = keep_mask(case), case.dropout
    B, H, Sq, Sk, D = case.size
    res = {}
    if Sk > 1:
        res["1_last_key_left_out"] = _without_keys(q, k, v, gout, keep, p, torch.arange(Sk - 1))
    if Sk > 32:
        res["2_keys_32_63_left_out"] = _without_keys(q, k, v, gout, keep, p, torch.tensor([j for j in range(Sk) if not 32 <= j < 64]))
    g3 = gout.clone()
    g3[:, :, -1] = 0.0
    res["3_last_gout_row_zeroed"] = ao.grads_explicit(q, k, v, g3, keep, p)
    g4 = gout.clone()
    g4[-1, -1, Sq // 2, g4[-1, -1, Sq // 2].abs().argmax()] = 0.0        # (the largest of its row: not a tiny one)
    res["4_one_gout_element_zeroed"] = ao.grads_explicit(q, k, v, g4, keep, p)
    res["5_delta_omitted"] = ao.grads_explicit(q, k, v, gout, keep, p, omit_delta=True)
    good = ao.grads_explicit(q, k, v, gout, keep, p)
    res["6_scale_missing_from_dq"] = (good[0] * math.sqrt(D), good[1], good[2])
    if H >= 2:
        res["7_heads_of_k_swapped"] = ao.grads_explicit(q, k.flip(1), v, gout, keep, p)
    if p:
        res["8_keep_ignored_in_backward"] = ao.grads_explicit(q, k, v, gout, keep, p, keep_bwd=None)
        res["9_keep_transposed_in_tile"] = ao.grads_explicit(q, k, v, gout, keep, p, keep_bwd=_transpose_in_tiles(keep))
    return res
