"""Shared references and checks for the 16-bit deformable-convolution tests (CPU and GPU).  Built from
tests/deform_conv_cases.py and tests/deform_conv_oracle.py alone; nothing is imported from mvdetr_amd.

The bar, on EVERY element:  |out - ref| <= u |ref| + bars(...)["out"],  u = 2^-11 (float16) or 2^-8 (bfloat16): one rounding
of the result to the storage type plus the committed fp32 error model of the sum.  ref is the fp64 oracle on the inputs
ROUNDED to the dtype (what the kernel is given), and the bars are taken on those values too.  Pooled over a set of cases, at
least 99 % of the elements must equal rn16(ref): a kernel that rounds once and accumulates in fp32 does; one that rounds the
sampled column to 16 bits does not (tests/test_deform_conv_half.py shows both from torch alone)."""
import functools

import torch

import deform_conv_cases as cases
from deform_conv_oracle import columns, deform_conv2d as oracle
from helpers import ulp_of

DTYPES = [torch.float16, torch.bfloat16]
HALF_MIN = 2.0 ** -14                      # the smallest normal float16
SMALL_CASES = ("k3_default", "k3_s2_rem_c16")     # run with x and bias scaled by 2^-4 in float16


def scale_of(kind):
    return 2.0 ** -4 if kind.endswith("_small") else 1.0


@functools.lru_cache(maxsize=None)
def rounded_reference(name, dtype, kind="random"):
    """((x, off, w, b) rounded to dtype on the CPU, fp64 oracle output, fp32 bar of the output).  kind: "random", "dyadic",
    "random_small" (x and bias scaled by 2^-4 before the rounding), "nonfinite" (20 taps given a NaN, +-inf or +-60000 by
    cases.poison), "nonfinite_moved" (the same taps at a finite position far outside: the reference of both) or "nobias"."""
    case = cases.by_name(name)
    base = "dyadic" if kind == "dyadic" else "random"
    x, off, w, b, gout = cases.matrix_reference(name, base)[0]
    s = scale_of(kind)
    x, off, w, b = (x * s).to(dtype), off.to(dtype), w.to(dtype), (b * s).to(dtype)
    ref_off = off
    if kind in ("nonfinite", "nonfinite_moved"):
        bad, finite, _ = cases.poison(case, off.float(), 7)
        bad = torch.where(bad.abs() == 1e9, bad.sign() * 60000, bad)           # (+-1e9 is not a float16)
        ref_off = finite.to(dtype)
        off = bad.to(dtype) if kind == "nonfinite" else ref_off
    if kind == "nobias":
        b = None
    ref = oracle(x, ref_off, w, b, **case.conf)
    bar = cases.bars(case, x.float(), ref_off.float(), w.float(), None if b is None else b.float(), gout)["out"]
    return (x, off, w, b), ref, bar


def bar_ratio_and_equal(out, ref, fbar, dtype):
    """(largest |out - ref| / (u |ref| + bar) over ALL elements, number of elements equal to rn16(ref), number of elements)."""
    assert out.dtype == dtype and out.shape == ref.shape, (out.dtype, out.shape, ref.shape)
    o = out.detach().cpu()
    assert torch.isfinite(o).all()
    bar = ulp_of(dtype) * ref.abs() + fbar
    err = (o.double() - ref).abs()
    ratio = torch.where(bar > 0, err / bar, torch.where(err > 0, torch.full_like(err, float("inf")), err)).max().item()
    return ratio, int((o == ref.to(dtype)).sum()), o.numel()


def flush16(t):
    """float16 values with the subnormal ones sent to 0 (what a matrix unit that flushes its operands would see)."""
    return torch.where(t.float().abs() < HALF_MIN, torch.zeros_like(t), t)


def composition(name, dtype, kind, scheme):
    """The fp32-accumulated composition on the rounded inputs of the case, with the sampled column (fp32) entering the product
    with the weight as 16-bit numbers:
      "one"            rn16(col): the column rounded once
      "two"            hi = rn16(col), lo = rn16(col - hi): dc_fwd_mfma_half's bfloat16 form
      "two_flushed"    the same with subnormal float16 column operands flushed to 0
      "scaled_flushed" float16 form: a |col| below 2^-14 has hi = 0, lo = rn16(2^11 (col - hi)) accumulated on its own and
                       folded in as acc + 2^-11 acc_lo; subnormal column operands flushed to 0"""
    case = cases.by_name(name)
    (x, off, w, b), _, _ = rounded_reference(name, dtype, kind)
    col = columns(x, off, case.kh, case.kw, **case.conf).float()               # [B, C, T, Ho, Wo]
    wf = w.float().reshape(case.C_out, case.C, case.kh * case.kw)

    def gemm(c16):
        return torch.einsum("okt,bkthw->bohw", wf, c16.float())
    if scheme == "one":
        acc = gemm(col.to(dtype))
    elif scheme in ("two", "two_flushed"):
        hi = col.to(dtype)
        lo = (col - hi.float()).to(dtype)
        if scheme == "two_flushed":
            hi, lo = flush16(hi), flush16(lo)
        acc = gemm(hi) + gemm(lo)
    elif scheme == "scaled_flushed":
        hi = torch.where(col.abs() < HALF_MIN, torch.zeros_like(col), col).to(dtype)
        lo = ((col - hi.float()) * 2048.0).to(dtype)
        acc = gemm(flush16(hi)) + gemm(flush16(lo)) * (1.0 / 2048.0)
    else:
        raise ValueError(scheme)
    if b is not None:
        acc = acc + b.float()[None, :, None, None]
    return acc.to(dtype)
