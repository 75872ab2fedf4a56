"""16-bit attention, the part that needs no GPU: the API contracts of ops.attention and MVDeTr.to_inference, the new C-ABI
symbols, and a proof -- made from torch alone -- that the bar of tests/test_attention_half_gpu.py discriminates: the fp32
composition with the probabilities split into TWO 16-bit terms (what attn_fwd_mfma_half computes) stays inside it, the same
composition with the probabilities rounded to 16 bits ONCE exceeds it."""
import ctypes
import functools
import importlib
import math
import os
import re

import pytest
import torch

import attention_cases as ac
import attention_oracle as ao
from helpers import ulp_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float16, torch.bfloat16]
# the cases of the GPU test: every tile edge of the fp32 MFMA kernel, the 64-query workgroup's +-1 and the large logits
EXTRA = [ac.Case("h16_63x70", 1, 2, 63, 70, 16), ac.Case("h32_65x33_seq", 2, 2, 65, 33, 32, layout="seq_first")]
CASES = ac.MFMA_EDGES + EXTRA + [ac.by_name("m32_65x130_amp80")]


@functools.lru_cache(maxsize=None)
def rounded_case(case, dtype, seed):
    """(q, k, v) of the case rounded to ``dtype`` (CPU, 16-bit), the fp64 oracle on those values and the fp32 bar."""
    q, k, v = (x.to(dtype) for x in ac.make_inputs(case, seed)[:3])
    return (q, k, v), ao.attention(q, k, v), ao.fp32_bar(q, k, v)


def bar_ratio_and_equal(out, ref, fbar, dtype):
    """max over ALL elements of |out - ref| / (u |ref| + fp32_bar), and the number of elements with out == rn16(ref)."""
    assert out.dtype == dtype and out.shape == ref.shape and torch.isfinite(out).all()
    o = out.detach().cpu()
    bar = ulp_of(dtype) * ref.abs() + fbar
    err = (o.double() - ref).abs()
    ratio = torch.where(bar > 0, err / bar, torch.where(err > 0, torch.full_like(err, float("inf")), err)).max().item()
    return ratio, int((o == ref.to(dtype)).sum()), o.numel()


def composition(q, k, v, dtype, terms):
    """torch's fp32 composition in the kernel's form: exp2 of the scores reduced by the row maximum, un-normalised P, the
    division by the row sum at the end; P enters the product with v as ``terms`` 16-bit numbers."""
    qf, kf, vf = q.float(), k.float(), v.float()
    c2 = (1.0 / math.sqrt(q.shape[-1])) * 1.4426950408889634
    s = qf @ kf.transpose(-1, -2)
    p = torch.exp2((s - s.max(-1, keepdim=True)[0]) * c2)
    hi = p.to(dtype).float()
    acc = hi @ vf
    if terms == 2:
        acc = acc + (p - hi).to(dtype).float() @ vf
    return (acc / p.sum(-1, keepdim=True)).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_bar_tells_two_terms_from_one(dtype):
    """Two terms: inside the bar on every case and seed, >= 99 % of the outputs correctly rounded (pooled per seed, as on the
    GPU).  One term: outside the bar on every case with more than one key -- except the large-logit case, whose nearly
    one-hot rows that route barely moves -- and far fewer correctly rounded.  (With ONE key the only probability is 1, which
    16 bits hold exactly: no route can differ there.)"""
    for seed in ac.SEEDS:
        same = {1: 0, 2: 0}
        total = 0
        for case in CASES:
            (q, k, v), ref, fbar = rounded_case(case, dtype, seed)
            r2, e2, n = bar_ratio_and_equal(composition(q, k, v, dtype, 2), ref, fbar, dtype)
            r1, e1, _ = bar_ratio_and_equal(composition(q, k, v, dtype, 1), ref, fbar, dtype)
            print(f"ATBAR cpu_two_terms/{dtype} {case.name} seed {seed} out {r2:.3f}   one term {r1:.3f}")
            assert r2 <= 1.0, (case.name, seed, r2)
            if case.Sk > 1 and case.amp == 1.0:
                assert r1 > 1.0, (case.name, seed, r1)
            same[1], same[2], total = same[1] + e1, same[2] + e2, total + n
        print(f"rounded-equal {dtype} seed {seed}: two terms {same[2] / total:.4f}, one term {same[1] / total:.4f}")
        assert same[2] / total >= 0.99 and same[1] / total < 0.9


def test_cpu_half_tensors_are_refused():
    A = importlib.import_module("mvdetr_amd.ops.attention")
    for dtype in DTYPES:
        x = torch.zeros(1, 1, 2, 16, dtype=dtype)
        with pytest.raises(RuntimeError, match="not implemented for"):
            A.attention(x, x, x)
        with pytest.raises(RuntimeError, match="not implemented for"):
            A.attention(x, x, x, dropout_p=0.25)
    mha = A.MultiheadAttention(32, 2).to(torch.bfloat16).eval()
    x = torch.zeros(3, 1, 32, dtype=torch.bfloat16)
    assert not mha._fused_ok(x, x, x, None, False, None, {})                  # a 16-bit CPU call stays torch's


def test_to_inference_serves_trans_on_the_gpu_only_and_refuses_deform_conv():
    from mvdetr_amd.model import build_model
    with pytest.raises(NotImplementedError, match=r"trans.*GPU") as e:
        build_model("mini", seed=0, world_feat_arch="trans", channels_last=False).to_inference(torch.bfloat16)
    assert "CUDA" in str(e.value)
    with pytest.raises(NotImplementedError, match="deform_conv"):
        build_model("mini", seed=0, world_feat_arch="deform_conv", channels_last=False).to_inference(torch.float16)


def test_new_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from mvdetr_amd import _lib
    with open(os.path.join(ROOT, "include", "mvdetr_ops.h")) as f:
        hdr = f.read()
    lib = _lib.lib()
    for name in ("mvdetr_attn_forward_f16", "mvdetr_attn_forward_bf16", "mvdetr_attn_half_set_query_tile"):
        assert re.search(rf"\b{name}\(", hdr) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 18 and lib.mvdetr_ops_abi_version() == 18
    # the entries validate before they touch the device: no GPU is needed to be refused
    strides = (ctypes.c_int64 * 12)()
    assert lib.mvdetr_attn_forward_bf16(None, None, None, None, strides, 1, 1, 4, 4, 20, None) == 801
    assert lib.mvdetr_attn_forward_f16(None, None, None, None, strides, 1, 1, 4, 0, 16, None) == 801
    assert lib.mvdetr_attn_forward_f16(None, None, None, None, strides, 0, 1, 4, 4, 16, None) == 0
    assert lib.mvdetr_attn_half_set_query_tile(96) == -1 and lib.mvdetr_attn_half_set_query_tile(0) == 0
