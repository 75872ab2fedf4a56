"""16-bit deformable convolution, the part that needs no GPU: the new C-ABI symbols and their refusals, the API contracts of
ops.deform_conv2d and MVDeTr.to_inference on the CPU, and a proof -- made from torch and tests/deform_conv_oracle.py alone --
that the bar of tests/test_deform_conv_half_gpu.py discriminates: the fp32-accumulated composition with the sampled column
split into TWO 16-bit terms (what dc_fwd_mfma_half computes) stays inside it, the same composition with the column rounded to
16 bits ONCE exceeds it."""
import ctypes
import os
import re

import pytest
import torch

import deform_conv_cases as cases
import deform_conv_half_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c.name for c in cases.MFMA_CASES]


def test_new_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from mvdetr_amd import _lib
    with open(os.path.join(ROOT, "include", "mvdetr_ops.h")) as f:
        hdr = f.read()
    lib = _lib.lib()
    for name in ("mvdetr_deform_conv2d_forward_f16", "mvdetr_deform_conv2d_forward_bf16"):
        assert re.search(rf"\b{name}\(", hdr) and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 18 and lib.mvdetr_ops_abi_version() == 18


def test_entries_refuse_before_they_touch_the_device():
    """No GPU is needed to be refused: the pointers below are never read (16-byte aligned host memory)."""
    from mvdetr_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_char * 256)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    #        B  C   H  W  Co  kh kw sh sw ph pw dh dw G nhwc relu
    geom = [1, 32, 4, 4, 32, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 0]
    for fn in (lib.mvdetr_deform_conv2d_forward_f16, lib.mvdetr_deform_conv2d_forward_bf16):
        def call(ptrs=(p, p, p, p), out=p, stride=32 * 16, **kw):
            g = list(geom)
            for k, v in kw.items():
                g[{"C": 1, "Co": 4, "G": 13, "nhwc": 14}[k]] = v
            return fn(None, *ptrs, *g, stride, out)
        assert call(C=5) != 0                                      # channels not a multiple of 16
        assert call(C=48, Co=48) != 0                              # output channels not a multiple of 32
        assert call(ptrs=(None, p, p, p)) != 0                     # a null input
        assert call(ptrs=(p, None, p, p)) != 0 and call(ptrs=(p, p, None, p)) != 0 and call(out=None) != 0
        assert call(G=2) != 0 and call(nhwc=0) != 0
        assert call(ptrs=(p + 2, p, p, p)) != 0 and call(ptrs=(p, p, p + 2, p)) != 0      # misaligned input / weight
        assert call(stride=32 * 16 - 1) != 0                       # the batch stride does not hold one item


def test_api_contracts_on_the_cpu():
    from mvdetr_amd.model import build_model
    from mvdetr_amd.ops import deform_conv2d
    x, w, off = torch.randn(1, 16, 5, 5), torch.randn(32, 16, 3, 3), torch.zeros(1, 18, 3, 3)
    for dtype in hc.DTYPES:
        with pytest.raises(RuntimeError, match="mvdetr_ops"):      # no 16-bit host path
            deform_conv2d(x.to(dtype), off.to(dtype), w.to(dtype))
        with pytest.raises(NotImplementedError, match="deform_conv") as e:
            build_model("mini", seed=0, world_feat_arch="deform_conv", channels_last=False).to_inference(dtype)
        assert "CUDA" in str(e.value)


def pooled(dtype, kind, scheme, names):
    """[(name, err / bar)], pooled share of outputs equal to rn16(ref)"""
    ratios, eq, n = [], 0, 0
    for name in names:
        _, ref, bar = hc.rounded_reference(name, dtype, kind)
        r, e, m = hc.bar_ratio_and_equal(hc.composition(name, dtype, kind, scheme), ref, bar, dtype)
        ratios.append((name, r))
        eq, n = eq + e, n + m
    return ratios, eq / n


@pytest.mark.parametrize("dtype", hc.DTYPES, ids=["f16", "bf16"])
def test_the_bar_tells_two_terms_from_one(dtype):
    """Two terms: inside the bar on every MFMA case, >= 99 % of the outputs correctly rounded (pooled).  One term: outside the
    bar on at least 10 of the 12 cases, fewer than 70 % correctly rounded."""
    two, share2 = pooled(dtype, "random", "two", NAMES)
    one, share1 = pooled(dtype, "random", "one", NAMES)
    print(f"DCHALF cpu {dtype} two-term max err/bar {max(r for _, r in two):.3f} share {share2:.4f}; "
          f"one-term max {max(r for _, r in one):.1f} share {share1:.4f}")
    for name, r in two:
        assert r <= 1.0, (name, r)
    assert share2 >= 0.99, share2
    assert sum(r > 1.0 for _, r in one) >= 10, one
    assert share1 < 0.70, share1


def test_float16_small_values_need_the_scaled_lo_term():
    """x and bias scaled by 2^-4: most of the column's lo terms, and some of its hi terms, are subnormal float16.  With such
    operands flushed to 0 the kernel's scheme (hi = 0 below 2^-14, lo scaled by 2^11 into accumulators of its own) holds the
    bar and the 99 %; the plain two-term split does not."""
    dtype = torch.float16
    scaled, share_s = pooled(dtype, "random_small", "scaled_flushed", hc.SMALL_CASES)
    plain, share_p = pooled(dtype, "random_small", "two_flushed", hc.SMALL_CASES)
    print(f"DCHALF cpu small scaled {scaled} share {share_s:.4f}; plain {plain} share {share_p:.4f}")
    for name, r in scaled:
        assert r <= 1.0, (name, r)
    assert share_s >= 0.99, share_s
    for name, r in plain:
        assert r > 1.0, (name, r)
    assert share_p < 0.99, share_p
