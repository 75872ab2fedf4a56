"""The refusals of the deformable-convolution and attention route tables (tests/test_deform_conv_route.py,
tests/test_attention_route.py) through the built library, without a GPU: every row whose status is not `ok` is made as a C ABI call
on host pointers or nulls and must return the status's code -- 0 for an empty call, 1 (hipErrorInvalidValue), 801
(hipErrorNotSupported) -- and leave *_last_kernel() alone.  Such a call returns before the library touches the device or any of
the pointers (the attention entries read the host array of strides, which is real here); no `ok` row is called.

And mvdetr_deform_conv2d_route_kind / mvdetr_attention_route_kind, the questions the Python layer asks, answer every row they can
express (all pointers given, one alignment flag, any out_batch_stride) as the table does."""
import ctypes

import pytest

from mvdetr_amd import _lib
from test_attention_route import ROWS as ATTN_ROWS
from test_deform_conv_route import ROWS as DC_ROWS

CODES = {"empty": 0, "invalid_value": 1, "not_supported": 801}
SUFFIXES = {4: ("f32",), 8: ("f64",), 2: ("f16", "bf16")}
DC_NAMES = {"dc_fwd_generic": "fwd_generic", "dc_fwd_mfma": "fwd_mfma", "dc_fwd_mfma_half": "fwd_mfma_half", "dc_bwd_generic": "bwd_generic",
            "dc_bwd_mfma": "bwd_mfma", "zero_fill": "bwd_zero_fill"}
ENTRIES = {"forward": _lib.ROUTE_FORWARD, "backward": _lib.ROUTE_BACKWARD, "half": _lib.ROUTE_FORWARD_HALF}

_BUF = ctypes.create_string_buffer(64)
BASE = (ctypes.addressof(_BUF) + 15) // 16 * 16          # a 16-byte aligned host address that nothing dereferences


def ptr(given, offset=0):
    return BASE + offset if given else None


def refused(rows):
    return [pytest.param(args, want, id=f"{i}-{args[0]}{args[1]}-{want}") for i, (args, want) in enumerate(rows) if want in CODES]


def dc_call(lib, sfx, args):
    entry, elem, *rest = args
    shape, nhwc, obs, f = rest[:14], rest[14], rest[15], rest[16:]
    has, (in16, wt16, rest2) = f[:8], f[8:]
    # misaligned: 4 bytes off a 16-byte boundary (a whole element of every type); the 16-bit entry's other pointers: an odd address
    inp, off, wt, out = ptr(has[0], 0 if in16 else 4), ptr(has[1], 0 if rest2 else 1), ptr(has[2], 0 if wt16 else 4), ptr(has[3])
    if entry == "forward":
        return getattr(lib, f"mvdetr_deform_conv2d_forward_{sfx}")(None, inp, off, wt, None, *shape, nhwc, out)
    if entry == "half":
        return getattr(lib, f"mvdetr_deform_conv2d_forward_{sfx}")(None, inp, off, wt, None, *shape, nhwc, 0, obs, out)
    return getattr(lib, f"mvdetr_deform_conv2d_backward_{sfx}")(None, ptr(has[4]), inp, off, wt, *shape, nhwc, ptr(has[5]), ptr(has[6]),
                                                                ptr(has[7]))


def attn_call(lib, sfx, args):
    entry, elem, B, H, Sq, Sk, D, p, tile, has_strides, strides_ok, *f = args
    has, al = f[:10], f[10]
    q, k, v, out, lse, go, work, gq, gk, gv = (ptr(h, 0 if al or i else 4) for i, h in enumerate(has))      # misaligned: q
    unit = 8 if entry == "half" else 4
    strides = (ctypes.c_int64 * 24)(*([unit * D] * 23 + [unit * D if strides_ok else unit * D + 1])) if has_strides else None
    if entry == "half":
        # (the last of ITS 12 strides carries the flag)
        strides = (ctypes.c_int64 * 12)(*([8 * D] * 11 + [8 * D if strides_ok else 8 * D + 1])) if has_strides else None
        return getattr(lib, f"mvdetr_attn_forward_{sfx}")(None, q, k, v, strides, B, H, Sq, Sk, D, out)
    if entry == "forward":
        if has_strides and not strides_ok:
            strides[11] += 1                                # (one of the forward's 12)
        return getattr(lib, f"mvdetr_attention_forward_{sfx}")(None, q, k, v, strides, B, H, Sq, Sk, D, float(p), 0, out, lse)
    return getattr(lib, f"mvdetr_attention_backward_{sfx}")(None, go, q, k, v, out, lse, strides, B, H, Sq, Sk, D, float(p), 0, work, gq,
                                                            gk, gv)


@pytest.mark.parametrize("args,want", refused(DC_ROWS))
def test_deform_conv_refusals_return_their_code_and_launch_nothing(args, want):
    lib = _lib.lib()
    before = lib.mvdetr_deform_conv2d_last_kernel()
    for sfx in SUFFIXES[args[1]]:
        assert dc_call(lib, sfx, args) == CODES[want], sfx
    assert lib.mvdetr_deform_conv2d_last_kernel() == before


@pytest.mark.parametrize("args,want", refused(ATTN_ROWS))
def test_attention_refusals_return_their_code_and_launch_nothing(args, want):
    lib = _lib.lib()
    before = lib.mvdetr_attention_last_kernel()
    for sfx in SUFFIXES[args[1]]:
        assert attn_call(lib, sfx, args) == CODES[want], sfx
    assert lib.mvdetr_attention_last_kernel() == before


def test_deform_conv_route_kind_answers_as_the_table():
    asked = 0
    for args, want in DC_ROWS:
        entry, elem, *rest = args
        shape, nhwc, obs, f = rest[:14], rest[14], rest[15], rest[16:]
        has, (in16, wt16, rest2) = f[:8], f[8:]
        mine = has[:4] if entry != "backward" else has[:3] + has[4:]
        if not all(mine) or (entry == "half" and (in16 != wt16 or not rest2 or _short_stride(args))):
            continue
        got = _lib.dc_route(ENTRIES[entry], elem, *shape, nhwc, in16)
        assert got == DC_NAMES.get(want.split()[0], want), (args, want)
        asked += 1
    assert asked >= len(DC_ROWS) * 2 // 3                  # (the rest have a null pointer or mixed alignment)


def _short_stride(args):
    """Is the row's out_batch_stride below its floor (the question assumes one that is large enough)?"""
    shape, obs = args[2:16], args[17]
    B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, G = shape
    if min(H, W, kh, kw, sh, sw, dh, dw) < 1:
        return False
    Ho, Wo = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    return obs < Co * Ho * Wo


def test_attention_route_kind_answers_as_the_table():
    asked = 0
    for args, want in ATTN_ROWS:
        entry, elem, B, H, Sq, Sk, D, p, tile, has_strides, strides_ok, *f = args
        has, al = f[:10], f[10]
        mine = has[:4] if entry == "half" else has[:5] if entry == "forward" else has
        if not has_strides or not all(mine):
            continue
        got = _lib.attn_route(ENTRIES[entry], elem, B, H, Sq, Sk, D, float(p), strides_ok, al)
        assert got == want.split()[0].replace("attn_", ""), (args, want)
        asked += 1
    assert asked >= len(ATTN_ROWS) * 2 // 3
