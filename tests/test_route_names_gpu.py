"""The `ok` side of the two route tables on the device: a dozen rows per operator of tests/test_deform_conv_route.py and
tests/test_attention_route.py, at the tables' own tiny shapes, are made as C ABI calls on device tensors.  Each returns 0, leaves
*_last_kernel() at the name the table gives the row, and -- the fp32 rows -- computes what the library's host-path entry computes
for the same arguments, within the per-element fp32 bars that tests/test_deform_conv_gpu.py and tests/test_attention_gpu.py hold
the same kernels to (fp32_bar / bars of the deformable convolution, fp32_bar / grad_bars_elementwise of the attention)."""
import ctypes

import pytest
import torch

import attention_oracle as ao
import deform_conv_cases as cases
import test_attention_route as at
import test_deform_conv_route as dt
from test_deform_conv import fp32_bar

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = {("forward", 4): torch.float32, ("backward", 4): torch.float32, ("forward", 8): torch.float64, ("backward", 8): torch.float64}
DC_TABLE, AT_TABLE = dict(dt.ROWS), dict(at.ROWS)


def _lib():
    from mvdetr_amd import _lib
    return _lib


def _within(label, got, want, bar, mask=None):
    err = (got.detach().cpu().double() - want.detach().cpu().double()).abs()
    ok = err <= bar
    if mask is not None:
        ok = ok | ~mask
    worst = (err / bar.clamp_min(1e-300))[ok].max().item() if ok.any() else 0.0
    print(f"ROUTEBAR {label} err/bar={worst:.4f}")
    assert ok.all(), (label, (err / bar.clamp_min(1e-300)).max().item())
    assert want.abs().max().item() > 0, label


DC_ROWS = [("forward", 4, {}), ("forward", 4, dict(B=2)), ("forward", 4, dict(C=32)), ("forward", 4, dict(C=24)), ("forward", 4, dict(Co=33)),
           ("forward", 4, dict(nhwc=0)), ("forward", 8, {}), ("backward", 4, {}), ("backward", 4, dict(C=24)), ("backward", 4, dict(nhwc=0)),
           ("backward", 8, {}), ("half", 2, {}), ("half", 2, dict(C=32))]


@pytest.mark.parametrize("entry,elem,kw", DC_ROWS, ids=[f"{e}{n}-{'-'.join(f'{k}{v}' for k, v in kw.items())}" for e, n, kw in DC_ROWS])
def test_deform_conv_rows_run_the_kernel_the_table_names(entry, elem, kw):
    lib = _lib().lib()
    args = dt.row(entry, elem, None, **kw)[0][0]
    name = DC_TABLE[args].split()[0]
    B, C, H, W, Co, kh, kw_, sh, sw, ph, pw, dh, dw, G = shape = args[2:16]
    nhwc = args[16]
    assert (kh, kw_, sh, sw, ph, pw, dh, dw) == (3, 3, 1, 1, 1, 1, 1, 1)      # the tables' defaults: the output is the input's size
    Ho, Wo = H, W
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, C, H, W, generator=g)
    off = (torch.rand(B, 2 * G * kh * kw_, Ho, Wo, generator=g) - 0.5) * 3
    w = torch.randn(Co, C, kh, kw_, generator=g) / (C * kh * kw_) ** 0.5
    b = torch.randn(Co, generator=g) * 0.1
    gout = torch.randn(B, Co, Ho, Wo, generator=g)
    fmt = torch.channels_last if nhwc else torch.contiguous_format
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for sfx, dtype in (("f16", torch.float16), ("bf16", torch.bfloat16)) if entry == "half" else ((_lib().suffix(DTYPES[entry, elem]), DTYPES[entry, elem]),):
        host = [t.to(dtype) for t in (x.contiguous(memory_format=fmt), off, w, b, gout)]
        xd, od, wd, bd, gd = dev = [t.to(DEV) for t in host]
        if entry == "half":
            wd = wd.permute(2, 3, 0, 1).reshape(kh * kw_, Co, C).contiguous()
            out = torch.empty(B, Co, Ho, Wo, dtype=dtype, device=DEV)
            rc = getattr(lib, f"mvdetr_deform_conv2d_forward_{sfx}")(stream, xd.data_ptr(), od.data_ptr(), wd.data_ptr(), bd.data_ptr(), *shape,
                                                                    nhwc, 0, Co * Ho * Wo, out.data_ptr())
        elif entry == "forward":
            out, out_h = torch.empty(B, Co, Ho, Wo, dtype=dtype, device=DEV), torch.empty(B, Co, Ho, Wo, dtype=dtype)
            rc = getattr(lib, f"mvdetr_deform_conv2d_forward_{sfx}")(stream, *(t.data_ptr() for t in dev[:4]), *shape, nhwc, out.data_ptr())
            assert getattr(lib, f"mvdetr_deform_conv2d_forward_host_{sfx}")(*(t.data_ptr() for t in host[:4]), *shape, nhwc, out_h.data_ptr()) == 0
        else:
            grads = [torch.zeros_like(xd), torch.empty_like(od), torch.empty_like(wd)]
            grads_h = [torch.zeros_like(host[0]), torch.empty_like(host[1]), torch.empty_like(host[2])]
            rc = getattr(lib, f"mvdetr_deform_conv2d_backward_{sfx}")(stream, gd.data_ptr(), *(t.data_ptr() for t in dev[:3]), *shape, nhwc,
                                                                     *(t.data_ptr() for t in grads))
            assert getattr(lib, f"mvdetr_deform_conv2d_backward_host_{sfx}")(host[4].data_ptr(), *(t.data_ptr() for t in host[:3]), *shape, nhwc,
                                                                            *(t.data_ptr() for t in grads_h)) == 0
        torch.cuda.synchronize()
        assert rc == 0
        assert lib.mvdetr_deform_conv2d_last_kernel().decode() == name
        if entry == "half":
            assert torch.isfinite(out.float()).all()
        elif dtype == torch.float32 and entry == "forward":
            _within(f"{name} {kw}", out, out_h, fp32_bar(x, off, w, 1, 1, 1))
        elif dtype == torch.float32:
            case = cases.Case("adhoc", kh, kw_, (sh, sw), (ph, pw), (dh, dw), C, Co, H, W, B, G)
            bars = cases.bars(case, x, off, w, b, gout)
            mask = cases.tap_mask_to_channels(cases.smooth_mask(case, off))
            for key, got, want in zip(("grad_input", "grad_offset", "grad_weight"), grads, grads_h):
                _within(f"{name} {kw} {key}", got, want, bars[key], mask if key == "grad_offset" else None)


AT_ROWS = [("forward", 4, {}), ("forward", 4, dict(D=32)), ("forward", 4, dict(D=17)), ("forward", 4, dict(Sq=129)), ("forward", 4, dict(al=0)),
           ("forward", 8, dict(D=16)), ("backward", 4, {}), ("backward", 4, dict(D=17)), ("backward", 4, dict(Sq=129, Sk=129)), ("backward", 8, {}),
           ("half", 2, {}), ("half", 2, dict(D=32)), ("half", 2, dict(Sq=64))]


def _strides(*tensors):
    flat = [s for t in tensors for s in t.stride()[:3]]
    return (ctypes.c_int64 * len(flat))(*flat)


@pytest.mark.parametrize("entry,elem,kw", AT_ROWS, ids=[f"{e}{n}-{'-'.join(f'{k}{v}' for k, v in kw.items())}" for e, n, kw in AT_ROWS])
def test_attention_rows_run_the_kernel_the_table_names(entry, elem, kw):
    lib = _lib().lib()
    args = at.row(entry, elem, None, **kw)[0][0]
    name = AT_TABLE[args].split()[0]
    B, H, Sq, Sk, D = args[2:7]
    g = torch.Generator().manual_seed(3)
    q, k, v, gout = (torch.randn(B, H, S, D, generator=g) for S in (Sq, Sk, Sk, Sq))
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def on_device(t, dtype):
        if kw.get("al", 1):
            return t.to(dtype).to(DEV)
        buf = torch.empty(t.numel() + 1, dtype=dtype, device=DEV)          # one element off a 16-byte boundary
        buf[1:].copy_(t.reshape(-1))
        return buf[1:].view(t.shape)

    for sfx, dtype in (("f16", torch.float16), ("bf16", torch.bfloat16)) if entry == "half" else ((_lib().suffix(DTYPES[entry, elem]), DTYPES[entry, elem]),):
        host = [t.to(dtype) for t in (q, k, v, gout)]
        qd, kd, vd, gd = (on_device(t, dtype) for t in host)
        out = torch.empty(B, H, Sq, D, dtype=dtype, device=DEV)
        if entry == "half":
            rc = getattr(lib, f"mvdetr_attn_forward_{sfx}")(stream, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), _strides(qd, kd, vd, out), B, H, Sq, Sk,
                                                           D, out.data_ptr())
            torch.cuda.synchronize()
            assert rc == 0 and lib.mvdetr_attention_last_kernel().decode() == name
            assert torch.isfinite(out.float()).all()
            continue
        lse, out_h, lse_h = torch.empty(B, H, Sq, dtype=dtype, device=DEV), torch.empty(B, H, Sq, D, dtype=dtype), torch.empty(B, H, Sq, dtype=dtype)
        rc = getattr(lib, f"mvdetr_attention_forward_{sfx}")(stream, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), _strides(qd, kd, vd, out), B, H, Sq, Sk,
                                                            D, 0.0, 0, out.data_ptr(), lse.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0
        assert getattr(lib, f"mvdetr_attention_forward_host_{sfx}")(*(t.data_ptr() for t in host[:3]), _strides(*host[:3], out_h), B, H, Sq, Sk, D, 0.0,
                                                                   0, out_h.data_ptr(), lse_h.data_ptr()) == 0
        if entry == "forward":
            assert lib.mvdetr_attention_last_kernel().decode() == name
            if dtype == torch.float32:
                _within(f"{name} {kw}", out, out_h, ao.fp32_bar(q, k, v))
            continue
        grads = [torch.empty_like(t) for t in (qd, kd, vd)]
        grads_h = [torch.empty_like(t) for t in host[:3]]
        work = torch.empty(max(lib.mvdetr_attention_workspace_bytes(B, H, Sq, Sk, D, elem), 1), dtype=torch.uint8, device=DEV)
        rc = getattr(lib, f"mvdetr_attention_backward_{sfx}")(stream, gd.data_ptr(), qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(),
                                                             lse.data_ptr(), _strides(qd, kd, vd, out, gd, *grads), B, H, Sq, Sk, D, 0.0, 0,
                                                             work.data_ptr(), *(t.data_ptr() for t in grads))
        torch.cuda.synchronize()
        assert rc == 0 and lib.mvdetr_attention_last_kernel().decode() == name
        assert getattr(lib, f"mvdetr_attention_backward_host_{sfx}")(host[3].data_ptr(), *(t.data_ptr() for t in host[:3]), out_h.data_ptr(),
                                                                    lse_h.data_ptr(), _strides(*host[:3], out_h, host[3], *grads_h), B, H, Sq, Sk, D,
                                                                    0.0, 0, *(t.data_ptr() for t in grads_h)) == 0
        if dtype == torch.float32:
            for key, got, want, bar in zip("qkv", grads, grads_h, ao.grad_bars_elementwise(q, k, v, gout)):
                _within(f"{name} {kw} grad_{key}", got, want, bar)
