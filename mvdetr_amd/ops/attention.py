"""attention / MultiheadAttention: nn.MultiheadAttention's softmax(q k^T / sqrt(D)) v on the library's fused kernels.

The reference's ``trans`` ground-plane aggregator (multiview_detector/models/transformer.py:40,59) attends over the
whole ground grid with ``nn.MultiheadAttention``, whose fp32 path materialises the [B * H, S, S] scores (233 MB per layer
at Wildtrack size) for the softmax, the second matmul and the backward.  ``attention`` computes the same result without
ever writing a score: CUDA tensors run the HIP kernels of csrc/attention.hip (fp32 with head dimension 16 or 32 the MFMA
kernels, everything else the generic ones), CPU tensors the library's host path.  The backward recomputes the
probabilities from the saved log-sum-exp, uses no atomics and is bit-reproducible run to run.

16-bit inference: CUDA float16 / bfloat16 q, k, v with ``dropout_p == 0`` and nothing to differentiate run
``attn_fwd_mfma_half`` (csrc/attention_half.hip: 16-bit MFMA, fp32 softmax, the probabilities as two 16-bit terms, one
rounding on the way out) where the library's route (csrc/attention_route.h) takes the call; every other such call is
``attention(q.float(), k.float(), v.float()).to(dtype)`` on the fp32 kernels.  A 16-bit call that needs gradients or dropout is
refused, and there is no 16-bit host path.

* ``attention(q, k, v, dropout_p=0.0, seed=None)``: q [B, H, Sq, D], k and v [B, H, Sk, D] -> [B, H, Sq, D].  The operands
  may be any views whose last dimension is contiguous (a head-split view of a seq-first or batch-first projection is read in
  place).  Dropout acts on the probabilities as in torch, by a counter-based hash of (seed, element index)
  (include/mvdetr_ops.h); ``seed`` defaults to a draw from torch's CPU generator, so ``torch.manual_seed`` reproduces a run.
* ``MultiheadAttention``: ``nn.MultiheadAttention`` (same parameters, state dict and signature).  ``need_weights=False``
  without masks runs in-projection GEMM(s) -> ``attention`` -> out-projection; any other call is torch's implementation.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib

MAX_HEAD_DIM = 256


def last_kernel() -> str:
    """Route of the last attention call of this process on the device: "attn_fwd_mfma", "attn_fwd_generic",
    "attn_bwd_mfma", "attn_bwd_generic" or "attn_fwd_mfma_half" (tests / tools introspection)."""
    return _lib.lib().mvdetr_attention_last_kernel().decode()


def set_half_query_tile(queries: int) -> int:
    """Queries per workgroup of the 16-bit kernel: 64, 128 or 0 (by the shape, the default); returns the previous value.  The
    results do not depend on it (tests / tools)."""
    prev = _lib.lib().mvdetr_attn_half_set_query_tile(int(queries))
    if prev < 0:
        raise ValueError(f"set_half_query_tile: 0, 64 or 128, got {queries}")
    return prev


def dropout_keep_mask(seed: int, p: float, B: int, H: int, Sq: int, Sk: int) -> torch.Tensor:
    """The keep decisions (bool [B, H, Sq, Sk], CPU) that ``attention(..., dropout_p=p, seed=seed)`` makes on every path."""
    mask = torch.empty((B, H, Sq, Sk), dtype=torch.uint8)
    _lib.check(_lib.lib().mvdetr_attention_dropout_mask_host(seed & (2 ** 64 - 1), float(p), B, H, Sq, Sk, mask.data_ptr()),
               "attention_dropout_mask")
    return mask.bool()


def draw_seed() -> int:
    """A 64-bit seed from torch's CPU generator (no device sync)."""
    return int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64).item()) & (2 ** 64 - 1)


def _rows(t):
    """The tensor the kernels read: `t` itself when its channels are contiguous, else a dense copy."""
    return t if t.stride(-1) == 1 or t.shape[-1] == 1 else t.contiguous()


def _empty_like_order(t):
    """An uninitialised dense tensor of t's shape whose dimensions lie in memory in t's order (t may be a strided view)."""
    order = sorted(range(t.dim() - 1), key=lambda d: (-t.stride(d), d)) + [t.dim() - 1]
    inv = [order.index(d) for d in range(t.dim())]
    return torch.empty([t.shape[d] for d in order], dtype=t.dtype, device=t.device).permute(inv)


def _strides(*tensors):
    flat = [s for t in tensors for s in t.stride()[:3]]
    return (ctypes.c_int64 * len(flat))(*flat)


class AttentionFunction(Function):
    @staticmethod
    def forward(ctx, q, k, v, dropout_p, seed):
        q, k, v = _rows(q), _rows(k), _rows(v)
        B, H, Sq, D = q.shape
        Sk = k.shape[2]
        out = _empty_like_order(q)
        lse = torch.empty((B, H, Sq), dtype=q.dtype, device=q.device)
        sfx = _lib.suffix(q.dtype)
        args = [q.data_ptr(), k.data_ptr(), v.data_ptr(), _strides(q, k, v, out), B, H, Sq, Sk, D, dropout_p, seed,
                out.data_ptr(), lse.data_ptr()]
        if q.is_cuda:
            with torch.cuda.device(q.device):
                rc = getattr(_lib.lib(), f"mvdetr_attention_forward_{sfx}")(_lib.current_stream_ptr(q.device), *args)
        else:
            rc = getattr(_lib.lib(), f"mvdetr_attention_forward_host_{sfx}")(*args)
        _lib.check(rc, "attention_forward")
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.dropout_p, ctx.seed = dropout_p, seed
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        q, k, v, out, lse = ctx.saved_tensors
        B, H, Sq, D = q.shape
        Sk = k.shape[2]
        grad_out = _rows(grad_out)
        gq, gk, gv = _empty_like_order(q), _empty_like_order(k), _empty_like_order(v)
        if B * H * Sq == 0:
            return gq, gk.zero_(), gv.zero_(), None, None
        sfx = _lib.suffix(q.dtype)
        head = [grad_out.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(),
                _strides(q, k, v, out, grad_out, gq, gk, gv), B, H, Sq, Sk, D, ctx.dropout_p, ctx.seed]
        tail = [gq.data_ptr(), gk.data_ptr(), gv.data_ptr()]
        if q.is_cuda:
            nbytes = _lib.lib().mvdetr_attention_workspace_bytes(B, H, Sq, Sk, D, q.element_size())
            work = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=q.device)
            with torch.cuda.device(q.device):
                rc = getattr(_lib.lib(), f"mvdetr_attention_backward_{sfx}")(
                    _lib.current_stream_ptr(q.device), *head, work.data_ptr(), *tail)
        else:
            rc = getattr(_lib.lib(), f"mvdetr_attention_backward_host_{sfx}")(*head, *tail)
        _lib.check(rc, "attention_backward")
        return gq, gk, gv, None, None


HALF_DTYPES = (torch.float16, torch.bfloat16)


def _half_rows_ok(t) -> bool:
    """Can attn_fwd_mfma_half read this view in place?  Every row 16-byte aligned: base and strides (in elements, % 8)."""
    return t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(s % 8 == 0 for s in t.stride()[:3])


def _attention_half(q, k, v):
    """The 16-bit forward (inference only; the caller has checked dtype, device, dropout and grad)."""
    B, H, Sq, D = q.shape
    if all(_half_rows_ok(t) for t in (q, k, v)):                # (about the tensors; everything else is the route's)
        ok = int(_half_rows_ok(out := _empty_like_order(q)))
        if _lib.attn_route(_lib.ROUTE_FORWARD_HALF, 2, B, H, Sq, k.shape[2], D, 0.0, ok, ok) == "fwd_mfma_half":
            with torch.cuda.device(q.device):
                rc = getattr(_lib.lib(), f"mvdetr_attn_forward_{_lib.suffix(q.dtype, half_ok=True)}")(
                    _lib.current_stream_ptr(q.device), q.data_ptr(), k.data_ptr(), v.data_ptr(), _strides(q, k, v, out),
                    B, H, Sq, k.shape[2], D, out.data_ptr())
            _lib.check(rc, "attention_forward_half")
            return out
    return attention(q.float(), k.float(), v.float()).to(q.dtype)       # what the 16-bit kernel does not take


def attention(q, k, v, dropout_p=0.0, seed=None):
    """softmax(q k^T / sqrt(D)) v per (batch, head): q [B, H, Sq, D], k and v [B, H, Sk, D] -> [B, H, Sq, D] (laid out in
    memory like q).  ``dropout_p`` in [0, 1) drops probabilities (kept ones scaled by 1 / (1 - p)); ``seed``: 64-bit
    integer of the keep hash, drawn from torch's CPU generator when None."""
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError(f"attention: expected 4-D q, k and v [B, H, S, D], got {tuple(q.shape)}, {tuple(k.shape)} and "
                         f"{tuple(v.shape)}")
    devices = {t.device for t in (q, k, v)}
    if len(devices) != 1:
        raise RuntimeError(f"attention: all tensors must be on one device, got {sorted(map(str, devices))}")
    dtypes = {t.dtype for t in (q, k, v)}
    if len(dtypes) != 1:
        raise RuntimeError(f"attention: all tensors must have one dtype, got {sorted(map(str, dtypes))}")
    half = q.dtype in HALF_DTYPES and q.is_cuda
    _lib.suffix(q.dtype, half_ok=half)                             # 16-bit CPU tensors raise here
    B, H, Sq, D = q.shape
    if k.shape != v.shape or k.shape[0] != B or k.shape[1] != H or k.shape[3] != D:
        raise ValueError(f"attention: k {tuple(k.shape)} and v {tuple(v.shape)} must both be [B, H, Sk, D] for q "
                         f"{tuple(q.shape)}")
    if k.shape[2] < 1:
        raise ValueError("attention: at least one key is needed")
    if not 1 <= D <= MAX_HEAD_DIM:
        raise ValueError(f"attention: head dimension {D} is outside 1..{MAX_HEAD_DIM}")
    dropout_p = float(dropout_p)
    if not 0.0 <= dropout_p < 1.0:
        raise ValueError(f"attention: dropout_p must be in [0, 1), got {dropout_p}")
    if half:
        if dropout_p != 0.0:
            raise ValueError(f"attention: the {q.dtype} kernel is inference-only and has no dropout (dropout_p = {dropout_p})")
        if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
            raise RuntimeError(f"attention: the {q.dtype} kernel is forward-only (inference); run it under torch.no_grad() "
                               f"or on tensors that do not require grad")
        return _attention_half(q, k, v)
    if dropout_p == 0.0:
        seed = 0
    elif seed is None:
        seed = draw_seed()
    return AttentionFunction.apply(q, k, v, dropout_p, int(seed) & (2 ** 64 - 1))


class MultiheadAttention(nn.MultiheadAttention):
    """``nn.MultiheadAttention`` with the fused kernels under it: same constructor, parameters (``in_proj_weight`` [3E, E],
    ``in_proj_bias``, ``out_proj.weight``, ``out_proj.bias``), initial values and state dict.  ``forward`` keeps torch's
    signature and return pair.  With ``need_weights=False``, no masks, ``bias=True``, equal embedding sizes, 3-D fp32 / fp64
    inputs it returns ``(out, None)`` from in-projection GEMM(s) (one for q and k when ``query is key``) -> ``attention`` ->
    out-projection, the heads read from the projections in place.  Every other call (weights requested, masks, kdim / vdim,
    add_bias_kv, add_zero_attn, unbatched inputs, is_causal) is torch's own implementation, unchanged.  16-bit (float16 /
    bfloat16) CUDA inputs take the same route in eval mode when nothing needs a gradient (``attention`` is forward-only in
    16 bits); a training-mode or differentiated 16-bit call is torch's implementation."""

    def _dtype_ok(self, query, key, value):
        if query.dtype in (torch.float32, torch.float64):
            return True
        if query.dtype not in HALF_DTYPES or not query.is_cuda or self.training:
            return False
        return not (torch.is_grad_enabled() and (any(t.requires_grad for t in (query, key, value))
                                                 or any(p.requires_grad for p in self.parameters())))

    def _fused_ok(self, query, key, value, key_padding_mask, need_weights, attn_mask, kw):
        return (not need_weights and key_padding_mask is None and attn_mask is None and not kw.get("is_causal", False)
                and self._qkv_same_embed_dim and self.in_proj_bias is not None and self.bias_k is None
                and self.bias_v is None and not self.add_zero_attn and query.dim() == 3 and key.dim() == 3
                and value.dim() == 3 and key.shape == value.shape
                and self._dtype_ok(query, key, value) and query.dtype == key.dtype == value.dtype
                and query.dtype == self.in_proj_weight.dtype and query.device == key.device == value.device
                and self.head_dim <= MAX_HEAD_DIM and key.shape[0 if not self.batch_first else 1] > 0
                and not torch.is_autocast_enabled())

    def forward(self, query, key, value, key_padding_mask=None, need_weights=True, attn_mask=None, **kw):
        if not self._fused_ok(query, key, value, key_padding_mask, need_weights, attn_mask, kw):
            return super().forward(query, key, value, key_padding_mask=key_padding_mask, need_weights=need_weights,
                                   attn_mask=attn_mask, **kw)
        E, H, D = self.embed_dim, self.num_heads, self.head_dim
        w, b = self.in_proj_weight, self.in_proj_bias
        if query is key and key is value:
            qp, kp, vp = F.linear(query, w, b).split(E, dim=-1)
        elif query is key:
            qp, kp = F.linear(query, w[:2 * E], b[:2 * E]).split(E, dim=-1)
            vp = F.linear(value, w[2 * E:], b[2 * E:])
        else:
            qp = F.linear(query, w[:E], b[:E])
            kp = F.linear(key, w[E:2 * E], b[E:2 * E])
            vp = F.linear(value, w[2 * E:], b[2 * E:])
        perm = (0, 2, 1, 3) if self.batch_first else (1, 2, 0, 3)          # -> [B, H, S, D] views, no copy
        q, k, v = (t.unflatten(-1, (H, D)).permute(perm) for t in (qp, kp, vp))
        o = attention(q, k, v, dropout_p=self.dropout if self.training else 0.0)
        back = (0, 2, 1, 3) if self.batch_first else (2, 0, 1, 3)
        o = o.permute(back).reshape(*query.shape[:2], E)                    # o lies in memory like q: a view
        return F.linear(o, self.out_proj.weight, self.out_proj.bias), None
