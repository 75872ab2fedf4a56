"""fp64 restatement of multi-head attention for the tests (plain torch, no library code; lives beside
deform_conv_oracle.py because oracle/ is frozen):

    out[b, h, i, :] = sum_j P[b, h, i, j] * v[b, h, j, :],   P = softmax_j(q k^T / sqrt(D)) [* keep / (1 - p)]

and the fp32 error model the tests' bars come from.  Everything is evaluated per (batch, head) slice so that a
2,700 x 2,700 problem never holds more than a few score matrices.

fp32 error model (``fp32_bar``), per output element, in units of EPS32 = 2^-24, from |.|-operand quantities only:
  * a score s_ij = scale * sum_d q_id k_jd computed as a length-D chain errs by at most (D + 4) * A_ij,
    A_ij = scale * sum_d |q_id| |k_jd| (D products and adds, the scaling, the conversion to the exp2 argument); the
    subtraction of the running maximum and the exponential act at magnitude |s - m| <= 2 max_j A_ij: 4 * max_j A_ij more.
    delta_ij = (D + 4) * A_ij + 4 * max_j A_ij  is an ABSOLUTE error of the score and therefore a RELATIVE error of
    exp(s_ij); after the normalisation p_ij is off by at most p_ij * (delta_ij + sum_k p_ik delta_ik);
  * the sum over the Sk keys (of the row sum and of p v) is a chain of Sk roundings of independent sign: a random walk,
    (sqrt(Sk) + 4) each relative to sum_j p_ij |v_jd| (the worst case Sk is never approached at Sk in the thousands and
    would hide a lost key at Sk = 2,700, which the self-test of the bar forbids);
  bar_id = MARGIN * EPS32 * (sum_j p_ij |v_jd| (delta_ij + dbar_i) + 2 (sqrt(Sk) + 4) sum_j p_ij |v_jd|),
  dbar_i = sum_j p_ij delta_ij.  MARGIN is the smallest whole number with which torch's own fp32 composition on the CPU
  passes at every size and seed the tests use (DESIGN.md section 4.8 records it and every route's observed err / bar).
Gradient bars (``grad_bars``) are one number per tensor in the style of tests/test_deform_conv_gpu.py::_grad_check: the
same chain lengths times the largest element of the gradient's |.|-operand restatement.
"""
import math

import torch

EPS32 = 2.0 ** -24
MARGIN = 1


def _slices(q, k, v, keep):
    B, H = q.shape[:2]
    for b in range(B):
        for h in range(H):
            yield b, h, q[b, h].double(), k[b, h].double(), v[b, h].double(), None if keep is None else keep[b, h].double()


def attention(q, k, v, keep=None, p=0.0, drop_last_key=False):
    """[B, H, Sq, D] fp64.  ``keep``: bool [B, H, Sq, Sk] dropout keep mask (kept probabilities scaled by 1 / (1 - p));
    ``drop_last_key``: leave the last key out (the wrong answer the bar's self-test must detect)."""
    out = torch.empty(q.shape, dtype=torch.float64)
    for b, h, qs, ks, vs, ms in _slices(q, k, v, keep):
        if drop_last_key:
            ks, vs = ks[:-1], vs[:-1]
        P = torch.softmax(qs @ ks.t() / math.sqrt(q.shape[-1]), -1)
        if ms is not None:
            P = P * ms / (1.0 - p)
        out[b, h] = P @ vs
    return out


def with_grads(q, k, v, gout, keep=None, p=0.0):
    """(out, grad_q, grad_k, grad_v) in fp64 by autograd, one (batch, head) slice at a time."""
    res = [torch.empty(x.shape, dtype=torch.float64) for x in (q, q, k, v)]
    for b, h, qs, ks, vs, ms in _slices(q, k, v, keep):
        leaves = [x.requires_grad_(True) for x in (qs, ks, vs)]
        P = torch.softmax(leaves[0] @ leaves[1].t() / math.sqrt(q.shape[-1]), -1)
        if ms is not None:
            P = P * ms / (1.0 - p)
        out = P @ leaves[2]
        grads = torch.autograd.grad(out, leaves, gout[b, h].double())
        for dst, src in zip(res, (out.detach(),) + tuple(grads)):
            dst[b, h] = src
    return tuple(res)


def fp32_bar(q, k, v, margin=None):
    """Per-element bound [B, H, Sq, D] of |fp32 result - exact| (module docstring)."""
    D, Sk = q.shape[-1], k.shape[2]
    scale = 1.0 / math.sqrt(D)
    bar = torch.empty(q.shape, dtype=torch.float64)
    for b, h, qs, ks, vs, _ in _slices(q, k, v, None):
        P = torch.softmax(qs @ ks.t() * scale, -1)
        A = scale * (qs.abs() @ ks.abs().t())
        delta = (D + 4) * A + 4 * A.max(-1, keepdim=True)[0]
        pv = P @ vs.abs()
        bar[b, h] = (P * delta) @ vs.abs() + (P * delta).sum(-1, keepdim=True) * pv + 2 * (math.sqrt(Sk) + 4) * pv
    return (MARGIN if margin is None else margin) * EPS32 * bar


def grad_bars(q, k, v, gout, margin=None):
    """(bar_q, bar_k, bar_v): one bound per gradient tensor.  With W_ij = p_ij (sum_d |gout_id| |v_jd| + sum_k p_ik sum_d
    |gout_id| |v_kd|) >= |dS_ij|:  |dq_id| <= scale sum_j W_ij |k_jd|, |dk_jd| <= scale sum_i W_ij |q_id|, |dv_jd| <= sum_i p_ij
    |gout_id|; the chains are the score's (delta, relative, at its largest), the D-term dot products (2 D + 8) and the random
    walk over the tokens summed (2 sqrt(S) + 8)."""
    D, Sq, Sk = q.shape[-1], q.shape[2], k.shape[2]
    scale = 1.0 / math.sqrt(D)
    mq = mk = mv = dmax = 0.0
    for b, h, qs, ks, vs, _ in _slices(q, k, v, None):
        g = gout[b, h].double().abs()
        P = torch.softmax(qs @ ks.t() * scale, -1)
        A = scale * (qs.abs() @ ks.abs().t())
        dmax = max(dmax, float(((D + 4) * A + 4 * A.max(-1, keepdim=True)[0]).max()))
        dP = g @ vs.abs().t()
        W = P * (dP + (P * dP).sum(-1, keepdim=True))
        mq = max(mq, float((scale * (W @ ks.abs())).max()))
        mk = max(mk, float((scale * (W.t() @ qs.abs())).max()))
        mv = max(mv, float((P.t() @ g).max()))
    chain = 2 * dmax + 2 * D + 8 + 2 * math.sqrt(max(Sq, Sk)) + 8
    m = (MARGIN if margin is None else margin) * EPS32 * chain
    return m * mq, m * mk, m * mv
