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

Per-element gradient bars (``grad_bars_elementwise``), in units of EPS32, per (batch, head) slice.  With g = grad_out,
  dP_ij = g_i . v_j [* keep_ij / (1 - p)],  delta_i = sum_j p_ij dP_ij = g_i . out_i,  dS_ij = p_ij (dP_ij - delta_i),
  dq_id = scale sum_j dS_ij k_jd,  dk_jd = scale sum_i dS_ij q_id,  dv_jd = sum_i p_ij [keep_ij / (1 - p)] g_id
every chain of n roundings of independent sign is a random walk, (sqrt(n) + 4) relative to the sum of the |terms| (the
worst case n is ~ 100 x what torch's fp32 composition shows for the D-term chains and hides a dropped grad_out element):
  * the score: rdelta_ij = (sqrt(D) + 4) A_ij, an absolute error of s_ij, so a relative one of exp(s_ij);
    dbar_i = sum_j p_ij rdelta_ij is what the normalisation adds;
  * the backward recomputes p_ij = exp(s_ij - lse_i) from two numbers of magnitude <= max_j A_ij + ln Sk (the stored lse,
    the products with log2 e, the difference): 4 (max_j A_ij + ln Sk); the stored lse carries the row sum's walk over the
    keys and the logarithm: sqrt(Sk) + 6.  Together
        rp_ij = rdelta_ij + dbar_i + 4 (max_j A_ij + ln Sk) + sqrt(Sk) + 6          (relative error of p_ij),
        dp_ij = p_ij rp_ij + TINY32 / EPS32                                          (absolute error of p_ij):
    below TINY32 = 2^-126 fp32 has no relative precision left (a probability there is a denormal or flushed to 0), which
    is all that remains of a key that no query attends to when the logits are large;
  * G_ij = sum_d |g_id| |v_jd| [* keep_ij / (1 - p)] >= |dP_ij|, a D-term chain: (sqrt(D) + 4) G_ij;  Gbar_i = sum_j p_ij G_ij
    >= |delta_i|, computed as g_i . out_i from the forward's out, whose probabilities are normalised by the sum of the
    very numbers they are (relative error delta_ij - sum_k p_ik delta_ik, at most rdelta_ij + dbar_i - 2 p_ij rdelta_ij:
    a one-hot row has none) and summed over the keys as in ``fp32_bar``:
        ddelta_i = sum_j p_ij G_ij (rdelta_ij + dbar_i - 2 p_ij rdelta_ij + sqrt(D) + 4) + 2 (sqrt(Sk) + 4) Gbar_i;
    (the backward's recomputed p_ij has no such cancellation: its score is a second evaluation, not the forward's;)
  * dS_ij = p_ij X_ij with X_ij = dP_ij - delta_i: to first order |error| <= dp_ij |X_ij| + p_ij |error of X_ij|, |X_ij| the
    exact value (the one quantity here that is no |.|-operand restatement: with G_ij + Gbar_i in its place the bar of a
    nearly one-hot row, where X vanishes, is ~ 1e3 x the row's whole gradient at logits of magnitude 80 and a zeroed
    grad_out row passes), and the error of X the two chains' (at Sk = 1, where X is pure cancellation, all there is):
        E_ij = (dp_ij + 2 p_ij) |X_ij| + p_ij ((sqrt(D) + 4) G_ij + ddelta_i)           (absolute error of dS_ij),
        W_ij = p_ij |X_ij| = |dS_ij|                                                   (what the sums over tokens walk on);
  bar_q_id = MARGIN * EPS32 * scale * (sum_j E_ij |k_jd| + (sqrt(Sk) + 6) sum_j W_ij |k_jd|)
  bar_k_jd = MARGIN * EPS32 * scale * (sum_i E_ij |q_id| + (sqrt(Sq) + 6) sum_i W_ij |q_id|)
  bar_v_jd = MARGIN * EPS32 * sum_i (dp_ij [* keep_ij / (1 - p)] + (sqrt(Sq) + 7) pk_ij) |g_id|,  pk = p [* keep / (1 - p)]
each capped by the per-tensor bar of ``grad_bars`` (times 1 / (1 - p) under dropout, as the tests scale it).  Errors common
to a row (lse, delta) are added at full size; only the roundings inside one chain walk.  An element whose |.| terms all
vanish (a zero grad_out row, a key every query dropped) has a zero bar: its gradient is exactly 0 and must be returned so.
"""
import math

import torch

EPS32 = 2.0 ** -24
TINY32 = 2.0 ** -126                # the smallest normal fp32 number
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


def grads_explicit(q, k, v, gout, keep=None, p=0.0, keep_bwd="same", omit_delta=False):
    """(grad_q, grad_k, grad_v) in fp64 from the formulas of the module docstring (no autograd), so that a wrong backward
    can be written down: ``keep_bwd`` is the mask the backward applies ("same": the forward's ``keep``; None: none, the
    forward's dropout forgotten), ``omit_delta`` leaves delta out of dS.  delta is always g . out of the true forward."""
    scale = 1.0 / math.sqrt(q.shape[-1])
    if isinstance(keep_bwd, str):
        keep_bwd = keep
    res = [torch.empty(x.shape, dtype=torch.float64) for x in (q, k, v)]
    for b, h, qs, ks, vs, ms in _slices(q, k, v, keep):
        g = gout[b, h].double()
        P = torch.softmax(qs @ ks.t() * scale, -1)
        out = (P if ms is None else P * ms / (1.0 - p)) @ vs
        mb = None if keep_bwd is None else keep_bwd[b, h].double() / (1.0 - p)
        dP = g @ vs.t() if mb is None else (g @ vs.t()) * mb
        dS = P * dP if omit_delta else P * (dP - (g * out).sum(-1, keepdim=True))
        res[0][b, h] = scale * (dS @ ks)
        res[1][b, h] = scale * (dS.t() @ qs)
        res[2][b, h] = (P if mb is None else P * mb).t() @ g
    return tuple(res)


def grad_bars_elementwise(q, k, v, gout, keep=None, p=0.0, margin=None):
    """(bar_q, bar_k, bar_v): fp64 bounds shaped like the gradients of |fp32 gradient - exact| (module docstring)."""
    D, Sq, Sk = q.shape[-1], q.shape[2], k.shape[2]
    scale = 1.0 / math.sqrt(D)
    cd, cq, ck = math.sqrt(D) + 4, math.sqrt(Sq) + 6, math.sqrt(Sk) + 6
    bars = [torch.empty(x.shape, dtype=torch.float64) for x in (q, k, v)]
    for b, h, qs, ks, vs, ms in _slices(q, k, v, keep):
        g = gout[b, h].double().abs()
        P = torch.softmax(qs @ ks.t() * scale, -1)
        A = scale * (qs.abs() @ ks.abs().t())
        rdelta = cd * A
        dbar = (P * rdelta).sum(-1, keepdim=True)
        rp = rdelta + dbar + 4 * (A.max(-1, keepdim=True)[0] + math.log(Sk)) + ck
        G, Pk = g @ vs.abs().t(), P
        if ms is not None:
            G, Pk = G * ms / (1.0 - p), P * ms / (1.0 - p)
        Gbar = (P * G).sum(-1, keepdim=True)
        dP = gout[b, h].double() @ vs.t()
        if ms is not None:
            dP = dP * ms / (1.0 - p)
        X = (dP - (P * dP).sum(-1, keepdim=True)).abs()                # |dP_ij - delta_i|, exact
        ddelta = (P * G * (rdelta + dbar - 2 * P * rdelta + cd)).sum(-1, keepdim=True) + 2 * (math.sqrt(Sk) + 4) * Gbar
        dp = P * rp + TINY32 / EPS32                                   # absolute error of p_ij
        E = (dp + 2 * P) * X + P * (cd * G + ddelta)
        W = P * X
        bars[0][b, h] = scale * (E @ ks.abs() + ck * (W @ ks.abs()))
        bars[1][b, h] = scale * (E.t() @ qs.abs() + cq * (W.t() @ qs.abs()))
        bars[2][b, h] = ((dp if ms is None else dp * ms / (1.0 - p)) + (cq + 1) * Pk).t() @ g
    m = (MARGIN if margin is None else margin) * EPS32
    caps = grad_bars(q, k, v, gout, margin)
    return tuple(torch.clamp(m * bar, max=cap / (1.0 - p)) for bar, cap in zip(bars, caps))
