"""Input builders shared by the GPU parity tests and the bench (synthetic, seeded)."""
import math

import torch


def level_start_index(shapes):
    return torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))


def random_msda_inputs(B, shapes_hw, M, D, Lq, P, seed=0, dtype=torch.float32, lo=-0.2, hi=1.2,
                       value_scale=1.0):
    """value ~ N(0,1)*scale, locations ~ U[lo, hi] (a good part outside [0,1]), weights normalised
    over L*P like ops/test.py:33-36."""
    g = torch.Generator().manual_seed(seed)
    shapes = torch.as_tensor(shapes_hw, dtype=torch.long)
    L = shapes.shape[0]
    S = int(shapes.prod(1).sum())
    value = (torch.randn(B, S, M, D, generator=g) * value_scale).to(dtype)
    loc = (torch.rand(B, Lq, M, L, P, 2, generator=g) * (hi - lo) + lo).to(dtype)
    aw = torch.rand(B, Lq, M, L, P, generator=g) + 1e-5
    aw = (aw / aw.sum((-1, -2), keepdim=True)).to(dtype)
    return value, shapes, level_start_index(shapes), loc, aw


def encoder_msda_inputs(L, H, W, M=8, D=16, P=4, B=1, seed=0, noise_px=1.0, dtype=torch.float32):
    """Locality-realistic inputs of MVDeTr's shadow transformer: L equal H x W levels,
    Lq = S, reference = identity pixel-centre grid for every level, offsets = the module's initial
    bias grid (ms_deform_attn.py:64-69) + N(0, noise_px) pixels, weights = softmax(N(0,1))."""
    g = torch.Generator().manual_seed(seed)
    shapes = torch.as_tensor([(H, W)] * L, dtype=torch.long)
    S = L * H * W
    value = torch.randn(B, S, M, D, generator=g).to(dtype)
    ys, xs = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
    ref = torch.stack([xs / W, ys / H], -1).reshape(-1, 2).repeat(L, 1)            # [S,2]
    ang = torch.arange(M, dtype=torch.float32) * (2.0 * math.pi / M)
    dirs = torch.stack([ang.cos(), ang.sin()], -1)
    dirs = dirs / dirs.abs().max(-1, keepdim=True)[0]
    bias = dirs.view(M, 1, 1, 2) * torch.arange(1, P + 1).view(1, 1, P, 1)         # [M,1,P,2]
    off = bias[None, None] + noise_px * torch.randn(B, S, M, L, P, 2, generator=g)
    loc = ref[None, :, None, None, None, :] + off / torch.tensor([W, H], dtype=torch.float32)
    aw = torch.softmax(torch.randn(B, S, M, L * P, generator=g), -1).view(B, S, M, L, P)
    return value, shapes, level_start_index(shapes), loc.to(dtype).contiguous(), aw.to(dtype)


def fused_train_inputs(L, H, W, M=8, D=16, P=4, B=1, seed=0, noise_px=1.0, level_logit_offsets=None):
    """The same realistic encoder input in the fused TRAINING pair's form (include/mvdetr_ops.h): -> value, shapes, lsi,
    reference points [1, L, Lq, 2] (one per (query, level): the query's own cell centre), raw [B, Lq, M*L*P*3] = the
    module's single GEMM output in the slice-interleaved, level-outermost layout (offsets in pixels = bias grid +
    N(0, noise_px); logits N(0, 1)), and the row permutation that produced it (slice_major_rows(level_outer=True)).
    level_logit_offsets: added to the logits of level l of head m as offs[(l + m) % len(offs)] (the pattern rolled by head,
    so that every head sees another level order; per-level, because a per-head offset cancels in the per-head softmax)."""
    g = torch.Generator().manual_seed(seed)
    shapes = torch.as_tensor([(H, W)] * L, dtype=torch.long)
    S = L * H * W
    value = torch.randn(B, S, M, D, generator=g)
    ys, xs = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
    cells = torch.stack([xs / W, ys / H], -1).reshape(-1, 2).repeat(L, 1)           # [S, 2]
    ref_lm = cells[None, None].expand(1, L, S, 2).contiguous()
    ang = torch.arange(M, dtype=torch.float32) * (2.0 * math.pi / M)
    dirs = torch.stack([ang.cos(), ang.sin()], -1)
    dirs = dirs / dirs.abs().max(-1, keepdim=True)[0]
    bias = dirs.view(M, 1, 1, 2) * torch.arange(1, P + 1).view(1, 1, P, 1)          # [M, 1, P, 2]
    off = bias[None, None] + noise_px * torch.randn(B, S, M, L, P, 2, generator=g)  # reference order (m, l, p, xy)
    logit = torch.randn(B, S, M, L, P, generator=g)
    if level_logit_offsets is not None:
        offs = torch.as_tensor(level_logit_offsets, dtype=torch.float32)
        idx = (torch.arange(L).view(1, L) + torch.arange(M).view(M, 1)) % offs.numel()
        logit = logit + offs[idx].view(1, 1, M, L, 1)
    hps, n_off = 32 // D, M * L * P * 2
    rows = []
    for l in range(L):                                                              # runs: (level, slice) -> hps heads' offsets, then logits
        for s_ in range(M // hps):
            for h in range(hps):
                rows += [(((s_ * hps + h) * L + l) * P + p) * 2 + xy for p in range(P) for xy in range(2)]
            for h in range(hps):
                rows += [n_off + ((s_ * hps + h) * L + l) * P + p for p in range(P)]
    rows = torch.tensor(rows)
    plain = torch.cat([off.reshape(B, S, -1), logit.reshape(B, S, -1)], -1)
    return value, shapes, level_start_index(shapes), ref_lm, plain.index_select(-1, rows).contiguous(), rows


def smooth_features(n, c, h, w, seed=0, dtype=torch.float32):
    """O(1) band-limited feature maps (a few low spatial frequencies per channel)."""
    g = torch.Generator().manual_seed(seed)
    ys = torch.linspace(0, 1, h).view(1, 1, h, 1)
    xs = torch.linspace(0, 1, w).view(1, 1, 1, w)
    out = torch.zeros(n, c, h, w)
    for _ in range(4):
        fy = torch.rand(n, c, 1, 1, generator=g) * 6
        fx = torch.rand(n, c, 1, 1, generator=g) * 6
        ph = torch.rand(n, c, 1, 1, generator=g) * 2 * math.pi
        out += torch.randn(n, c, 1, 1, generator=g) * torch.sin(2 * math.pi * (fy * ys + fx * xs) + ph)
    return out.to(dtype)


def pyramid_encoder_inputs(shapes_hw, M=8, D=32, P=4, B=1, seed=0, noise_px=1.5, dtype=torch.float32):
    """Deformable-DETR-style encoder inputs over levels of DIFFERENT sizes: Lq = S, each query's
    reference point is its own normalised cell centre in every level, offsets ~ N(0, noise_px) pixels
    of the sampled level."""
    g = torch.Generator().manual_seed(seed)
    shapes = torch.as_tensor(shapes_hw, dtype=torch.long)
    L = shapes.shape[0]
    S = int(shapes.prod(1).sum())
    value = torch.randn(B, S, M, D, generator=g).to(dtype)
    refs = []
    for H, W in shapes_hw:
        ys, xs = torch.meshgrid(torch.arange(H) + 0.5, torch.arange(W) + 0.5, indexing="ij")
        refs.append(torch.stack([xs / W, ys / H], -1).reshape(-1, 2))
    ref = torch.cat(refs, 0)                                                     # [S,2]
    wh = torch.tensor([[w, h] for h, w in shapes_hw], dtype=torch.float32)       # [L,2]
    off = noise_px * torch.randn(B, S, M, L, P, 2, generator=g) / wh[None, None, None, :, None, :]
    loc = ref[None, :, None, None, None, :] + off
    aw = torch.softmax(torch.randn(B, S, M, L * P, generator=g), -1).view(B, S, M, L, P)
    return value, shapes, level_start_index(shapes), loc.to(dtype).contiguous(), aw.to(dtype)


# ---- skewed attention-weight mass: block bars per (level, head) (test_msda_mass_skew_gpu.py, test_knob_routes_gpu.py) ----
# msda_bwd_onepass runs jobs (4 x 16-cell tile, head, level) in contiguous ranges per workgroup and GUESSES each job's
# fixed-point scale from the job before; its grid on MI355X is 256 CUs x at most 3 workgroups (launch_onepass_nc, rounded up
# to a multiple of 8).  A case exercises the guess only if every workgroup runs several jobs.
ONEPASS_TILE_H, ONEPASS_TILE_W = 4, 16
ONEPASS_MAX_GRID = 768
MIN_JOBS_PER_WORKGROUP = 8
# band_cliff compares the tokens this many columns or more from an inner band edge: a job whose tile holds queries of both bands
# quantises at the heavier band's step (the guarantee is relative to the job's own bound), and the widest job -- msda_bwd_value_tok's
# 32-column tile with its 6-column window radius -- plus the window shift and the tap reach stays inside 48
BAND_EDGE_MARGIN = 48

LEVEL_CLIFF = [0, 20, 0, 29, 10, 0, 24]           # 2^-k per level: falls and rises between neighbouring levels
HEAD_CLIFF = [0, 20, 0, 16, 4, 28, 0, 12]         # 2^-k per head
BAND_CLIFF_K = 22                                 # queries of every other band of columns
LOGIT_CLIFF = [0, -14, 0, -21, -7, 0, -17]        # fused pair: per-level logit offsets (rolled by head)


# scaled-down forms for the library's host path (test_block_bars.py: runs without a GPU)
HOST_SKEW_CASES = {
    "level_cliff_host": ("public", dict(L=7, H=9, W=20, M=8, D=16, B=1, seed=61), ("level", LEVEL_CLIFF)),
    "head_cliff_host": ("public", dict(L=7, H=9, W=20, M=8, D=16, B=1, seed=62), ("head", HEAD_CLIFF)),
}


def skew_spec(case):
    return SKEW_CASES[case] if case in SKEW_CASES else HOST_SKEW_CASES[case]


def onepass_jobs(B, L, H, W, M):
    return B * -(-H // ONEPASS_TILE_H) * -(-W // ONEPASS_TILE_W) * M * L


# name -> (form, builder arguments, skew)
SKEW_CASES = {
    "level_cliff_wildtrack": ("public", dict(L=7, H=60, W=180, M=8, D=16, B=1, seed=51), ("level", LEVEL_CLIFF)),
    "head_cliff_wildtrack": ("public", dict(L=7, H=60, W=180, M=8, D=16, B=1, seed=52), ("head", HEAD_CLIFF)),
    "band_cliff_wildtrack": ("public", dict(L=7, H=60, W=180, M=8, D=16, B=1, seed=53), ("band", 90)),
    "level_cliff_multiviewx": ("public", dict(L=6, H=80, W=125, M=8, D=16, B=2, seed=54), ("level", [0, 20, 0, 29, 10, 24])),
    "fused_level_cliff_wildtrack": ("fused", dict(L=7, H=60, W=180, M=8, D=16, B=1, seed=55), ("logit", LOGIT_CLIFF)),
    "fused_level_cliff_l12": ("fused", dict(L=12, H=36, W=128, M=8, D=16, B=1, seed=56), ("logit", LOGIT_CLIFF)),
    "fused_level_cliff_d32": ("fused", dict(L=6, H=40, W=90, M=8, D=32, B=1, seed=57), ("logit", LOGIT_CLIFF)),
}


def skew_msda_inputs(L, H, W, M, D, B, seed, skew):
    """encoder_msda_inputs with the attention weights of whole levels, heads or column bands of queries scaled by powers of two:
    skew = ("level", k[L]) | ("head", k[M]) | ("band", width) (queries in every other band of `width` columns, the first one
    included, scaled by 2^-BAND_CLIFF_K) | None.  -> value, shapes, lsi, loc, aw, grad_out."""
    value, shapes, lsi, loc, aw = encoder_msda_inputs(L, H, W, M=M, D=D, B=B, seed=seed, noise_px=1.0)
    kind = skew[0] if skew else None
    if kind == "level":
        aw = aw * torch.pow(2.0, -torch.tensor(skew[1], dtype=torch.float32)).view(1, 1, 1, L, 1)
    elif kind == "head":
        aw = aw * torch.pow(2.0, -torch.tensor(skew[1], dtype=torch.float32)).view(1, 1, M, 1, 1)
    elif kind == "band":
        light = (torch.arange(W) // skew[1]) % 2 == 0                                   # [W], query column
        f = torch.where(light, 2.0 ** -BAND_CLIFF_K, 1.0).repeat(L * H)                  # [Lq]
        aw = aw * f.view(1, -1, 1, 1, 1)
    go = torch.randn(B, loc.shape[1], M * D, generator=torch.Generator().manual_seed(seed + 1000))
    return value, shapes, lsi, loc, aw.contiguous(), go


def skew_case(name):
    """-> (form, tensors): public: value, shapes, lsi, loc, aw, grad_out; fused: value, shapes, lsi, ref, raw, rows, grad_out."""
    form, a, skew = skew_spec(name)
    if form == "public":
        return form, skew_msda_inputs(skew=skew, **a)
    value, shapes, lsi, ref, raw, rows = fused_train_inputs(a["L"], a["H"], a["W"], M=a["M"], D=a["D"], B=a["B"], seed=a["seed"],
                                                            level_logit_offsets=skew[1])
    go = torch.randn(a["B"], value.shape[1], a["M"] * a["D"], generator=torch.Generator().manual_seed(a["seed"] + 1000))
    return form, (value, shapes, lsi, ref, raw, rows, go)


def fused_plain(raw_like, rows, M, L, P=4):
    """A tensor in the fused pair's raw layout -> (offsets [B, Lq, M, L, P, 2], logits [B, Lq, M, L, P]) in the plain order."""
    inv = torch.empty_like(rows)
    inv[rows] = torch.arange(rows.numel())
    plain = raw_like.index_select(-1, inv)
    B, Lq = plain.shape[:2]
    n_off = M * L * P * 2
    return plain[..., :n_off].reshape(B, Lq, M, L, P, 2), plain[..., n_off:].reshape(B, Lq, M, L, P)


def fused_reference(value, shapes, lsi, ref, raw, rows, go, P=4):
    """fp64 chain on the CPU (test_fused_train_gpu._reference_grads): the C oracle's backward at (loc, aw), then the module
    arithmetic's backward by hand.  -> grad_value, grad of the offsets, grad of the logits, loc."""
    from oracle import c_oracle
    H, W = int(shapes[0, 0]), int(shapes[0, 1])
    M, L = value.shape[2], shapes.shape[0]
    off, logit = fused_plain(raw.double(), rows, M, L, P)
    wh = torch.tensor([W, H], dtype=torch.float64)
    ref_ql = ref[0].transpose(0, 1).double()                                        # [Lq, L, 2]
    loc = (ref_ql[None, :, None, :, None, :] + off / wh).contiguous()
    B, Lq = logit.shape[:2]
    aw = torch.softmax(logit.flatten(-2), -1).view(B, Lq, M, L, P).contiguous()
    gv, gl, ga = c_oracle.msda_backward(value.double(), shapes, lsi, loc, aw, go.double())
    g_logit = aw * (ga - (aw * ga).sum((-1, -2), keepdim=True))
    return gv, gl / wh, g_logit, loc


def texel_smooth(loc, shapes):
    """[..., L, P] bool: taps more than 1e-4 px from a texel centre (the bilinear blend's slope jumps there, so the sign of
    fp32 rounding decides grad_sampling_loc: such taps are left out, as in test_msda_gpu.py)."""
    wh = torch.stack([shapes[:, 1], shapes[:, 0]], -1).double()
    px = loc.double() * wh[None, None, None, :, None, :] - 0.5
    return (px - px.round()).abs().amin(-1) > 1e-4


def block_bar(got, ref, block_dims, rel, floor=0.0, mask=None):
    """The block bar: inside every block, max |got - ref| <= rel * max |ref| + floor.

    block_dims: ascending dims of got / ref that index the blocks; every other dim is reduced over.  mask (bool, broadcastable
    to ref): False entries are left out of both the error and the block's maximum.  NaN in got fails its block.
    -> dict: ratio (the worst block's err / (rel * max + floor): above 1 the bar fails), block (its index), err, ref_max (its
    error and reference maximum), blocks_min / blocks_max (the smallest / largest reference maximum over all blocks)."""
    ref = ref.double()
    d = (got.double() - ref).abs()
    r = ref.abs()
    if mask is not None:
        mask = mask.expand_as(ref)
        d = torch.where(mask, d, torch.zeros((), dtype=d.dtype))
        r = torch.where(mask, r, torch.zeros((), dtype=r.dtype))
    assert list(block_dims) == sorted(block_dims)
    red = tuple(i for i in range(ref.dim()) if i not in block_dims)
    err, rmax = d.amax(red), r.amax(red)
    ratio = err / (rel * rmax + floor)
    ratio = torch.where(torch.isnan(ratio), torch.full((), float("inf"), dtype=ratio.dtype), ratio)
    worst = int(ratio.flatten().argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), ratio.shape))
    return dict(ratio=ratio.flatten()[worst].item(), block=idx, err=err.flatten()[worst].item(), ref_max=rmax.flatten()[worst].item(),
                blocks_min=rmax.min().item(), blocks_max=rmax.max().item())


def _value_blocks(t, shapes, M, band):
    """grad_value [B, S, M, D] (equal levels) -> (view, block dims, mask): blocks [b, level, head] -- or [b, level, band, head]
    with only the tokens BAND_EDGE_MARGIN or more columns from an inner band edge."""
    L, H, W = shapes.shape[0], int(shapes[0, 0]), int(shapes[0, 1])
    B, D = t.shape[0], t.shape[-1]
    if not band:
        return t.view(B, L, H, W, M, D), (0, 1, 4), None
    nb = W // band
    assert nb * band == W and nb >= 2
    x = torch.arange(W)
    edges = torch.arange(1, nb) * band
    dist = torch.minimum((x[:, None] - edges[None]).abs(), (x[:, None] + 1 - edges[None]).abs()).amin(1)
    keep = (dist >= BAND_EDGE_MARGIN).view(1, 1, 1, nb, band, 1, 1)
    return t.view(B, L, H, nb, band, M, D), (0, 1, 3, 5), keep


def _query_blocks(t, shapes, band):
    """a sampling gradient [B, Lq, M, L, P, ...] -> (view, block dims): blocks [b, head, level] -- or [b, band, head, level] by
    the query's column (Lq = the L equal levels' cells)."""
    L, H, W = shapes.shape[0], int(shapes[0, 0]), int(shapes[0, 1])
    if not band:
        return t, (0, 2, 3)
    nb = W // band
    return t.reshape(t.shape[0], L, H, nb, band, *t.shape[2:]), (0, 3, 5, 6)


def skew_bars(case, got, ref, gv_floor=0.0):
    """Block bars of one skewed case.  got: the library's gradients on the CPU (public: grad_value, grad_sampling_loc,
    grad_attn_weight; fused: grad_value, grad of the raw tensor); ref: skew_reference(case).
    -> {gradient: block_bar(...)}: grad_value within 2e-5 (+ gv_floor) of its block's maximum, the sampling gradients within
    2e-4 of theirs (offsets away from texel centres)."""
    form, a, skew = skew_spec(case)
    shapes = ref["shapes"]
    M, L = a["M"], a["L"]
    band = skew[1] if skew[0] == "band" else 0
    out = {}
    v, dims, keep = _value_blocks(got[0], shapes, M, band)
    out["grad_value"] = block_bar(v, _value_blocks(ref["gv"], shapes, M, band)[0], dims, 2e-5, gv_floor, keep)
    smooth = ref["smooth"][..., None]
    if form == "public":
        pairs = (("grad_sampling_loc", got[1], ref["gl"], smooth), ("grad_attn_weight", got[2], ref["ga"], None))
    else:
        goff, glogit = fused_plain(got[1], ref["rows"], M, L)
        pairs = (("grad_offsets", goff, ref["gl"], smooth), ("grad_logits", glogit, ref["ga"], None))
    for name, g, r, m in pairs:
        gq, dims = _query_blocks(g, shapes, band)
        rq = _query_blocks(r, shapes, band)[0]
        mq = _query_blocks(m.expand_as(r), shapes, band)[0] if m is not None else None
        out[name] = block_bar(gq, rq, dims, 2e-4, 0.0, mq)
    return out


def assert_skew_bars(case, bars):
    """Every block bar holds, and the case is not vacuous: the grad_value blocks' maxima span 2^20 or more and every block's
    maximum is a normal fp32 number above 1e-30."""
    gv = bars["grad_value"]
    assert gv["blocks_max"] >= 2.0 ** 20 * gv["blocks_min"], (case, gv)
    for name, b in bars.items():
        assert b["blocks_min"] > 1e-30, (case, name, b)
    for name, b in bars.items():
        assert b["ratio"] <= 1.0, (f"{case}: {name} block {b['block']} err {b['err']:.3g} vs block max {b['ref_max']:.3g} "
                                   f"({b['ratio']:.3g} x the bar)")


_SKEW_REF = {}


def skew_reference(case):
    """fp64 oracle gradients of a skewed case (cached per process, kept as fp32: the bars are 2e-5 and wider) + what the bars
    need: shapes, the texel-centre mask, the raw layout's rows (fused)."""
    if case not in _SKEW_REF:
        from oracle import c_oracle
        form, x = skew_case(case)
        if form == "public":
            value, shapes, lsi, loc, aw, go = x
            gv, gl, ga = c_oracle.msda_backward(value.double(), shapes, lsi, loc.double(), aw.double(), go.double())
            rows = None
        else:
            value, shapes, lsi, refp, raw, rows, go = x
            gv, gl, ga, loc = fused_reference(value, shapes, lsi, refp, raw, rows, go)
        _SKEW_REF[case] = dict(gv=gv.float(), gl=gl.float(), ga=ga.float(), shapes=shapes, rows=rows, smooth=texel_smooth(loc, shapes))
    return _SKEW_REF[case]


# ---- the 16-bit bar: one rounding on the way out (test_half_inference_gpu.py, test_half_edges_gpu.py) ----
def ulp_of(dtype):
    return 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8


def assert_rounded_once(out, ref, dtype, floor, extra=None):
    """|out - ref| <= ulp |ref| + floor (+ extra) on EVERY element, and out is ref rounded to nearest on >= 99 % of them."""
    assert out.dtype == dtype and out.shape == ref.shape
    o = out.detach().cpu()
    err = (o.double() - ref.double()).abs()
    bar = ulp_of(dtype) * ref.double().abs() + floor
    if extra is not None:
        bar = bar + extra
    worst = (err - bar).max().item()
    same = (o == ref.to(dtype)).float().mean().item()
    print(f"max |err| {err.max().item():.3e}, max (err - bar) {worst:.3e}, rounded-equal {same:.5f}")
    assert (err <= bar).all(), (err.max().item(), worst)
    assert same >= 0.99, same
    return same
