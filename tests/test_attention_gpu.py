"""Fused multi-head attention on the MI355X: the MFMA and the generic kernels of csrc/attention.hip against the fp64 oracle,
within the bars of attention_oracle (see tests/test_attention.py), with the route pinned by last_kernel(); determinism,
dropout, peak memory, streams; the trans aggregator and model on the device against the CPU host path.  The case table of
attention_cases.py (MFMA tile edges, strided layouts, grad_out forms, wide heads, fp64, dropout, large logits) runs with
the per-element gradient bars; every ``ATBAR route case tensor err/bar`` line is a figure of DESIGN.md section 4.8.

Each fp64 oracle case is evaluated once per module (``_oracle``, ``attention_cases.oracle``)."""
import ctypes
import functools
import importlib
import math

import pytest
import torch

import attention_cases as ac
import attention_oracle as ao

pytestmark = pytest.mark.gpu

DEV = "cuda"

WILDTRACK, MULTIVIEWX, STRESS16, BATCH2 = (1, 8, 2700, 2700, 16), (1, 8, 2520, 2520, 16), (1, 8, 2700, 2700, 32), (2, 8, 2700, 2700, 16)
# tails: Sq, Sk from {1, 12, 63, 64, 65, 130} in mixed pairs
TAILS = [(2, 3, 1, 130, 16), (1, 2, 12, 63, 32), (2, 2, 63, 64, 16), (1, 3, 64, 65, 32), (1, 2, 65, 12, 16), (2, 2, 130, 1, 32),
         (1, 2, 130, 130, 16), (1, 2, 64, 64, 32)]


def _ops():
    return importlib.import_module("mvdetr_amd.ops.attention")


@functools.lru_cache(maxsize=None)
def _inputs(size, seed=0, amp=1.0, dtype=torch.float32):
    B, H, Sq, Sk, D = size
    g = torch.Generator().manual_seed(seed * 100 + Sq + Sk)
    q, k, v = (torch.randn(B, H, S, D, generator=g) for S in (Sq, Sk, Sk))
    gout = torch.randn(B, H, Sq, D, generator=g)
    if amp != 1.0:                                   # logits of magnitude ~amp: std(q . k / sqrt(D)) = amp
        q, k = q * math.sqrt(amp), k * math.sqrt(amp)
    return tuple(x.to(dtype) for x in (q, k, v, gout))


@functools.lru_cache(maxsize=None)
def _oracle(size, seed=0, amp=1.0):
    q, k, v, _ = _inputs(size, seed, amp)
    return ao.attention(q, k, v), ao.fp32_bar(q, k, v)


@functools.lru_cache(maxsize=None)
def _oracle_grads(size, seed=0):
    q, k, v, gout = _inputs(size, seed)
    return ao.with_grads(q, k, v, gout)[1:], ao.grad_bars(q, k, v, gout)


@functools.lru_cache(maxsize=None)
def _oracle_grad_bars_elementwise(size, seed=0):
    return ao.grad_bars_elementwise(*_inputs(size, seed))


def _forward_check(size, want_kernel, seed=0, amp=1.0, layout="dense"):
    op = _ops()
    q, k, v, _ = _inputs(size, seed, amp)
    B, H, Sq, Sk, D = size
    if layout == "dense":
        qd, kd, vd = (x.to(DEV) for x in (q, k, v))
    else:                                            # head-split views of seq-first / batch-first token tensors
        perm, back = ((1, 2, 0, 3), (2, 0, 1, 3)) if layout == "seq_first" else ((0, 2, 1, 3), (0, 2, 1, 3))
        qd, kd, vd = (x.to(DEV).permute(back).contiguous().permute(perm) for x in (q, k, v))
        assert not qd.is_contiguous() or 1 in (B, H, Sq)
    got = op.attention(qd, kd, vd)
    torch.cuda.synchronize()
    assert op.last_kernel() == want_kernel
    want, bar = _oracle(size, seed, amp)
    assert torch.isfinite(got).all()
    ratio = ((got.cpu().double() - want).abs() / bar).max().item()
    print(f"{want_kernel} {size} amp {amp} {layout}: err / bar = {ratio:.3f}")
    assert ratio <= 1.0, (size, ratio)
    return got


@pytest.mark.parametrize("size", [WILDTRACK, MULTIVIEWX, STRESS16, BATCH2])
def test_forward_mfma_model_sizes(size):
    _forward_check(size, "attn_fwd_mfma")
    want, bar = _oracle(size)
    q, k, v, _ = _inputs(size)
    assert ((ao.attention(q[:1, :2], k[:1, :2], v[:1, :2], drop_last_key=True) - want[:1, :2]).abs() > bar[:1, :2]).any()


@pytest.mark.parametrize("size", TAILS)
def test_forward_mfma_tails(size):
    _forward_check(size, "attn_fwd_mfma")
    _forward_check(size, "attn_fwd_mfma", layout="seq_first")
    _forward_check(size, "attn_fwd_mfma", layout="batch_first")


@pytest.mark.parametrize("D", [4, 20, 64])
def test_forward_generic_route(D):
    for Sq, Sk in ((65, 130), (12, 63), (130, 1)):
        _forward_check((2, 3, Sq, Sk, D), "attn_fwd_generic")
    _forward_check((2, 3, 65, 130, D), "attn_fwd_generic", layout="seq_first")


def test_generic_route_takes_what_the_fast_one_cannot():
    """fp64, and fp32 rows that are not 16-byte aligned, go to the generic kernels and give the same answer."""
    op = _ops()
    size = (1, 2, 65, 130, 16)
    q, k, v, _ = _inputs(size)
    want, bar = _oracle(size)
    got = op.attention(q.double().to(DEV), k.double().to(DEV), v.double().to(DEV))
    assert op.last_kernel() == "attn_fwd_generic"
    assert torch.allclose(got.cpu(), want, atol=1e-12, rtol=1e-12)
    pad = torch.zeros(1, 2, 65, 17, device=DEV)
    pad[..., 1:] = q.to(DEV)
    got = op.attention(pad[..., 1:], k.to(DEV), v.to(DEV))              # rows start 4 bytes off a 16-byte boundary
    assert op.last_kernel() == "attn_fwd_generic"
    assert ((got.cpu().double() - want).abs() <= bar).all()


@pytest.mark.parametrize("size", [(1, 8, 2700, 2700, 16), (1, 2, 65, 130, 32), (1, 2, 130, 63, 4)])
def test_large_logits_stay_finite_and_within_the_bar(size):
    """Logits of magnitude ~80: exp of the unreduced scores would overflow fp32; the bar grows with |q| |k| by construction."""
    q, k, _, _ = _inputs(size, 0, 80.0)
    assert (q[0, 0] @ k[0, 0].t() / math.sqrt(size[4])).abs().max() > 88.8       # exp(88.8) overflows fp32
    _forward_check(size, "attn_fwd_mfma" if size[4] in (16, 32) else "attn_fwd_generic", amp=80.0)


@pytest.mark.parametrize("D", [16, 32, 20])
def test_equal_scores_return_the_mean_of_v(D):
    op = _ops()
    g = torch.Generator().manual_seed(2)
    k = torch.randn(1, 2, 130, D, generator=g).to(DEV)
    v = torch.randn(1, 2, 130, D, generator=g).to(DEV)
    q = torch.zeros(1, 2, 65, D, device=DEV)                       # every score of a row is 0
    got = op.attention(q, k, v)
    want = v.double().mean(2, keepdim=True).expand(-1, -1, 65, -1)
    assert (got.double() - want).abs().max().item() <= ao.EPS32 * (2 * (math.sqrt(130) + 4)) * v.abs().max().item()


def _backward_check(size, want_kernel):
    op = _ops()
    q, k, v, gout = _inputs(size)
    leaves = [x.to(DEV).requires_grad_(True) for x in (q, k, v)]
    op.attention(*leaves).backward(gout.to(DEV))
    torch.cuda.synchronize()
    assert op.last_kernel() == want_kernel
    want, bars = _oracle_grads(size)
    for name, a, b, bar in zip("qkv", leaves, want, bars):
        err = (a.grad.cpu().double() - b).abs().max().item()
        print(f"{want_kernel} {size} grad_{name}: err / bar = {err / bar:.3f}")
        assert err <= bar, (name, err, bar)
        assert b.abs().max().item() > 0, name
    if max(size[2:4]) <= 130:                             # the small shapes: per element as well
        for name, a, b, bar in zip("qkv", leaves, want, _oracle_grad_bars_elementwise(size)):
            r = ac.ratio(a.grad.cpu(), b, bar)
            print(f"ATBAR {want_kernel} {size} grad_{name} {r:.3f}")
            assert r <= 1.0, (name, r)


@pytest.mark.parametrize("size", [WILDTRACK, STRESS16, (2, 3, 12, 130, 16), (1, 2, 63, 64, 32), (2, 2, 65, 12, 16), (1, 2, 130, 65, 32)])
def test_backward_mfma(size):
    _backward_check(size, "attn_bwd_mfma")


@pytest.mark.parametrize("size", [(2, 3, 65, 130, 4), (1, 2, 12, 63, 20), (1, 2, 130, 65, 64)])
def test_backward_generic(size):
    _backward_check(size, "attn_bwd_generic")


# ---- the case table -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ac.TABLE, ids=lambda c: c.name)
def test_table_on_the_device(case):
    """Every case in its own layout and grad_out form: routes pinned after the forward and after the backward, out within
    fp32_bar, gradients within the per-element (and per-tensor) bars; fp64 cases at 1e-12 / 1e-11."""
    out, grads, fwd, bwd = ac.run(_ops(), case, DEV)
    assert (fwd, bwd) == ("attn_" + case.fwd, "attn_" + case.bwd)
    if case.dtype == torch.float64:
        ac.check_fp64(case, out, grads)
    else:
        ac.check_out(case, out, fwd)
        ac.check_grads(case, grads, bwd)


@pytest.mark.parametrize("case", [c for c in ac.TABLE if c.layout != "dense" or c.gout == "expanded"], ids=lambda c: c.name)
def test_strided_layouts_equal_the_dense_run(case):
    """The kernels' arithmetic does not depend on addresses: packed / split, seq-first / batch-first operands and an
    expanded grad_out give the bits of the dense run.  (The misaligned grad_out takes another backward route than the
    dense run, attn_bwd_generic after attn_fwd_mfma: it has the oracle's bars in test_table_on_the_device only.)"""
    out, grads, fwd, bwd = ac.run(_ops(), case, DEV)
    ref_out, ref_grads, ref_fwd, ref_bwd = ac.run(_ops(), case, DEV, layout="dense", gout="proj")
    assert (fwd, bwd) == (ref_fwd, ref_bwd) == ("attn_" + case.fwd, "attn_" + case.bwd)
    assert torch.equal(out, ref_out)
    for name, a, b in zip("qkv", grads, ref_grads):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("D,fwd,bwd", [(16, "attn_fwd_mfma", "attn_bwd_mfma"), (65, "attn_fwd_generic", "attn_bwd_generic")])
def test_padded_outputs_through_the_c_entry_points(D, fwd, bwd):
    """out, grad_q, grad_k, grad_v with a token stride of D + 4 in NaN-filled buffers: the rows are the op's bit for bit
    and no pad element is written (attn_store_acc's d0 < D on the MFMA route, lane + 64 c < D on the generic one)."""
    from mvdetr_amd import _lib
    op, lib = _ops(), _lib.lib()
    B, H, Sq, Sk = 2, 2, 33, 97
    g = torch.Generator().manual_seed(D)
    q, k, v, gout = (torch.randn(B, H, S, D, generator=g).to(DEV) for S in (Sq, Sk, Sk, Sq))
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
    ref = op.attention(*leaves)
    ref.backward(gout)
    assert op.last_kernel() == bwd
    bufs = [torch.full((B, H, S, D + 4), float("nan"), device=DEV) for S in (Sq, Sq, Sk, Sk)]      # out, gq, gk, gv
    out, gq, gk, gv = bufs
    lse = torch.empty(B, H, Sq, device=DEV)
    stream = _lib.current_stream_ptr(q.device)

    def strides(*tensors):
        flat = [s for t in tensors for s in t.stride()[:3]]
        return (ctypes.c_int64 * len(flat))(*flat)
    rc = lib.mvdetr_attention_forward_f32(stream, q.data_ptr(), k.data_ptr(), v.data_ptr(), strides(q, k, v, out), B, H, Sq, Sk, D,
                                          0.0, 0, out.data_ptr(), lse.data_ptr())
    assert rc == 0 and op.last_kernel() == fwd
    work = torch.empty(lib.mvdetr_attention_workspace_bytes(B, H, Sq, Sk, D, 4), dtype=torch.uint8, device=DEV)
    rc = lib.mvdetr_attention_backward_f32(stream, gout.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
                                           lse.data_ptr(), strides(q, k, v, out, gout, gq, gk, gv), B, H, Sq, Sk, D, 0.0, 0,
                                           work.data_ptr(), gq.data_ptr(), gk.data_ptr(), gv.data_ptr())
    assert rc == 0 and op.last_kernel() == bwd
    torch.cuda.synchronize()
    for name, buf, want in zip(("out", "grad_q", "grad_k", "grad_v"), bufs, (ref.detach(), *(x.grad for x in leaves))):
        assert torch.equal(buf[..., :D], want), name
        assert torch.isnan(buf[..., D:]).all(), name


@pytest.mark.parametrize("batch_first", [False, True])
@pytest.mark.parametrize("E,heads,routes", [(64, 4, ("attn_fwd_mfma", "attn_bwd_mfma")), (40, 2, ("attn_fwd_generic", "attn_bwd_generic"))])
def test_module_on_the_device_is_fp64_nn_multihead_attention(E, heads, routes, batch_first):
    from test_attention import module_against_fp64_torch
    module_against_fp64_torch(E, heads, batch_first, DEV, routes)


def test_device_fp64_gradcheck():
    op = _ops()
    g = torch.Generator().manual_seed(6)
    q = torch.randn(1, 2, 5, 3, generator=g, dtype=torch.float64).to(DEV).requires_grad_(True)
    k = torch.randn(1, 2, 7, 3, generator=g, dtype=torch.float64).to(DEV).requires_grad_(True)
    v = torch.randn(1, 2, 7, 3, generator=g, dtype=torch.float64).to(DEV).requires_grad_(True)
    assert torch.autograd.gradcheck(op.attention, (q, k, v), eps=1e-6, atol=1e-7)
    assert op.last_kernel() == "attn_bwd_generic"
    assert torch.autograd.gradcheck(lambda a, b, c: op.attention(a, b, c, 0.3, 9), (q, k, v), eps=1e-6, atol=1e-7)


@pytest.mark.parametrize("size,p", [(WILDTRACK, 0.0), ((2, 3, 65, 130, 32), 0.2), ((2, 3, 65, 130, 20), 0.0), ((1, 2, 130, 63, 4), 0.2)])
def test_two_runs_are_bitwise_equal(size, p):
    op = _ops()
    q, k, v, gout = (x.to(DEV) for x in _inputs(size))
    runs = []
    for _ in range(2):
        leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
        out = op.attention(*leaves, dropout_p=p, seed=31)
        out.backward(gout)
        runs.append([out.detach()] + [x.grad for x in leaves])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("size,fwd,bwd", [((2, 3, 65, 130, 16), "attn_fwd_mfma", "attn_bwd_mfma"),
                                          ((1, 2, 130, 63, 32), "attn_fwd_mfma", "attn_bwd_mfma"),
                                          ((2, 3, 65, 130, 20), "attn_fwd_generic", "attn_bwd_generic")])
def test_dropout_matches_the_oracle_given_the_mask(size, fwd, bwd):
    op = _ops()
    p, seed = 0.25, 2 ** 63 + 12345
    q, k, v, gout = _inputs(size)
    keep = op.dropout_keep_mask(seed, p, *size[:4])
    leaves = [x.to(DEV).requires_grad_(True) for x in (q, k, v)]
    got = op.attention(*leaves, dropout_p=p, seed=seed)
    assert op.last_kernel() == fwd
    got.backward(gout.to(DEV))
    assert op.last_kernel() == bwd
    want = ao.with_grads(q, k, v, gout, keep, p)
    assert (want[0] - _oracle(size)[0]).abs().max() > 0.01
    assert ((got.detach().cpu().double() - want[0]).abs() <= _oracle(size)[1] / (1 - p)).all()
    for name, a, b, bar in zip("qkv", leaves, want[1:], _oracle_grads(size)[1]):
        err = (a.grad.cpu().double() - b).abs().max().item()
        assert err <= bar / (1 - p), (name, err, bar)


def test_peak_memory_stays_far_below_one_score_tensor():
    op = _ops()
    B, H, Sq, Sk, D = WILDTRACK
    leaves = [x.to(DEV).requires_grad_(True) for x in _inputs(WILDTRACK)[:3]]
    gout = _inputs(WILDTRACK)[3].to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    op.attention(*leaves).backward(gout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"peak memory of forward + backward at Wildtrack size: {peak / 2 ** 20:.1f} MiB")
    assert peak < B * H * Sq * Sk * 4
    assert peak < 16 * 2 ** 20                                       # out, lse, delta and three gradients


def test_side_stream_and_inputs_unchanged():
    op = _ops()
    leaves = [x.to(DEV).requires_grad_(True) for x in _inputs((2, 3, 130, 65, 16))[:3]]
    keep = [x.detach().clone() for x in leaves]
    ref = op.attention(*leaves).detach()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch.cuda._sleep(2_000_000)                      # the side stream is busy: a launch on the default one would race
        out = op.attention(*leaves)
        out.sum().backward()
    s.synchronize()
    assert torch.equal(out.detach(), ref)
    for x, kept in zip(leaves, keep):
        assert torch.equal(x.detach(), kept)
        assert torch.isfinite(x.grad).all()
    assert leaves[2].grad.abs().sum().item() > 0


def test_mini_trans_model_gpu_matches_cpu():
    from mvdetr_amd import geometry
    from mvdetr_amd.model import build_model
    g = torch.Generator().manual_seed(3)
    imgs = torch.randn(1, 3, 3, *geometry.MINI.input_img_shape, generator=g)
    M = geometry.random_affine_mats(1, 3, geometry.MINI.input_img_shape, seed=2, translate=0.05, scale=(0.9, 1.1))
    cpu = build_model("mini", seed=0, world_feat_arch="trans", channels_last=False).eval()
    gpu = build_model("mini", seed=0, world_feat_arch="trans").to(DEV).eval()
    with torch.no_grad():
        feat = cpu.features(imgs)
        proj = cpu.frame_proj_mats(M)
        want = cpu.hot_path(feat, proj)
        got = gpu.hot_path(feat.to(DEV), proj.to(DEV))
        assert _ops().last_kernel() == "attn_fwd_generic"            # 32 channels over 8 heads: D = 4
    err = (got.cpu() - want).abs().max().item()
    assert err <= 1e-4 * max(1.0, want.abs().max().item()), err


def test_fullsize_wildtrack_aggregator_gpu_matches_cpu_and_trains():
    from mvdetr_amd.world_feat import TransformerWorldFeat
    torch.manual_seed(0)
    model = TransformerWorldFeat(7, (120, 360), 128, hidden_dim=128).eval()
    x = torch.randn(1, 7, 128, 120, 360, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = model(x)
        model.to(DEV)
        got = model(x.to(DEV))
        assert _ops().last_kernel() == "attn_fwd_mfma"
    err = (got.cpu() - want).abs().max().item()
    assert err <= 1e-4 * max(1.0, want.abs().max().item()), err
    # a training step (dropout on) runs the MFMA pair and reaches every parameter; a reference-shaped state dict loads
    model.train()
    model(x.to(DEV)).square().mean().backward()
    assert _ops().last_kernel() == "attn_bwd_mfma"
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, n
    layer = torch.nn.MultiheadAttention(128, 8, dropout=0.1)
    state = {k: v.cpu() for k, v in model.state_dict().items()}
    assert all(f"encoder.layers.0.self_attn.{k}" in state for k in layer.state_dict())
    TransformerWorldFeat(7, (120, 360), 128, hidden_dim=128).load_state_dict(state, strict=True)


def test_wildtrack_model_runs_and_trains_through_the_mfma_kernels():
    """MVDeTr(world_feat_arch="trans") at Wildtrack size: warp + aggregator + world heads forward (eval) and one training
    step, on attn_fwd_mfma / attn_bwd_mfma (128 channels over 8 heads: D = 16)."""
    from mvdetr_amd import geometry
    from mvdetr_amd.model import build_model
    geom = geometry.WILDTRACK
    model = build_model("wildtrack", seed=0, world_feat_arch="trans").to(DEV)
    g = torch.Generator().manual_seed(4)
    feat = torch.randn(geom.num_cam, geom.feat_channels, *geom.Rimg_shape, generator=g).to(DEV)
    M = geometry.random_affine_mats(1, geom.num_cam, geom.input_img_shape, seed=2, translate=0.05, scale=(0.9, 1.1))
    proj = model.frame_proj_mats(M, DEV)
    model.eval()
    with torch.no_grad():
        world = model.hot_path(feat.contiguous(memory_format=torch.channels_last), proj)
        assert _ops().last_kernel() == "attn_fwd_mfma"
        assert world.shape == (1, geom.feat_channels, *geom.Rworld_shape) and torch.isfinite(world).all()
        assert torch.allclose(world, model.hot_path(feat, proj), atol=1e-4 * max(1.0, world.abs().max().item()))
    model.train()
    world = model.hot_path(feat, proj)
    (model.world_heatmap(world).square().mean() + model.world_offset(world).square().mean()).backward()
    assert _ops().last_kernel() == "attn_bwd_mfma"
    for n, p in model.world_feat.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, n
