"""Fused multi-head attention on the library's host path, ops.MultiheadAttention, the TransformerWorldFeat aggregator and
MVDeTr(world_feat_arch="trans") on CPU tensors.

The fp32 bar is attention_oracle.fp32_bar: an error model of the fp32 arithmetic evaluated per element by the fp64 oracle
from |.|-operand quantities (score error (D + 4) eps A_ij + 4 eps max_j A_ij with A_ij = scale sum_d |q_id| |k_jd|, entering
the probabilities as a relative error; a random-walk accumulation term 2 (sqrt(Sk) + 4) eps sum_j p_ij |v_jd|), times
MARGIN = 1, the smallest whole number with which torch's own fp32 composition passes at every size and seed used here and in
test_attention_gpu.py (observed err / bar: torch's composition <= 0.07, the host path <= 0.10, the device kernels <= 0.08).  The bar
tests itself: the oracle with one key left out must exceed it, torch's fp32 composition must pass it.

Gradients are held to attention_oracle.grad_bars_elementwise (one bound per gradient element, formula in that module's
docstring) on the case table of attention_cases.py: the bars test themselves against torch's fp32 composition (MARGIN = 1) and
nine oracle-made mutants, and the host path runs every case of the table in fp32 and fp64, strided layouts bit-equal to the
dense run.  test_attention_gpu.py runs the same table on the device."""
import math

import numpy as np
import pytest
import torch
from torch import nn

import attention_cases as ac
import attention_oracle as ao
from conftest import load_golden, t

# (B, H, Sq, Sk, D): self- and cross-attention, sizes below, at and across the host path's 64-key tile
SIZES = [(2, 3, 70, 130, 4), (1, 2, 65, 65, 16), (1, 2, 130, 63, 32), (2, 2, 1, 64, 16), (1, 2, 12, 130, 16), (1, 2, 63, 65, 32),
         (1, 1, 64, 1, 8)]
SEEDS = [0, 1, 2]


def _ops():
    import importlib
    return importlib.import_module("mvdetr_amd.ops.attention")      # (ops.attention itself is the function)


def _case(size, seed, dtype=torch.float32):
    B, H, Sq, Sk, D = size
    g = torch.Generator().manual_seed(seed * 100 + Sq)
    q, k, v = (torch.randn(B, H, S, D, generator=g) for S in (Sq, Sk, Sk))
    return q.to(dtype), k.to(dtype), v.to(dtype), torch.randn(B, H, Sq, D, generator=g).to(dtype)


def torch_fp32_composition(q, k, v):
    return torch.softmax(q @ k.transpose(-1, -2) * (1.0 / math.sqrt(q.shape[-1])), -1) @ v


def _check_grads(got, q, k, v, gout, keep=None, p=0.0):
    """got = (grad_q, grad_k, grad_v) fp32 vs the oracle within attention_oracle.grad_bars."""
    want = ao.with_grads(q, k, v, gout, keep, p)[1:]
    bars = ao.grad_bars(q, k, v, gout)
    if p:
        bars = [b / (1.0 - p) for b in bars]
    for name, a, b, bar in zip("qkv", got, want, bars):
        err = (a.double() - b).abs().max().item()
        assert err <= bar, (name, err, bar)
        assert b.abs().max().item() > 0 or (k.shape[2] == 1 and name != "v"), name      # (one key: dq = dk = 0)


def test_public_names_exist():
    from mvdetr_amd.ops import MultiheadAttention, attention  # noqa: F401
    from mvdetr_amd.world_feat import TransformerEncoder, TransformerEncoderLayer, TransformerWorldFeat  # noqa: F401


@pytest.mark.parametrize("size", SIZES)
def test_the_bar_tests_itself(size):
    """One key left out EXCEEDS the bar somewhere; torch's own fp32 composition PASSES it everywhere."""
    for seed in SEEDS:
        q, k, v, _ = _case(size, seed)
        want, bar = ao.attention(q, k, v), ao.fp32_bar(q, k, v)
        if size[3] > 1:
            assert ((ao.attention(q, k, v, drop_last_key=True) - want).abs() > bar).any()
        ratio = ((torch_fp32_composition(q, k, v).double() - want).abs() / bar).max().item()
        print(f"torch fp32 composition {size} seed {seed}: err / bar = {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("size", SIZES)
def test_host_path_matches_the_oracle(size, dtype):
    op = _ops()
    for seed in SEEDS[:2]:
        q, k, v, gout = _case(size, seed, dtype)
        leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
        got = op.attention(*leaves)
        got.backward(gout)
        want = ao.attention(q, k, v)
        if dtype == torch.float64:
            assert torch.allclose(got.detach(), want, atol=1e-12, rtol=1e-12)
            for a, b in zip(leaves, ao.with_grads(q, k, v, gout)[1:]):
                assert torch.allclose(a.grad, b, atol=1e-11, rtol=1e-11)
        else:
            ratio = ((got.detach().double() - want).abs() / ao.fp32_bar(q, k, v)).max().item()
            print(f"host path {size} seed {seed}: err / bar = {ratio:.3f}")
            assert ratio <= 1.0
            _check_grads([x.grad for x in leaves], q, k, v, gout)


@pytest.mark.parametrize("batch_first", [False, True])
def test_strided_projections_are_read_in_place(batch_first):
    """Head-split views of a packed [S, B, 3E] (seq-first) or [B, S, 3E] (batch-first) projection reach the entry point as
    they are (same data_ptr, same strides), and the result equals that of dense copies."""
    op = _ops()
    S, B, H, D = 70, 2, 3, 8
    g = torch.Generator().manual_seed(5)
    packed = torch.randn((B, S, 3 * H * D) if batch_first else (S, B, 3 * H * D), generator=g).requires_grad_(True)
    perm = (0, 2, 1, 3) if batch_first else (1, 2, 0, 3)
    q, k, v = (x.unflatten(-1, (H, D)).permute(perm) for x in packed.split(H * D, dim=-1))
    assert not q.is_contiguous()
    out = op.attention(q, k, v)
    saved = out.grad_fn.saved_tensors
    for view, reached in zip((q, k, v), saved[:3]):
        assert reached.data_ptr() == view.data_ptr() and reached.stride() == view.stride()
    assert saved[3].stride() == out.stride() and out.permute((0, 2, 1, 3) if batch_first else (2, 0, 1, 3)).is_contiguous()
    gout = torch.randn(out.shape, generator=g)
    out.backward(gout)
    dense = [x.detach().contiguous().requires_grad_(True) for x in (q, k, v)]
    ref = op.attention(*dense)
    ref.backward(gout)
    assert torch.equal(out, ref)
    want = torch.cat([x.grad.permute((0, 2, 1, 3) if batch_first else (2, 0, 1, 3)).flatten(2) for x in dense], -1)
    assert torch.equal(packed.grad, want)


def test_host_path_fp64_gradcheck():
    op = _ops()
    g = torch.Generator().manual_seed(6)
    q = torch.randn(1, 2, 5, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    k = torch.randn(1, 2, 7, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    v = torch.randn(1, 2, 7, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(op.attention, (q, k, v), eps=1e-6, atol=1e-7)
    assert torch.autograd.gradcheck(lambda a, b, c: op.attention(a, b, c, 0.3, 9), (q, k, v), eps=1e-6, atol=1e-7)


# ---- the case table (attention_cases.py): bars, mutants, the host path ------------------------------------------------------

def _composition_with_grads(case, seed):
    """torch's own fp32 composition differentiated by autograd, with the case's keep mask: the reference MARGIN is set by."""
    q, k, v, gout = ac.make_inputs(case, seed)
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
    P = torch.softmax(leaves[0] @ leaves[1].transpose(-1, -2) * (1.0 / math.sqrt(case.D)), -1)
    if case.dropout:
        P = P * ac.keep_mask(case) / (1.0 - case.dropout)
    (P @ leaves[2]).backward(gout)
    return [x.grad for x in leaves]


@pytest.mark.parametrize("name", ["m16_33x97_seq", "m32_129x1", "w65_5x70_drop", "m32_65x130_amp80"])
def test_explicit_gradient_formulas_are_autograds(name):
    """The formulas the mutants are altered copies of give autograd's gradients when nothing is altered."""
    case = ac.by_name(name)
    q, k, v, gout = ac.make_inputs(case)
    for a, b in zip(ao.grads_explicit(q, k, v, gout, ac.keep_mask(case), case.dropout), ac.oracle(case).grads):
        assert torch.allclose(a, b, atol=1e-12 * max(1.0, b.abs().max().item()), rtol=1e-10)


@pytest.mark.parametrize("case", ac.TABLE, ids=lambda c: c.name)
def test_the_gradient_bars_test_themselves(case):
    """At every case and seed: torch's fp32 composition PASSES the per-element bars (this is what sets MARGIN); no bar
    exceeds the per-tensor one; every mutant EXCEEDS the bar of every tensor it changes, on an element that has a bar."""
    if case.amp != 1.0:
        q, k, _, _ = ac.make_inputs(case)
        assert (q[0, 0] @ k[0, 0].t() / math.sqrt(case.D)).abs().max() > 88.8          # exp(88.8) overflows fp32
    for seed in ac.SEEDS:
        o = ac.oracle(case, seed)
        for name, got, want, bar, tbar in zip("qkv", _composition_with_grads(case, seed), o.grads, o.bars, o.tensor_bars):
            assert bar.shape == want.shape and bar.dtype == torch.float64 and (bar <= tbar).all(), name
            r = ac.ratio(got, want, bar)
            print(f"ATBAR torch_fp32_composition {case.name} seed {seed} grad_{name} {r:.3f}")
            assert r <= 1.0, (name, seed, r)
        for mutant, grads in ac.mutants(case, seed).items():
            for name, mut, want, bar, tbar in zip("qkv", grads, o.grads, o.bars, o.tensor_bars):
                if ac.changed(mut, want, tbar):
                    margin = ((mut - want).abs()[bar > 0] / bar[bar > 0]).max().item()
                    print(f"ATMUT {mutant} {case.name} seed {seed} grad_{name} {margin:.1f}")
                    assert margin > 1.0, (mutant, name, seed, margin)
    if case.gout == "zero_rows":
        o = ac.oracle(case)
        assert (o.bars[0][:, :, -1] == 0).all() and (o.bars[2][..., 0] == 0).all() and (o.bars[1] > 0).all()


def test_every_mutant_applies_somewhere_and_changes_what_it_should():
    seen = {}
    for case in ac.TABLE:
        o = ac.oracle(case)
        for mutant, grads in ac.mutants(case).items():
            hit = seen.setdefault(mutant, set())
            hit.update(n for n, mut, want, tbar in zip("qkv", grads, o.grads, o.tensor_bars) if ac.changed(mut, want, tbar))
    assert sorted(seen) == ["1_last_key_left_out", "2_keys_32_63_left_out", "3_last_gout_row_zeroed", "4_one_gout_element_zeroed",
                            "5_delta_omitted", "6_scale_missing_from_dq", "7_heads_of_k_swapped", "8_keep_ignored_in_backward",
                            "9_keep_transposed_in_tile"]
    assert seen.pop("5_delta_omitted") == {"q", "k"} and seen.pop("6_scale_missing_from_dq") == {"q"}
    assert all(v == {"q", "k", "v"} for v in seen.values()), seen


@pytest.mark.parametrize("name,seed,mutant,tensor", [("w200_66x3", 1, "4_one_gout_element_zeroed", 1),
                                                     ("m32_65x130_amp80", 0, "1_last_key_left_out", 0)])
def test_the_per_tensor_bars_miss_what_the_per_element_bars_catch(name, seed, mutant, tensor):
    """Why the per-element bars exist: one zeroed grad_out element moves grad_k of w200_66x3 by at most 0.28 of its
    per-tensor bar, a left-out key grad_q of m32_65x130_amp80 by 0.22 of it."""
    case = ac.by_name(name)
    o = ac.oracle(case, seed)
    d = (ac.mutants(case, seed)[mutant][tensor] - o.grads[tensor]).abs()
    assert d.max().item() <= o.tensor_bars[tensor]
    assert (d > o.bars[tensor]).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", ac.TABLE, ids=lambda c: c.name)
def test_host_path_on_the_table(case, dtype):
    """The host path on every case, in the case's layout and grad_out form: fp32 within fp32_bar and the per-element
    gradient bars, fp64 at 1e-12 / 1e-11; a strided run is bit-equal to the dense one."""
    op = _ops()
    out, grads, _, _ = ac.run(op, case, dtype=dtype)
    if dtype == torch.float64:
        ac.check_fp64(case, out, grads)
    else:
        ac.check_out(case, out, "host_path")
        ac.check_grads(case, grads, "host_path")
    if case.layout != "dense" or case.gout in ("expanded", "misaligned"):
        ref_out, ref_grads, _, _ = ac.run(op, case, dtype=dtype, layout="dense", gout="proj")
        assert torch.equal(out, ref_out)
        for a, b in zip(grads, ref_grads):
            assert torch.equal(a, b)


@pytest.mark.parametrize("case", [c for c in ac.TABLE if c.layout != "dense"], ids=lambda c: c.name)
def test_table_layouts_reach_the_entry_point_in_place(case):
    """The head-split views of the table are what the library is handed (no dense copy), and out lies in memory like q."""
    op = _ops()
    x = ac.lay_out(case)
    out = op.attention(x.q, x.k, x.v)
    for view, reached in zip((x.q, x.k, x.v), out.grad_fn.saved_tensors[:3]):
        assert reached.data_ptr() == view.data_ptr() and reached.stride() == view.stride()
    assert len({t.data_ptr() for t in (x.q, x.k, x.v)}) == 3 and len(x.leaves) == (1 if case.Sq == case.Sk else 2)
    assert out.permute((0, 2, 1, 3) if case.layout == "batch_first" else (2, 0, 1, 3)).is_contiguous()
    assert x.gout.permute((0, 2, 1, 3) if case.layout == "batch_first" else (2, 0, 1, 3)).is_contiguous()


def test_bad_calls_raise_clear_errors():
    op = _ops()
    q = torch.randn(1, 2, 4, 8)
    with pytest.raises(RuntimeError, match="not implemented for"):
        op.attention(q.half(), q.half(), q.half())
    with pytest.raises(RuntimeError, match="one dtype"):
        op.attention(q, q.double(), q)
    with pytest.raises(ValueError, match="4-D"):
        op.attention(q[0], q[0], q[0])
    with pytest.raises(ValueError, match="must both be"):
        op.attention(q, q, q[:, :, :2])
    with pytest.raises(ValueError, match="dropout_p"):
        op.attention(q, q, q, 1.0)
    with pytest.raises(ValueError, match="head dimension"):
        op.attention(*(torch.randn(1, 1, 2, 257),) * 3)
    if torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="one device"):
            op.attention(q.cuda(), q, q)


# ---- dropout ----------------------------------------------------------------------------------------------------------------

def test_dropout_mask_is_a_fair_deterministic_hash():
    op = _ops()
    p, shape = 0.1, (2, 4, 360, 400)                          # 1,152,000 decisions
    a = op.dropout_keep_mask(1234, p, *shape)
    assert torch.equal(a, op.dropout_keep_mask(1234, p, *shape))
    b = op.dropout_keep_mask(1235, p, *shape)
    assert not torch.equal(a, b)
    assert abs((a ^ b).double().mean().item() - 2 * p * (1 - p)) < 0.01          # independent of the neighbouring seed's

    def fair(frac, n):
        return (frac - (1 - p)).abs().max().item() <= 4 * math.sqrt(p * (1 - p) / n)
    n = a.numel()
    assert fair(a.double().mean().reshape(1), n)
    assert fair(a.double().mean((0, 1, 3)), n // shape[2])                       # per query row i
    assert fair(a.double().mean((0, 1, 2)), n // shape[3])                       # per key column j
    assert op.dropout_keep_mask(7, 0.0, 1, 1, 8, 8).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_host_path_dropout_matches_the_oracle_given_the_mask(dtype):
    op = _ops()
    size, p, seed = (2, 3, 70, 130, 4), 0.25, 99
    q, k, v, gout = _case(size, 3, dtype)
    keep = op.dropout_keep_mask(seed, p, *size[:4])
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
    got = op.attention(*leaves, dropout_p=p, seed=seed)
    got.backward(gout)
    want = ao.attention(q, k, v, keep, p)
    assert (want - ao.attention(q, k, v)).abs().max() > 0.01
    if dtype == torch.float64:
        assert torch.allclose(got.detach(), want, atol=1e-12, rtol=1e-12)
        for a, b in zip(leaves, ao.with_grads(q, k, v, gout, keep, p)[1:]):
            assert torch.allclose(a.grad, b, atol=1e-11, rtol=1e-11)
    else:
        assert ((got.detach().double() - want).abs() <= ao.fp32_bar(q, k, v) / (1 - p)).all()
        _check_grads([x.grad for x in leaves], q, k, v, gout, keep, p)


def test_dropout_follows_torch_manual_seed_and_p0_is_eval():
    from mvdetr_amd.ops import MultiheadAttention
    m = MultiheadAttention(32, 8, dropout=0.3).train()
    x = torch.randn(50, 2, 32, generator=torch.Generator().manual_seed(1))
    torch.manual_seed(5)
    a = m(x, x, x, need_weights=False)[0]
    torch.manual_seed(5)
    b = m(x, x, x, need_weights=False)[0]
    c = m(x, x, x, need_weights=False)[0]
    assert torch.equal(a, b) and not torch.equal(a, c)
    m.dropout = 0.0
    train_out = m(x, x, x, need_weights=False)[0]
    assert torch.equal(train_out, m.eval()(x, x, x, need_weights=False)[0])


# ---- the module -------------------------------------------------------------------------------------------------------------

def _module_bar(want):
    """Both sides are fp32 computations of the same formula: 10 x tighter than the model-level bar."""
    return 1e-5 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("batch_first", [False, True])
def test_module_is_nn_multihead_attention(batch_first):
    from mvdetr_amd.ops import MultiheadAttention
    torch.manual_seed(3)
    ours = MultiheadAttention(32, 8, dropout=0.1, batch_first=batch_first).eval()
    theirs = nn.MultiheadAttention(32, 8, dropout=0.1, batch_first=batch_first).eval()
    assert [(n, tuple(p.shape)) for n, p in ours.named_parameters()] == [(n, tuple(p.shape)) for n, p in theirs.named_parameters()]
    torch.manual_seed(4)
    again = MultiheadAttention(32, 8)
    torch.manual_seed(4)
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), nn.MultiheadAttention(32, 8).state_dict().values()))
    with torch.no_grad():
        for p in theirs.parameters():
            p.normal_(0, 0.3)
    ours.load_state_dict(theirs.state_dict(), strict=True)
    theirs.load_state_dict(ours.state_dict(), strict=True)
    g = torch.Generator().manual_seed(8)
    x, y, z = (torch.randn(2, 70, 32, generator=g) if batch_first else torch.randn(70, 2, 32, generator=g) for _ in range(3))
    for args in ((x, x, y), (x, x, x), (x, y, z)):                # q is k; all one; all different
        got, none = ours(*args, need_weights=False)
        want = theirs(*args, need_weights=False)[0]
        assert none is None
        assert (got - want).abs().max().item() <= _module_bar(want)
        gout = torch.randn(want.shape, generator=g)
        for m, o in ((ours, got), (theirs, want)):
            m.zero_grad()
            o.backward(gout)
        for (n, a), b in zip(ours.named_parameters(), theirs.parameters()):
            assert (a.grad - b.grad).abs().max().item() <= _module_bar(b.grad), n
    # calls the fused route does not take return exactly what torch returns
    mask = torch.zeros(2, 70, dtype=torch.bool)
    mask[:, 60:] = True
    for kw in (dict(need_weights=True), dict(key_padding_mask=mask, need_weights=False), dict(key_padding_mask=mask)):
        a, b = ours(x, x, y, **kw), theirs(x, x, y, **kw)
        assert torch.equal(a[0], b[0]) and (a[1] is None) == (b[1] is None) and (a[1] is None or torch.equal(a[1], b[1]))


def module_against_fp64_torch(E, heads, batch_first, device, routes=None):
    """ops.MultiheadAttention (fp32, eval, on ``device``) against fp64 nn.MultiheadAttention on the CPU with the same state
    dict: output, every parameter gradient and the input gradients within _module_bar, for (x, x, x), (x, x, y) and
    (x, y, z) with 70 queries and, in the cross case, 33 keys.  ``routes``: the (forward, backward) last_kernel() names."""
    from mvdetr_amd.ops import MultiheadAttention
    torch.manual_seed(3)
    theirs = nn.MultiheadAttention(E, heads, batch_first=batch_first).double().eval()
    with torch.no_grad():
        for p in theirs.parameters():
            p.normal_(0, 0.3)
    ours = MultiheadAttention(E, heads, batch_first=batch_first).eval()
    ours.load_state_dict({k: v.float() for k, v in theirs.state_dict().items()}, strict=True)
    ours.to(device)
    g = torch.Generator().manual_seed(8)

    def tokens(S):
        return torch.randn((2, S, E) if batch_first else (S, 2, E), generator=g)
    x, y, yk, zv = tokens(70), tokens(70), tokens(33), tokens(33)
    worst = 0.0
    for args in ((x, x, x), (x, x, y), (x, yk, zv)):
        leaves = {id(a): a for a in args}                              # (x, x, x) stays ONE tensor: `query is key`
        dev = {i: a.clone().to(device).requires_grad_(True) for i, a in leaves.items()}
        ref = {i: a.double().requires_grad_(True) for i, a in leaves.items()}
        got, none = ours(*(dev[id(a)] for a in args), need_weights=False)
        assert none is None
        if routes:
            assert _ops().last_kernel() == routes[0]
        want = theirs(*(ref[id(a)] for a in args), need_weights=False)[0]
        gout = torch.randn(want.shape, generator=g)
        ours.zero_grad()
        theirs.zero_grad()
        got.backward(gout.to(device))
        if routes:
            assert _ops().last_kernel() == routes[1]
        want.backward(gout.double())
        pairs = [("out", got.detach(), want.detach())]
        pairs += [(n, a.grad, b.grad) for (n, a), b in zip(ours.named_parameters(), theirs.parameters())]
        pairs += [(f"input{j}", dev[i].grad, ref[i].grad) for j, i in enumerate(leaves)]
        for n, a, b in pairs:
            r = (a.cpu().double() - b).abs().max().item() / _module_bar(b)
            worst = max(worst, r)
            assert r <= 1.0, (n, len(leaves), r)
    print(f"module E {E} heads {heads} batch_first {batch_first} on {device}: worst err / bar = {worst:.3f}")


@pytest.mark.parametrize("batch_first", [False, True])
@pytest.mark.parametrize("E,heads", [(64, 4), (40, 2)])
def test_module_against_fp64_nn_multihead_attention(E, heads, batch_first):
    module_against_fp64_torch(E, heads, batch_first, "cpu")


# ---- the aggregator and the model -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nhead", [8, 2])
def test_golden_transformer_world_feat(nhead):
    """The reference's TransformerWorldFeat (tests/golden/make_golden_trans.py): head dimension 4 and 16."""
    from mvdetr_amd.world_feat import TransformerWorldFeat
    z = load_golden("trans_world_feat_mini.npz")
    num_cam, H, W, dim, dff = (int(x) for x in z["dims"])
    model = TransformerWorldFeat(num_cam, (H, W), dim, hidden_dim=dim, nhead=nhead, dim_feedforward=dff).eval()
    model.load_state_dict({k[2:]: t(a) for k, a in z.items() if k.startswith("p.")}, strict=True)
    want = t(z[f"out_h{nhead}"])
    with torch.no_grad():
        got = model(t(z["x_q8"]).float() / 8)
    err = (got - want).abs().max().item()
    assert got.shape == want.shape and err <= 1e-4 * max(1.0, want.abs().max().item()), err


def test_transformer_world_feat_needs_equal_dims_and_takes_batches():
    from mvdetr_amd.world_feat import TransformerWorldFeat
    with pytest.raises(ValueError, match="hidden_dim == base_dim"):
        TransformerWorldFeat(3, (24, 72), 32, hidden_dim=64)
    torch.manual_seed(0)
    model = TransformerWorldFeat(2, (10, 14), 16, hidden_dim=16, nhead=4, dim_feedforward=32).eval()
    x = torch.randn(3, 2, 16, 10, 14)
    with torch.no_grad():
        both = model(x)
        for b in range(3):
            assert torch.allclose(both[b:b + 1], model(x[b:b + 1]), atol=1e-5)
    assert both.shape == (3, 16, 10, 14) and "pos_embedding" not in model.state_dict()


def test_mini_trans_model_runs_a_frame_and_trains_on_the_cpu():
    from mvdetr_amd import geometry
    from mvdetr_amd.model import build_model
    g = torch.Generator().manual_seed(3)
    imgs = torch.randn(1, 3, 3, *geometry.MINI.input_img_shape, generator=g)
    M = geometry.random_affine_mats(1, 3, geometry.MINI.input_img_shape, seed=2, translate=0.05, scale=(0.9, 1.1))
    model = build_model("mini", seed=0, world_feat_arch="trans", channels_last=False)
    other = build_model("mini", seed=0, world_feat_arch="conv", channels_last=False).eval()
    assert model.world_feat.encoder.layers[0].self_attn.head_dim == 4
    with torch.no_grad():
        want_shapes = [[o.shape for o in part] for part in other(imgs, M)]
    model.train()
    (heat, off), img_out = model(imgs, M)
    assert [[o.shape for o in part] for part in ((heat, off), img_out)] == want_shapes
    (heat.square().mean() + off.square().mean()).backward()
    for n, p in model.world_feat.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, n
    with pytest.raises(ValueError, match="'deform_trans', 'conv', 'deform_conv' or 'trans'"):
        build_model("mini", world_feat_arch="aio")


def test_abi_version_and_symbols():
    from mvdetr_amd import _lib
    assert _lib.ABI_VERSION == 18 and _lib.lib().mvdetr_ops_abi_version() == 18
    assert _lib.lib().mvdetr_attention_workspace_bytes(2, 8, 100, 50, 16, 4) == 2 * 8 * 100 * 4
    names = [n for n in _lib.SIGNATURES if "attention" in n]
    assert len(names) == 12 and np.all([hasattr(_lib.lib(), n) for n in names])
