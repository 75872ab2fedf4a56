"""The fp32 add + LayerNorm kernels (csrc/add_layernorm.hip) on the routes and edges tests/test_layernorm_gpu.py leaves out:
all four instantiations by name -- add_layernorm_rows<1> / <4> (64 / 256 columns), add_layernorm_rows128x2 (128 columns, 16-byte
aligned) and add_layernorm_rows<2> (128 columns, some pointer only 8-byte aligned) -- on five data families, odd row counts,
the grid-stride loop, rows that must not see their neighbours, constant rows and eps.  The oracle is fp64 layer_norm on the fp64
sum; unless a test compares bit patterns every comparison is the elementwise bar of tests/layernorm_oracle.py (K1 = 2, K2 = 4,
pinned on the CPU by tests/test_layernorm.py).  Every test asserts the kernel that ran."""
import itertools

import pytest
import torch

import layernorm_oracle as lo
from test_half_edges_gpu import at_offset

pytestmark = pytest.mark.gpu

# kernel -> (columns, offset of the inputs into their buffers in floats)
KERNELS = {"add_layernorm_rows<1>": (64, 0), "add_layernorm_rows128x2": (128, 0), "add_layernorm_rows<2>": (128, 2),
           "add_layernorm_rows<4>": (256, 0)}
NAN = float("nan")


def _ops():
    from mvdetr_amd.ops import add_layernorm
    return add_layernorm


def put(t, off):
    return None if t is None else (at_offset(t, off) if off else t.cuda())


def run(x, res, pos, w, b, eps, off=0, only=None):
    """add_layer_norm on CUDA copies of the arguments; with ``off`` the tensors named by ``only`` ("x", "res", "pos", "weight";
    None: all of them) start ``off`` floats into their buffers.  Returns (out, out2 or None, the kernel that ran)."""
    aln = _ops()
    shift = {k: off if only in (None, k) else 0 for k in ("x", "res", "pos", "weight")}
    norm = lo.make_norm(x.shape[-1], w, b, eps)
    if w is not None and shift["weight"]:
        norm.weight.data, norm.bias.data = at_offset(w, off), at_offset(b, off)
    with torch.no_grad():
        got = aln.add_layer_norm(put(x, shift["x"]), put(res, shift["res"]), norm, then_add=put(pos, shift["pos"]))
    got, got2 = got if pos is not None else (got, None)
    assert got.dtype == torch.float32 and got.shape == x.shape
    return got, got2, aln.last_kernel()


def entry(kernel, x, res, w, b, pos, eps):
    """The C entry itself on [rows, cols] inputs (``pos`` [add2_rows, cols]: any row count), the outputs placed inside
    NaN-filled buffers one row (and the kernel's offset) in: asserts the kernel name and that every word around the outputs
    is still NaN.  Returns (out, out2 or None)."""
    from mvdetr_amd import _lib
    cols, off = KERNELS[kernel]
    rows = x.shape[0]
    assert x.shape == (rows, cols) and (pos is None or pos.shape[1] == cols)
    dx, dr, dw, db, dp = (put(t, off) for t in (x, res, w, b, pos))
    lead, n = cols + off, rows * cols
    guards = [torch.full((lead + n + cols + 64,), NAN, device="cuda") for _ in range(1 if pos is None else 2)]
    outs = [g[lead:lead + n] for g in guards]
    ptr = lambda t: 0 if t is None else t.data_ptr()                                        # noqa: E731
    code = _lib.lib().mvdetr_add_layernorm_add_f32(
        _lib.current_stream_ptr(dx.device), ptr(dx), ptr(dr), ptr(dw), ptr(db), ptr(dp), 0 if pos is None else pos.shape[0],
        rows, cols, eps, outs[0].data_ptr(), outs[1].data_ptr() if pos is not None else 0)
    torch.cuda.synchronize()
    assert code == 0 and _ops().last_kernel() == kernel
    for g in guards:
        assert torch.isnan(g[:lead]).all() and torch.isnan(g[lead + n:]).all(), "a store outside the rows"
    outs = [o.view(rows, cols) for o in outs]
    return outs[0], (outs[1] if pos is not None else None)


def check(kernel, case, got, got2, y, bar, y2, bar2):
    r = lo.ratio(got, y, bar)
    r2 = lo.ratio(got2, y2, bar2) if y2 is not None else 0.0
    print(f"LNBAR {kernel} {case} out {r:.3f} out2 {r2:.3f}")
    assert r <= 1.0 and r2 <= 1.0, (kernel, case, r, r2)


# ---- a. every instantiation x every family ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(lo.FAMILIES))
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_every_kernel_every_family(kernel, name):
    """3 x 37 = 111 rows (an odd count), with and without residual, affine parameters and second output."""
    cols, off = KERNELS[kernel]
    x, res, pos, w, b, eps = lo.family(name, 3, 37, cols)
    for with_res, affine, with_add in itertools.product([True, False], repeat=3):
        args = (x, res if with_res else None, w if affine else None, b if affine else None, eps)
        p = pos if with_add else None
        got, got2, ran = run(args[0], args[1], p, *args[2:], off=off)
        assert ran == kernel
        check(kernel, f"{name}/res{with_res:d}_affine{affine:d}_add{with_add:d}", got, got2, *lo.oracle(*args, p))


# ---- b. alignment: add_layernorm_rows<2>, and what is refused -------------------------------------------------------------------
@pytest.mark.parametrize("only", [None, "x", "weight", "pos"])
def test_one_pointer_8_byte_aligned_takes_the_generic_128_column_kernel(only):
    x, res, pos, w, b, eps = lo.family("a", 3, 37, 128, seed=1)
    aligned = run(x, res, pos, w, b, eps)
    assert aligned[2] == "add_layernorm_rows128x2"
    got, got2, ran = run(x, res, pos, w, b, eps, off=2, only=only)
    assert ran == "add_layernorm_rows<2>"
    check(ran, f"a/offset2_{only or 'all'}", got, got2, *lo.oracle(x, res, w, b, eps, pos))


@pytest.mark.parametrize("cols,off", [(128, 1), (256, 1), (256, 2)])
def test_below_one_lanes_alignment_torch_runs_and_the_route_stays(cols, off):
    """Inputs below the alignment of a lane's cols / 64 floats: the C entry would refuse (801); add_layer_norm returns the
    module's own result, bit for bit, and no kernel of this family runs (a 64-column call before leaves its name)."""
    aln = _ops()
    x64, res64, pos64, w64, b64, eps64 = lo.family("a", 3, 37, 64, seed=2)
    got, got2, ran = run(x64, res64, pos64, w64, b64, eps64, off=1)                         # 64 columns: any float address
    assert ran == "add_layernorm_rows<1>"
    check(ran, "a/offset1", got, got2, *lo.oracle(x64, res64, w64, b64, eps64, pos64))
    x, res, pos, w, b, eps = lo.family("a", 3, 37, cols, seed=2)
    norm = lo.make_norm(cols, w, b, eps)
    for only in (None, "x", "res", "pos"):
        xo, ro, po = (at_offset(t, off if only in (None, k) else 0) for t, k in ((x, "x"), (res, "res"), (pos, "pos")))
        assert any(t.data_ptr() % (cols // 64 * 4) != 0 for t in (xo, ro, po))
        with torch.no_grad():
            got, got2 = aln.add_layer_norm(xo, ro, norm, then_add=po)
            want = norm(xo + ro)
            assert torch.equal(got, want) and torch.equal(got2, want + po)
        assert aln.last_kernel() == "add_layernorm_rows<1>"


# ---- c. odd row counts: the idle half wave of the two-row kernel, row pairs across batch elements ---------------------------------
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_odd_row_counts_write_their_rows_and_nothing_else(kernel):
    """Total rows 1, 3, 7, 9, 65 with a second addend of as many rows, and B = 3 batch elements of n = 1, 3, 37 rows sharing one
    element's addend (add2_rows = n: in the two-row kernel a wave's rows straddle batch elements, and the clamped row of the
    idle half wave is taken modulo n).  The outputs lie in NaN-filled buffers: nothing around them is written."""
    cols = KERNELS[kernel][0]
    for B, n in [(1, 1), (1, 3), (1, 7), (1, 9), (1, 65), (3, 1), (3, 3), (3, 37)]:
        x, res, pos, w, b, eps = lo.family("a", B, n, cols, seed=3)
        assert (B * n) % 2 == 1
        got, got2 = entry(kernel, x.view(-1, cols), res.view(-1, cols), w, b, pos.view(-1, cols), eps)
        check(kernel, f"a/rows{B}x{n}", got.view(x.shape), got2.view(x.shape), *lo.oracle(x, res, w, b, eps, pos))
        got, got2 = entry(kernel, x.view(-1, cols), None, None, None, None, eps)            # one output, no affine
        check(kernel, f"a/rows{B}x{n}_plain", got.view(x.shape), None, *lo.oracle(x, None, None, None, eps))


# ---- d. grid stride ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_grid_stride(kernel):
    """More rows than 4096 workgroups of four waves hold (one row per wave; two in add_layernorm_rows128x2), + 37: some waves
    run the loop twice, the last one stops short.  Through add_layer_norm with a second addend of all rows, and through the C
    entry with one of 1001 rows (rows of add2 repeat)."""
    cols, off = KERNELS[kernel]
    per_block = 8 if kernel == "add_layernorm_rows128x2" else 4
    rows = 4096 * per_block + 37
    assert -(-rows // per_block) > 4096 and -(-(rows - 37) // per_block) == 4096           # the launcher's block count, capped
    x, res, pos, w, b, eps = lo.family("a", 1, rows, cols, seed=4)
    y, bar, y2, bar2 = lo.oracle(x, res, w, b, eps, pos)
    got, got2, ran = run(x, res, pos, w, b, eps, off=off)
    assert ran == kernel
    check(kernel, f"a/rows{rows}", got, got2, y, bar, y2, bar2)
    del got, got2
    short = pos[0, :1001]
    y2 = y + short.double()[torch.arange(rows) % 1001]
    got, got2 = entry(kernel, x[0], res[0], w, b, short, eps)
    check(kernel, f"a/rows{rows}_add1001", got, got2, y[0], bar[0], y2[0], bar[0] + lo.U * y2[0].abs())


# ---- e. a row's result depends on that row alone ------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_rows_are_independent_bit_for_bit(kernel):
    """64 rows; the same rows in reversed order; every other row replaced; then a NaN, a +inf and a -inf in three rows that sit
    in different half waves and lanes (rows 5 and 23: upper half waves of the two-row kernel, row 40: a lower one).  A row's
    outputs are the same bits wherever it sits and whatever its neighbours hold; the poisoned rows are NaN throughout, as
    torch's are."""
    cols, off = KERNELS[kernel]
    x, res, pos, w, b, eps = lo.family("a", 1, 64, cols, seed=5)
    base, base2, ran = run(x, res, pos, w, b, eps, off=off)
    assert ran == kernel
    check(kernel, "a/rows64", base, base2, *lo.oracle(x, res, w, b, eps, pos))
    rev, rev2, ran = run(x.flip(1), res.flip(1), pos.flip(1), w, b, eps, off=off)
    assert ran == kernel and torch.equal(rev.flip(1), base) and torch.equal(rev2.flip(1), base2)
    other = lo.family("b", 1, 64, cols, seed=6)[0]
    x2 = x.clone()
    x2[:, 1::2] = other[:, 1::2]
    alt, alt2, ran = run(x2, res, pos, w, b, eps, off=off)
    assert ran == kernel and torch.equal(alt[:, 0::2], base[:, 0::2]) and torch.equal(alt2[:, 0::2], base2[:, 0::2])
    assert not torch.equal(alt[:, 1::2], base[:, 1::2])
    x3 = x.clone()
    x3[0, 5, 17], x3[0, 40, cols - 28], x3[0, 23, 3] = NAN, float("inf"), float("-inf")
    bad = torch.zeros(64, dtype=torch.bool)
    bad[[5, 23, 40]] = True
    got, got2, ran = run(x3, res, pos, w, b, eps, off=off)
    assert ran == kernel
    with torch.no_grad():
        theirs = lo.make_norm(cols, w, b, eps)(x3.cuda() + res.cuda())
    assert torch.isnan(theirs[0, bad]).all() and torch.isfinite(theirs[0, ~bad]).all()
    for o, clean in ((got, base), (got2, base2)):
        assert torch.isnan(o[0, bad]).all()
        assert torch.equal(o[0, ~bad], clean[0, ~bad])


# ---- f. constant rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_constant_rows_give_beta(kernel):
    """Rows of one value each (eighths below 16 plus sixteenths below 8: every partial sum of up to 256 of them is exact in
    fp32): the mean is exact, every centred element is exactly 0, so the output is beta bit for bit -- zero without affine
    parameters, whatever rsqrt(eps) is."""
    cols, off = KERNELS[kernel]
    g = torch.Generator().manual_seed(44)
    rows = 65
    x = (torch.randn(1, rows, 1, generator=g) * 24).round().div(8).clamp(-15, 15).expand(1, rows, cols).contiguous()
    res = (torch.randn(1, rows, 1, generator=g) * 8).round().div(16).clamp(-7, 7).expand(1, rows, cols).contiguous()
    assert x.abs().max() > 1 and torch.equal(x * 16, (x * 16).round()) and torch.equal(res * 16, (res * 16).round())
    w, b = lo.family("a", 1, 1, cols)[3:5]
    for r in (None, res):
        got, _, ran = run(x, r, None, w, b, 1e-5, off=off)
        assert ran == kernel
        assert torch.equal(got.cpu().view(torch.int32), b.expand(1, rows, cols).contiguous().view(torch.int32))
        for eps in (1e-12, 0.5):
            got, _, ran = run(x, r, None, None, None, eps, off=off)
            assert ran == kernel and (got == 0).all()


# ---- g. eps reaches the kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_eps_is_the_callers(kernel):
    """Rows of variance 2e-4 under eps 1e-12, 1e-5, 1e-3 and 0.5: four different results, each inside its own bar (an eps that
    arrived as another value, or not at all, is outside by orders of magnitude: tests/test_layernorm.py)."""
    cols, off = KERNELS[kernel]
    x, res, pos, w, b, _ = lo.family("c", 3, 37, cols, seed=7)
    outs = []
    for eps in (1e-12, 1e-5, 1e-3, 0.5):
        got, got2, ran = run(x, res, pos, w, b, eps, off=off)
        assert ran == kernel
        check(kernel, f"c/eps{eps:g}", got, got2, *lo.oracle(x, res, w, b, eps, pos))
        outs.append(got)
    for p, q in itertools.combinations(outs, 2):
        assert (p - q).abs().max().item() > 1e-3


# ---- the dispatcher: no host pointer reaches the kernel ---------------------------------------------------------------------------
def test_mixed_devices_and_dtypes_are_torchs_business(monkeypatch):
    """A CUDA x with a CPU residual, a CPU LayerNorm or a CPU then_add raises torch's RuntimeError, and an fp64 residual gives
    torch's fp64 result: the fp32 C entry is replaced by a spy, so nothing can be launched on a bad pointer."""
    from mvdetr_amd import _lib
    aln = _ops()
    calls = []

    def spy(*args):
        calls.append(args)
        pytest.fail("mvdetr_add_layernorm_add_f32 was called")

    monkeypatch.setattr(_lib.lib(), "mvdetr_add_layernorm_add_f32", spy)
    x, res, pos, w, b, eps = lo.family("a", 2, 5, 128, seed=8)
    norm = lo.make_norm(128, w, b, eps)
    with torch.no_grad():
        with pytest.raises(RuntimeError):
            aln.add_layer_norm(x.cuda(), res, norm)                                          # a CPU residual
        with pytest.raises(RuntimeError):
            aln.add_layer_norm(x.cuda(), res.cuda(), lo.make_norm(128, w, b, eps, device="cpu"))
        with pytest.raises(RuntimeError):
            aln.add_layer_norm(x.cuda(), None, lo.make_norm(128, w, b, eps, device="cpu"))
        with pytest.raises(RuntimeError):
            aln.add_layer_norm(x.cuda(), res.cuda(), norm, then_add=pos)                    # a CPU then_add
        plain = lo.make_norm(128, None, None, eps)
        got = aln.add_layer_norm(x.cuda(), res.double().cuda(), plain)                      # promoted, not rounded
        assert got.dtype == torch.float64 and torch.equal(got, plain(x.cuda() + res.double().cuda()))
        assert lo.ratio(got, *lo.oracle(x, res, None, None, eps)[:2]) < 1e-6
        try:                                                                                # with fp32 parameters: torch's call
            want = norm(x.cuda() + res.double().cuda())
        except RuntimeError:
            with pytest.raises(RuntimeError):
                aln.add_layer_norm(x.cuda(), res.double().cuda(), norm)
        else:
            got = aln.add_layer_norm(x.cuda(), res.double().cuda(), norm)
            assert got.dtype == want.dtype and torch.equal(got, want)
    assert calls == []
