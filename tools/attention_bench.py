"""Times the fused multi-head attention of the ``trans`` ground-plane aggregator on the GPU, per encoder layer, against what
torch runs for the same op, interleaved in one process:

  core       attention(q, k, v) forward and forward + backward vs (a) the ops nn.MultiheadAttention runs in fp32
             (bmm, softmax, bmm: the reference's op) and (b) F.scaled_dot_product_attention in fp32;
  module     ops.MultiheadAttention eval forward and training step vs nn.MultiheadAttention with the same weights, called
             as the reference calls it (need_weights left True: the weights are materialised and averaged) and with
             need_weights=False (torch then takes F.scaled_dot_product_attention);
  aggregator TransformerWorldFeat per frame (eval) and the peak memory of one training step vs the same module with
             nn.MultiheadAttention swapped in, both ways;
  core half  (--half-runs R: R runs of this row alone, nothing else) the 16-bit forward attn_fwd_mfma_half in bfloat16 and
             float16 on the head-split views of one seq-first packed [S, B, 3E] projection, with 64 and with 128 queries per
             workgroup and as the library picks, vs the fp32 attn_fwd_mfma on the same values, vs the upcast fallback
             (attention(q.float(), k.float(), v.float()).to(dtype)), vs what nn.MultiheadAttention runs in 16 bits
             (F.scaled_dot_product_attention with need_weights=False, bmm / softmax / bmm as the reference calls it).

    python tools/attention_bench.py [--reps N] [--sizes wildtrack,multiviewx,stress16,wildtrack_b4] [--half-runs R]

Every figure is the median of N (>= 20) device-event times after warm-up, with the spread (min .. max) beside it; the
implementations of one row are timed alternately, repetition by repetition.  TF/s counts 4 B H Sq Sk D FLOP forward and 2.5 x
that forward + backward, against the 157.3 TF fp32 MFMA peak.  Prints one JSON line per row and a table."""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TF = 157.3
# (B, heads, tokens, head dim): ground grid at 1/4 resolution, 8 heads
SIZES = {"wildtrack": (1, 8, 2700, 16), "multiviewx": (1, 8, 2520, 16), "stress16": (1, 8, 2700, 32), "wildtrack_b4": (4, 8, 2700, 16)}
GRIDS = {"wildtrack": (7, 128, 120, 360), "multiviewx": (6, 128, 160, 250)}


def interleaved(fns, reps, warmup=3):
    """{name: (median, min, max)} in us; the functions are run alternately so that clocks and caches treat them alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    times = {n: [] for n in fns}
    for _ in range(reps):
        for n, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[n].append(a.elapsed_time(b) * 1e3)
    return {n: (sorted(t)[len(t) // 2], min(t), max(t)) for n, t in times.items()}


def torch_composition(q, k, v):
    """What F.multi_head_attention_forward runs for fp32 without need_weights=False's SDPA shortcut: the reference's op."""
    B, H, S, D = q.shape
    q, k, v = (x.reshape(B * H, -1, D) for x in (q, k, v))
    return torch.bmm(torch.softmax(torch.bmm(q * (1.0 / math.sqrt(D)), k.transpose(1, 2)), -1), v).view(B, H, S, D)


def sdpa(q, k, v):
    return F.scaled_dot_product_attention(q, k, v)


def emit(rows, what, size, res, flop=None, extra=None):
    ours = res["hip"][0]
    for impl, (med, lo, hi) in res.items():
        row = {"what": what, "size": size, "impl": impl, "median_us": round(med, 1), "min_us": round(lo, 1), "max_us": round(hi, 1),
               "speedup_of_hip": round(med / ours, 2)}
        if flop:
            row["tflops"] = round(flop / med / 1e6, 2)
            row["frac_of_peak"] = round(flop / med / 1e6 / PEAK_TF, 4)
        row.update(extra or {})
        print(json.dumps(row), flush=True)
        rows.append(row)


def bench_core(name, reps, rows):
    from mvdetr_amd.ops import attention as attention_op
    from mvdetr_amd.ops.attention import last_kernel
    B, H, S, D = SIZES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, H, S, D, generator=g).to(dev).requires_grad_(True) for _ in range(3))
    gout = torch.randn(B, H, S, D, generator=g).to(dev)
    impls = {"hip": attention_op, "torch_bmm_softmax_bmm": torch_composition, "torch_sdpa": sdpa}
    with torch.no_grad():
        diff = (attention_op(q, k, v) - torch_composition(q, k, v)).abs().max().item()
        kern = last_kernel()

    def fwd(fn):
        def run():
            with torch.no_grad():
                fn(q, k, v)
        return run

    def fwd_bwd(fn):
        return lambda: torch.autograd.grad(fn(q, k, v), (q, k, v), gout)
    flop = 4.0 * B * H * S * S * D
    extra = {"kernel": kern, "max_abs_diff_vs_composition": diff}
    emit(rows, "core fwd", name, interleaved({n: fwd(f) for n, f in impls.items()}, reps), flop, extra)
    torch.autograd.grad(attention_op(q, k, v), (q, k, v), gout)
    extra = {"kernel": last_kernel()}
    emit(rows, "core fwd+bwd", name, interleaved({n: fwd_bwd(f) for n, f in impls.items()}, reps), 2.5 * flop, extra)


def bench_core_half(name, reps, rows, run):
    """The 16-bit forward at one size: every implementation on the same values, interleaved."""
    from mvdetr_amd.ops import attention as attention_op
    from mvdetr_amd.ops.attention import last_kernel, set_half_query_tile
    B, H, S, D = SIZES[name]
    E = H * D
    dev = torch.device("cuda:0")
    proj32 = torch.randn(S, B, 3 * E, generator=torch.Generator().manual_seed(0)).to(dev)

    def heads(proj):
        return [t.unflatten(-1, (H, D)).permute(1, 2, 0, 3) for t in proj.split(E, dim=-1)]

    def tiled(tile, qkv):
        def run_():
            set_half_query_tile(tile)
            attention_op(*qkv)
            set_half_query_tile(0)
        return run_
    flop = 4.0 * B * H * S * S * D
    with torch.no_grad():
        for dtype in (torch.bfloat16, torch.float16):
            proj = proj32.to(dtype)
            qkv = heads(proj)
            qkv32 = heads(proj.float())                      # the same values in fp32
            got = attention_op(*qkv)
            kern = last_kernel()
            diff = (got.float() - attention_op(*qkv32)).abs().max().item()
            fns = {"hip": lambda qkv=qkv: attention_op(*qkv), "hip_tq64": tiled(64, qkv), "hip_tq128": tiled(128, qkv),
                   "hip_fp32_same_values": lambda qkv32=qkv32: attention_op(*qkv32),
                   "hip_upcast_fallback": lambda qkv=qkv, dtype=dtype: attention_op(*(t.float() for t in qkv)).to(dtype),
                   "torch_sdpa_16bit": lambda qkv=qkv: sdpa(*qkv)}
            extra = {"kernel": kern, "dtype": str(dtype)[6:], "run": run, "max_abs_diff_vs_fp32_kernel": diff}
            emit(rows, f"core half fwd {str(dtype)[6:]}", name, interleaved(fns, reps), flop, extra)
            # a rotation of its own: the composition writes 2 x B H S S scores, and whatever runs after it starts on cold caches
            pair = {"hip": fns["hip"], "torch_bmm_softmax_bmm_16bit": lambda qkv=qkv: torch_composition(*qkv)}
            emit(rows, f"core half fwd {str(dtype)[6:]} (after the composition)", name, interleaved(pair, reps), flop, extra)


def bench_module(name, reps, rows):
    from mvdetr_amd.ops import MultiheadAttention
    B, H, S, D = SIZES[name]
    E = H * D
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ours = MultiheadAttention(E, H, dropout=0.1).to(dev)
    theirs = nn.MultiheadAttention(E, H, dropout=0.1).to(dev)
    theirs.load_state_dict(ours.state_dict())
    x = torch.randn(S, B, E, device=dev)
    pos = torch.randn(S, 1, E, device=dev)
    gout = torch.randn(S, B, E, device=dev)

    def fwd(m, need_weights=False):
        def run():
            with torch.no_grad():
                qk = x + pos
                m(qk, qk, x, need_weights=need_weights)
        return run

    def step(m, need_weights=False):
        def run():
            xs = x.detach().requires_grad_(True)
            qk = xs + pos
            m.zero_grad(set_to_none=True)
            m(qk, qk, xs, need_weights=need_weights)[0].backward(gout)
        return run
    ours.eval(), theirs.eval()
    emit(rows, "module eval fwd", name, interleaved({"hip": fwd(ours), REF_CALL: fwd(theirs, True), NO_WEIGHTS: fwd(theirs)}, reps))
    ours.train(), theirs.train()
    emit(rows, "module train step", name, interleaved({"hip": step(ours), REF_CALL: step(theirs, True), NO_WEIGHTS: step(theirs)}, reps))


REF_CALL, NO_WEIGHTS = "nn.MHA(reference call)", "nn.MHA(need_weights=False)"


class _ReferenceCall(nn.MultiheadAttention):
    """nn.MultiheadAttention as models/transformer.py:59 calls it: need_weights is left at its default, True."""

    def forward(self, *args, **kw):
        kw["need_weights"] = True
        return super().forward(*args, **kw)


def swap_in_torch_attention(model, cls):
    for layer in model.encoder.layers:
        theirs = cls(layer.self_attn.embed_dim, layer.self_attn.num_heads, dropout=layer.self_attn.dropout)
        theirs.load_state_dict(layer.self_attn.state_dict())
        layer.self_attn = theirs.to(next(layer.parameters()).device)
    return model


def bench_aggregator(name, reps, rows):
    import copy
    from mvdetr_amd.world_feat import TransformerWorldFeat
    N, C, H, W = GRIDS[name]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ours = TransformerWorldFeat(N, (H, W), C, hidden_dim=C).to(dev)
    impls = {"hip": ours, REF_CALL: swap_in_torch_attention(copy.deepcopy(ours), _ReferenceCall),
             NO_WEIGHTS: swap_in_torch_attention(copy.deepcopy(ours), nn.MultiheadAttention)}
    x = torch.randn(1, N, C, H, W, device=dev)

    def fwd(m):
        def run():
            with torch.no_grad():
                m(x)
        return run
    for m in impls.values():
        m.eval()
    emit(rows, "aggregator eval frame", name, interleaved({n: fwd(m) for n, m in impls.items()}, reps))
    if name == "wildtrack":
        peaks = {}
        for impl, m in impls.items():
            m.train()
            for _ in range(2):
                m.zero_grad(set_to_none=True)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                m(x).square().mean().backward()
                torch.cuda.synchronize()
                peaks[impl] = (torch.cuda.max_memory_allocated() - before) / 2 ** 20
        for impl, p in peaks.items():
            row = {"what": "aggregator train step peak memory", "size": name, "impl": impl, "peak_mib": round(p, 1)}
            print(json.dumps(row), flush=True)
            rows.append(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="wildtrack,multiviewx,stress16,wildtrack_b4")
    ap.add_argument("--half-runs", type=int, default=0, help="run only the 16-bit forward row, this many times")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attention_bench: needs a GPU (no CPU fallback for timings)")
    reps = max(20, a.reps)
    q = torch.randn(1, 8, 64, 16, device="cuda")
    backends = []
    import warnings
    from torch.nn.attention import SDPBackend, sdpa_kernel
    for b in ("FLASH_ATTENTION", "EFFICIENT_ATTENTION", "MATH"):
        try:
            with warnings.catch_warnings(), sdpa_kernel(getattr(SDPBackend, b)):
                warnings.simplefilter("ignore")
                F.scaled_dot_product_attention(q, q, q)
            backends.append(b)
        except RuntimeError:
            pass
    print(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median of {reps} interleaved repetitions (min .. max)")
    print(f"# F.scaled_dot_product_attention backends that accept fp32 here (torch picks among them): {backends}")
    rows = []
    for name in a.sizes.split(","):
        if a.half_runs:
            for run in range(a.half_runs):
                bench_core_half(name, reps, rows, run)
            continue
        bench_core(name, reps, rows)
        bench_module(name, reps, rows)
        if name in GRIDS:
            bench_aggregator(name, reps, rows)
        torch.cuda.empty_cache()
    print(f"\n{'what':<50} {'size':<13} {'impl':<27} {'median us':>10} {'min':>9} {'max':>9} {'TF/s':>7} {'% peak':>7} {'hip x':>6}")
    for r in rows:
        if "median_us" in r:
            tf = f"{r['tflops']:>7.2f} {100 * r['frac_of_peak']:>6.1f}%" if "tflops" in r else f"{'':>7} {'':>7}"
            print(f"{r['what']:<50} {r['size']:<13} {r['impl']:<27} {r['median_us']:>10.1f} {r['min_us']:>9.1f} {r['max_us']:>9.1f} "
                  f"{tf} {r['speedup_of_hip']:>6.2f}")
        else:
            print(f"{r['what']:<50} {r['size']:<13} {r['impl']:<27} {r['peak_mib']:>10.1f} MiB")


if __name__ == "__main__":
    main()
