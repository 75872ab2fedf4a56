"""Times the deform_conv ground-plane aggregator's deformable convolutions on the GPU: one 3x3 DeformConv2d(C, C, padding=1)
per camera (conv_world_feat.py:55-76), forward and backward, for the Wildtrack (7 x 128 x 120x360), MultiviewX
(6 x 128 x 160x250) and stress16 (16 x 256 x 120x360) world grids, against a torch composition on the same device:
9 x grid_sample(align_corners=True) im2col + matmul, fp32.

    python tools/deform_conv_bench.py [--iters N] [--configs wildtrack,multiviewx,stress16]

    python tools/deform_conv_bench.py --half-runs N      the 16-bit A/B only (below)

Prints one JSON line per (config, implementation) and a table.  Times are device-event times of whole frames (all cameras)
after warm-up; TF/s counts 2 * pixels * C_out * C_in * 9 FLOP per camera forward and twice that backward (g_col and grad_W)
against the 157.3 TF fp32 MFMA peak.

--half-runs N: at the Wildtrack frame, per 16-bit dtype, the forward of dc_fwd_mfma_half (channel-last 16-bit input, the
permuted weight cached as DeformConv2d caches it), of the fp32 dc_fwd_mfma on the same values (upcast once, outside the timing)
and of the upcast fallback (MVDETR_DEFORM_CONV_HALF=0: the four .float() casts, dc_fwd_mfma, one .to(dtype)); the three are
interleaved frame by frame in one session, each figure the median of 20 device-event frame times, N runs."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TF = 157.3
CONFIGS = {"wildtrack": (7, 128, 120, 360), "multiviewx": (6, 128, 160, 250), "stress16": (16, 256, 120, 360)}


def composition(x, off, w, b):
    """torch reference composition: the 9 taps' samples by grid_sample (pixel coordinates, align_corners=True, zeros) as an
    im2col tensor [B, C * 9, H * W], then one matmul."""
    B, C, H, W = x.shape
    Co = w.shape[0]
    ys = torch.arange(H, device=x.device, dtype=x.dtype).view(1, H, 1)
    xs = torch.arange(W, device=x.device, dtype=x.dtype).view(1, 1, W)
    cols = []
    for t in range(9):
        i, j = divmod(t, 3)
        y = ys - 1 + i + off[:, 2 * t]
        xx = xs - 1 + j + off[:, 2 * t + 1]
        grid = torch.stack((2 * xx / (W - 1) - 1, 2 * y / (H - 1) - 1), -1)
        cols.append(F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True))
    col = torch.stack(cols, 2).reshape(B, C * 9, H * W)
    return (w.reshape(Co, C * 9) @ col).view(B, Co, H, W) + b.view(1, Co, 1, 1)


def time_frame(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters                  # us per frame


def run(name, iters):
    from mvdetr_amd.ops import deform_conv
    N, C, H, W = CONFIGS[name]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    cams = []
    for _ in range(N):
        x = torch.randn(1, C, H, W, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        off = torch.randn(1, 18, H, W, generator=g).to(dev)                  # ~1 px, as the model's 1x1 conv produces
        w = (torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)).to(dev)
        b = (torch.randn(C, generator=g) * 0.1).to(dev)
        gout = torch.randn(1, C, H, W, generator=g).to(dev)
        cams.append([t.requires_grad_(True) if k < 4 else t for k, t in enumerate((x, off, w, b, gout))])
    flop_fwd = 2.0 * H * W * C * C * 9 * N
    rows = []
    impls = {"hip": lambda x, o, w, b: deform_conv.deform_conv2d(x, o, w, b, padding=1), "torch_composition": composition}
    # agreement of the two on camera 0
    with torch.no_grad():
        x, o, w, b, _ = cams[0]
        diff = (impls["hip"](x, o, w, b) - composition(x.contiguous(), o, w, b)).abs().max().item()
    for impl, fn in impls.items():
        def fwd():
            with torch.no_grad():
                for x, o, w, b, _ in cams:
                    fn(x, o, w, b)
        outs = [fn(x, o, w, b) for x, o, w, b, _ in cams]

        def bwd():
            for (x, o, w, b, gout), out in zip(cams, outs):
                torch.autograd.grad(out, (x, o, w, b), gout, retain_graph=True)
        t_f = time_frame(fwd, iters)
        t_b = time_frame(bwd, max(2, iters // 2))
        kern = (deform_conv.last_kernel() if impl == "hip" else "grid_sample+matmul")
        row = {"config": name, "impl": impl, "cameras": N, "channels": C, "grid": [H, W], "fwd_us_per_frame": round(t_f, 1),
               "bwd_us_per_frame": round(t_b, 1), "fwd_tflops": round(flop_fwd / t_f / 1e6, 2),
               "fwd_frac_of_peak": round(flop_fwd / t_f / 1e6 / PEAK_TF, 4),
               "bwd_tflops": round(2 * flop_fwd / t_b / 1e6, 2), "last_kernel": kern, "max_abs_diff_vs_composition": diff}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del outs
        torch.cuda.empty_cache()
    return rows


def half_ab(runs, frames=20):
    from mvdetr_amd.ops import deform_conv
    N, C, H, W = CONFIGS["wildtrack"]
    dev = torch.device("cuda:0")
    rows = []
    for dtype in (torch.float16, torch.bfloat16):
        g = torch.Generator().manual_seed(0)
        cams = []
        for _ in range(N):
            x = torch.randn(1, C, H, W, generator=g).to(dev, dtype).contiguous(memory_format=torch.channels_last)
            off = torch.randn(1, 18, H, W, generator=g).to(dev, dtype)
            w = (torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)).to(dev, dtype)
            b = (torch.randn(C, generator=g) * 0.1).to(dev, dtype)
            cams.append((x, off, w, b, deform_conv.permute_weight(w), [t.float() for t in (x, off, w, b)]))

        def half():
            for x, o, w, b, wt, _ in cams:
                deform_conv._deform_conv2d(x, o, w, b, 1, 1, 1, None, weight_t=wt)

        def fp32():
            for *_, f in cams:
                deform_conv.deform_conv2d(*f, padding=1)

        def upcast():
            os.environ["MVDETR_DEFORM_CONV_HALF"] = "0"
            for x, o, w, b, _, _ in cams:
                deform_conv.deform_conv2d(x, o, w, b, padding=1)
            del os.environ["MVDETR_DEFORM_CONV_HALF"]
        impls = {"dc_fwd_mfma_half": half, "dc_fwd_mfma_fp32_same_values": fp32, "upcast_fallback": upcast}
        routes = {}
        with torch.no_grad():
            for name, fn in impls.items():
                for _ in range(3):
                    fn()
                routes[name] = deform_conv.last_kernel()
            torch.cuda.synchronize()
            for run_ in range(runs):
                times = {k: [] for k in impls}
                for _ in range(frames):
                    for name, fn in impls.items():
                        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        start.record()
                        fn()
                        end.record()
                        end.synchronize()
                        times[name].append(start.elapsed_time(end) * 1e3)
                row = {"ab": "deform_conv_half", "dtype": str(dtype), "run": run_, "cameras": N, "channels": C, "grid": [H, W],
                       "median_of": frames, "last_kernel": routes}
                for name, ts in times.items():
                    row[name + "_us_per_frame"] = round(sorted(ts)[len(ts) // 2], 1)
                print(json.dumps(row), flush=True)
                rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--half-runs", type=int, default=0)
    ap.add_argument("--configs", default="wildtrack,multiviewx,stress16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("deform_conv_bench: needs a GPU (no CPU fallback for timings)")
    print(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {a.iters} frames per timing")
    if a.half_runs:
        half_ab(a.half_runs)
        return
    rows = []
    for name in a.configs.split(","):
        rows += run(name, a.iters)
    print(f"\n{'config':<11} {'impl':<18} {'fwd us/frame':>13} {'TF/s':>7} {'% peak':>7} {'bwd us/frame':>13} {'TF/s':>7}")
    for r in rows:
        print(f"{r['config']:<11} {r['impl']:<18} {r['fwd_us_per_frame']:>13.1f} {r['fwd_tflops']:>7.2f} "
              f"{100 * r['fwd_frac_of_peak']:>6.1f}% {r['bwd_us_per_frame']:>13.1f} {r['bwd_tflops']:>7.2f}")


if __name__ == "__main__":
    main()
