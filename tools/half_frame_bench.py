"""fp32 against 16-bit inference (MVDeTr.to_inference) at Wildtrack shape, in ONE process, the variants alternated
repetition by repetition (same call, alternating, spread first):

  detect          a whole frame, images -> ground-plane detections (MVDeTr.detect);
  hot_path        warp + shadow transformer on precomputed trunk features (MVDeTr.hot_path);
  warp            ops.warp_perspective alone, channel-last -> channel-last (warp_fwd_cl / warp_fwd_cl_half);
  msda            the fused deformable-attention forward alone on the encoder's input
                  (msda_fwd_group2 / msda_fwd_fused_half);
  add_layernorm   ops.add_layer_norm alone with the second output, 75,600 rows x 128;
  trans           a whole frame (MVDeTr.detect) of the ``trans`` world feature: the encoder's attention core is attn_fwd_mfma in
                  float32 and attn_fwd_mfma_half in 16 bits (models of its own, built only when the row is asked for);
  deform_conv     a whole frame (MVDeTr.detect) of the ``deform_conv`` world feature: the per-camera deformable convolutions
                  are dc_fwd_mfma in float32 and dc_fwd_mfma_half in 16 bits (models of its own, likewise);

each for float32, bfloat16 and float16; then, for each 16-bit variant,

  trunk           the whole 16-bit frame (MVDeTr.detect) with the trunk's fused epilogues on and off (ops.set_trunk_fusion),
                  alternated the same way; the baseline of this row is the variant with torch's ops;
  trunk_kernels   the four 16-bit epilogue kernels alone over the launches of one frame (bn_relu_half 8 launches,
                  bn_add_relu_half 5, bn_bn_add_relu_half 3, bn_relu_maxpool_half 1, every launch on tensors of its own):
                  bytes the pass must move (from the shapes) / device-event time.

`--only a,b` runs just those rows.

    python tools/half_frame_bench.py [--reps N] [--config wildtrack]

Clock: device events around the enqueued work, one repetition at a time.  Per row: median, the 10th and 90th percentile, min
and max of N repetitions after warm-up.  `spread` is the float32 variant's own p90 - p10 in that row; a 16-bit variant is
`faster` when its median is below float32's by more than that spread, `same` within it, `SLOWER` above it.  Also reports,
on one seeded frame, how many detections differ between float32 and each 16-bit run (information, not a bar: the weights
are seeded random, the threshold is set so that float32 keeps a few hundred candidates).  Prints one JSON line per row and
a table."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mvdetr_amd.model import build_model  # noqa: E402
from mvdetr_amd.ops import MultiScaleDeformableAttention as MSDA  # noqa: E402
from mvdetr_amd.ops import add_layer_norm, warp_perspective  # noqa: E402
from mvdetr_amd.ops import warp as warp_mod  # noqa: E402
from mvdetr_amd.ops import trunk_epilogue as te  # noqa: E402

DEV = "cuda:0"
VARIANTS = {"float32": None, "bfloat16": torch.bfloat16, "float16": torch.float16}


def perturb_sampling(model, std_px=1.5, seed=1234):
    """Seeded stand-in for learned sampling offsets / attention logits (the reference initialises both projections' weights
    to zero, which makes every query sample the same pattern): the benchmark's own recipe."""
    g = torch.Generator().manual_seed(seed)
    for layer in model.world_feat.encoder.layers:
        at = layer.self_attn
        with torch.no_grad():
            at.sampling_offsets.weight.copy_(torch.randn(at.sampling_offsets.weight.shape, generator=g) * (std_px / (1.4 * at.d_model ** 0.5)))
            at.attention_weights.weight.copy_(torch.randn(at.attention_weights.weight.shape, generator=g) * (1.0 / (1.4 * at.d_model ** 0.5)))


def alternated(fns, reps, warmup=3):
    """{variant: device-event times in us}, the variants taking turns inside every repetition."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in fns}
    for _ in range(reps):
        for n, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[n].append(a.elapsed_time(b) * 1e3)
    return times


def stats(t):
    s = sorted(t)
    pick = lambda q: s[min(len(s) - 1, int(q * (len(s) - 1) + 0.5))]  # noqa: E731
    return {"median_us": pick(0.5), "p10_us": pick(0.1), "p90_us": pick(0.9), "min_us": s[0], "max_us": s[-1]}


def detection_cells(model, imgs, M, thres):
    det = model.detect(imgs, M, cls_thres=thres)
    n = int(det.count[0])
    return set(det.cell[0, :min(n, det.cell.shape[1])].tolist())


ROWS = ("detect", "hot_path", "warp", "msda", "add_layernorm", "trans", "deform_conv", "trunk", "trunk_kernels", "detections")


def trunk_kernel_launches(views, feat_hw, dtype, device):
    """The fused 16-bit launches of one ResNet-18 frame, by kernel: name -> (closures, bytes the passes must move).  The
    stem's convolution output is 4 x 4 the feature map (stride 2 of the stride-8 trunk), layer1 runs at 2 x 2 of it, layers
    2 - 4 (dilated) at the feature map's size; 2 blocks per layer, a downsample branch in the first block of layers 2 - 4."""
    from torch import nn
    h, w = feat_hw

    def act(c, hh, ww):
        return torch.randn(views, c, hh, ww, device=device).to(dtype).contiguous(memory_format=torch.channels_last)

    def bn(c):
        # (mean 0, variance 1, gamma 1, beta 0: the passes run in place over and over, and their values must stay finite)
        return nn.BatchNorm2d(c).to(device).eval().requires_grad_(False)

    layers = [(64, 2 * h, 2 * w, False), (128, h, w, True), (256, h, w, True), (512, h, w, True)]
    out = {"bn_relu_half": ([], 0), "bn_add_relu_half": ([], 0), "bn_bn_add_relu_half": ([], 0), "bn_relu_maxpool_half": ([], 0)}

    def add(name, fn, nbytes):
        fns, total = out[name]
        out[name] = (fns + [fn], total + nbytes)

    stem = act(64, 4 * h, 4 * w)
    T = stem.numel() * stem.element_size()
    add("bn_relu_maxpool_half", lambda x=stem, m=bn(64): te.bn_relu_maxpool_half(x, m), T + T // 4)
    for c, hh, ww, down in layers:
        for block in range(2):
            x, m = act(c, hh, ww), bn(c)
            T = x.numel() * x.element_size()
            add("bn_relu_half", lambda x=x, m=m: te.bn_act_half(x, m, relu=True, inplace=True), 2 * T)
            x, r, m = act(c, hh, ww), act(c, hh, ww), bn(c)
            if down and block == 0:
                add("bn_bn_add_relu_half", lambda x=x, r=r, m=m, m2=bn(c): te.bn_act_half(x, m, r, m2, relu=True, inplace=True), 3 * T)
            else:
                add("bn_add_relu_half", lambda x=x, r=r, m=m: te.bn_act_half(x, m, r, relu=True, inplace=True), 3 * T)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--config", default="wildtrack")
    ap.add_argument("--only", default="", help="comma-separated rows to run (default: all): " + ", ".join(ROWS))
    a = ap.parse_args()
    only = set(filter(None, a.only.split(","))) or set(ROWS)
    if only - set(ROWS):
        raise SystemExit(f"half_frame_bench: unknown rows {sorted(only - set(ROWS))}")
    if not torch.cuda.is_available():
        raise SystemExit("half_frame_bench: needs a GPU (no CPU fallback for timings)")
    from helpers import fused_train_inputs
    print(f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; config {a.config}; {a.reps} alternated "
          f"repetitions per row, device events", flush=True)

    models = {}
    for name, dtype in VARIANTS.items():
        m = build_model(a.config, seed=0)
        perturb_sampling(m)
        m = m.to(DEV).eval()
        models[name] = m if dtype is None else m.to_inference(dtype)
    ref_model = models["float32"]
    # (the frame the trunk sees: the dataset resizes the camera image to input_img_shape -- bench.py's frame)
    N, (Hi, Wi), (H, W) = ref_model.num_cam, ref_model.geom.input_img_shape, ref_model.Rworld_shape
    imgs = torch.randn(1, N, 3, Hi, Wi, generator=torch.Generator().manual_seed(1000)).to(DEV)
    M = torch.eye(3).repeat(1, N, 1, 1)

    wf = ref_model.world_feat
    C, heads = wf.hidden_dim, 8
    h, w = H // wf.stride, W // wf.stride
    S = N * h * w
    value, shapes, lsi, ref_lm, raw, _ = [x.to(DEV) for x in fused_train_inputs(N, h, w, heads, C // heads, 4, seed=0)]
    g = torch.Generator().manual_seed(7)
    ln_x, ln_res, ln_pos = (torch.randn(b, S, C, generator=g).to(DEV) for b in (1, 1, 1))

    fns = {k: {} for k in ("detect", "hot_path", "warp", "msda", "add_layernorm")}
    kernels = {k: {} for k in fns}
    with torch.no_grad():
        for name, dtype in VARIANTS.items():
            model = models[name]
            feat = model.features(imgs)
            proj = model.frame_proj_mats(M, DEV)
            cast = (lambda t: t) if dtype is None else (lambda t, d=dtype: t.to(d))
            v_, raw_ = cast(value), cast(raw)
            x_, res_, pos_ = cast(ln_x), cast(ln_res), cast(ln_pos)
            norm = model.world_feat.encoder.layers[0].norm2
            fns["detect"][name] = lambda model=model: model.detect(imgs, M)
            fns["hot_path"][name] = lambda model=model, feat=feat, proj=proj: model.hot_path(feat, proj)
            fns["warp"][name] = lambda feat=feat, proj=proj: warp_perspective(feat, proj, (H, W), channels_last_out=True)
            if dtype is None:
                fns["msda"][name] = lambda v_=v_, raw_=raw_: MSDA.ms_deform_attn_forward_fused(
                    v_, shapes, lsi, ref_lm, None, None, raw=raw_, ref_level_major=True, raw_level_outer=True)
            else:
                fns["msda"][name] = lambda v_=v_, raw_=raw_: MSDA.ms_deform_attn_forward_fused_half(v_, shapes, lsi, ref_lm, raw_)
            fns["add_layernorm"][name] = lambda x_=x_, res_=res_, pos_=pos_, norm=norm: add_layer_norm(x_, res_, norm, then_add=pos_)
            # which kernels the variant runs (asked once, outside the timed window)
            fns["warp"][name]()
            kernels["warp"][name] = warp_mod.last_kernel()
            fns["msda"][name]()
            kernels["msda"][name] = MSDA.last_forward_kernel()
            fns["hot_path"][name]()
            kernels["hot_path"][name] = f"{warp_mod.last_kernel()} + {MSDA.last_forward_kernel()}"

        if "trans" in only:
            from mvdetr_amd.ops.attention import last_kernel as attn_last_kernel
            fns["trans"], kernels["trans"] = {}, {}
            for name, dtype in VARIANTS.items():
                m = build_model(a.config, seed=0, world_feat_arch="trans").to(DEV).eval()
                m = m if dtype is None else m.to_inference(dtype)
                fns["trans"][name] = lambda m=m: m.detect(imgs, M)
                fns["trans"][name]()
                kernels["trans"][name] = f"{warp_mod.last_kernel()} + {attn_last_kernel()}"

        if "deform_conv" in only:
            from mvdetr_amd.ops.deform_conv import last_kernel as dc_last_kernel
            fns["deform_conv"], kernels["deform_conv"] = {}, {}
            for name, dtype in VARIANTS.items():
                m = build_model(a.config, seed=0, world_feat_arch="deform_conv").to(DEV).eval()
                m = m if dtype is None else m.to_inference(dtype)
                fns["deform_conv"][name] = lambda m=m: m.detect(imgs, M)
                fns["deform_conv"][name]()
                kernels["deform_conv"][name] = f"{warp_mod.last_kernel()} + {dc_last_kernel()}"

        rows = []
        for what, variants in fns.items():
            if what not in only:
                continue
            res = {n: stats(t) for n, t in alternated(variants, a.reps).items()}
            base = res["float32"]
            spread = base["p90_us"] - base["p10_us"]
            for n, r in res.items():
                d = r["median_us"] - base["median_us"]
                verdict = "baseline" if n == "float32" else "faster" if -d > spread else "same" if d <= spread else "SLOWER"
                row = {"what": what, "variant": n, **{k: round(v, 1) for k, v in r.items()}, "fp32_spread_us": round(spread, 1),
                       "ratio_to_fp32": round(r["median_us"] / base["median_us"], 3), "verdict": verdict,
                       "kernel": kernels[what].get(n, "")}
                print(json.dumps(row), flush=True)
                rows.append(row)

        # the 16-bit frame with the trunk's fused epilogues on and off: the same model, the switch flipped inside the call
        def frame(model, fused):
            prev = te.set_trunk_fusion(fused)
            try:
                return model.detect(imgs, M)
            finally:
                te.set_trunk_fusion(prev)

        for n in ("bfloat16", "float16") if "trunk" in only else ():
            model = models[n]
            before = te.launch_count()
            frame(model, True)
            launches, kernel = te.launch_count() - before, te.last_kernel()
            frame(model, False)
            assert te.launch_count() == before + launches
            res = {k: stats(t) for k, t in alternated({"torch_ops": lambda model=model: frame(model, False),
                                                       "fused": lambda model=model: frame(model, True)}, a.reps).items()}
            base = res["torch_ops"]
            spread = base["p90_us"] - base["p10_us"]
            for k, r in res.items():
                d = r["median_us"] - base["median_us"]
                verdict = "baseline" if k == "torch_ops" else "faster" if -d > spread else "same" if d <= spread else "SLOWER"
                row = {"what": "trunk", "variant": f"{n}/{k}", **{q: round(v, 1) for q, v in r.items()}, "fp32_spread_us": round(spread, 1),
                       "ratio_to_fp32": round(r["median_us"] / base["median_us"], 3), "verdict": verdict,
                       "kernel": f"{launches} fused launches, last {kernel}" if k == "fused" else "torch's BatchNorm / ReLU / add / max-pool"}
                print(json.dumps(row), flush=True)
                rows.append(row)

        # the four 16-bit epilogue kernels alone, over one frame's launches
        kernel_rows = []
        for n in ("bfloat16", "float16") if "trunk_kernels" in only else ():
            h_feat, w_feat = models[n].features(imgs).shape[-2:]
            for kernel, (launches, nbytes) in trunk_kernel_launches(N, (h_feat, w_feat), VARIANTS[n], DEV).items():
                def once(launches=launches):
                    for fn in launches:
                        fn()
                once()
                assert te.last_kernel() == kernel, (te.last_kernel(), kernel)
                r = stats(alternated({kernel: once}, a.reps)[kernel])
                row = {"what": "trunk_kernels", "variant": n, "kernel": kernel, "launches": len(launches), "mbytes": round(nbytes / 1e6, 1),
                       **{q: round(v, 1) for q, v in r.items()}, "tbytes_per_s": round(nbytes / r["median_us"] / 1e6, 2)}
                print(json.dumps(row), flush=True)
                kernel_rows.append(row)

        # detections on one seeded frame: the threshold at which float32 keeps its 300 best-scoring cells as candidates
        (hm, _), _ = ref_model(imgs, M)
        thres = float(torch.sigmoid(hm.float()).flatten().topk(300).values[-1])
        cells = {n: detection_cells(m, imgs, M, thres) for n, m in models.items()} if "detections" in only else {}
        for n in ("bfloat16", "float16") if cells else ():
            row = {"what": "detections", "variant": n, "cls_thres": round(thres, 5), "kept_fp32": len(cells["float32"]),
                   "kept": len(cells[n]), "only_fp32": len(cells["float32"] - cells[n]), "only_16bit": len(cells[n] - cells["float32"])}
            print(json.dumps(row), flush=True)
            rows.append(row)

    print(f"\n{'what':<14} {'variant':<19} {'median us':>10} {'p10':>10} {'p90':>10} {'min':>10} {'max':>10} {'fp32 spread':>12} {'/ fp32':>7}  verdict   kernel")
    for r in rows:
        if r["what"] == "detections":
            print(f"{'detections':<14} {r['variant']:<19} kept by float32 {r['kept_fp32']}, by {r['variant']} {r['kept']}; only in float32 "
                  f"{r['only_fp32']}, only in {r['variant']} {r['only_16bit']} (cls_thres {r['cls_thres']})")
            continue
        print(f"{r['what']:<14} {r['variant']:<19} {r['median_us']:>10.1f} {r['p10_us']:>10.1f} {r['p90_us']:>10.1f} {r['min_us']:>10.1f} "
              f"{r['max_us']:>10.1f} {r['fp32_spread_us']:>12.1f} {r['ratio_to_fp32']:>7.3f}  {r['verdict']:<9} {r['kernel']}")
    if kernel_rows:
        print(f"\n{'kernel (one frame of launches)':<32} {'variant':<9} {'launches':>8} {'MB':>9} {'median us':>10} {'p10':>9} {'p90':>9} {'TB/s':>6}")
        for r in kernel_rows:
            print(f"{r['kernel']:<32} {r['variant']:<9} {r['launches']:>8} {r['mbytes']:>9.1f} {r['median_us']:>10.1f} {r['p10_us']:>9.1f} "
                  f"{r['p90_us']:>9.1f} {r['tbytes_per_s']:>6.2f}")


if __name__ == "__main__":
    main()
