"""The trunk's stride-1 3x3 convolutions at Wildtrack size (layer2-4: 7 x 90 x 160 pixels, layer1: 7 x 180 x 320; fp32,
channel-last): torch's
convolution (cudnn.benchmark = True, as bench.py sets: MIOpen picks by measurement) against the Winograd F(2x2,3x3)
MFMA kernel, interleaved in one process, HIP events.

    python tools/conv_bench.py [--reps 5] [--launches 20] [--out profiles/trunk_winograd_shapes.txt]
    python tools/conv_bench.py --epilogue [--out profiles/conv_winograd_epilogue_shapes.txt]
    python tools/conv_bench.py --tail [--out profiles/conv_winograd_w16_shapes.txt]
    python tools/conv_bench.py --variant
    python tools/conv_bench.py --schedule [--out profiles/conv_winograd_dephase_shapes.txt]
    python tools/conv_bench.py --backward [--out profiles/conv_winograd_backward_shapes.txt]

A repetition times `launches` back-to-back launches of one side, then of the other; a family is switched on in
mvdetr_amd/ops/conv_winograd.py only where the kernel is faster in EVERY repetition.  Also prints each shape's deviation
from an fp64 convolution for both sides (max-abs, on a post-ReLU N(0,1) input and kaiming weights).

--epilogue times the convolution WITH the block's epilogue, for every epilogue the trunk runs behind each shape, three sides
interleaved: (a) torch's convolution + bn_act in place, (b) the plain Winograd kernel + bn_act in place, (c) the Winograd
kernel with the epilogue in its store.  Besides the six layer3/4 shapes it times the two layer1/2 candidates at their own
sizes; the same rule decides about them: (c) faster than (a) in every repetition, for every epilogue.

--tail times the Winograd kernel against itself on the eight shapes, plain and with the first epilogue of each shape in its
store: the last round as whole units in the persistent kernel (tail mode 0) against half units in a second launch (mode 2),
interleaved.  A shape's tail is switched on (the tail flag of family_of in csrc/conv_winograd.hip) only where mode 2 is faster in every
repetition of every process run, on both rows.

--variant times the 4-wave persistent kernel (variant 1) against the 8-wave one on 16-channel wave blocks (variant 2) the same
way; the same rule sets the eight_wave flag.

--schedule times the 8-wave kernel against itself: all eight waves on one program (schedule 1, lockstep) against waves 4-7 on
a program of their own (schedule 2, de-phased), variant 2 and the default tail on both sides, interleaved; the same rule fills
the dephased flag.

--backward times the training pieces on the eight shapes, each against torch's convolution_backward (cudnn.benchmark) with the
matching output mask, interleaved: the data gradient alone (the forward kernel on Ut), the weight gradient alone
(conv3x3_winograd_wgrad_f32 and its reduction), and forward + backward together through winograd_conv3x3_train against
torch's conv + autograd.  A piece of a family goes into TRAIN_FAMILIES only where it is faster in every repetition."""
import argparse
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [  # name, C, K, dilation, pixels (None: --pixels)
    ("layer3.0.conv1", 128, 256, 1, None), ("layer3.x.conv2", 256, 256, 1, None), ("layer3.1.conv1", 256, 256, 2, None),
    ("layer4.0.conv1", 256, 512, 2, None), ("layer4.x.conv2", 512, 512, 1, None), ("layer4.1.conv1", 512, 512, 4, None),
    ("layer1.x.conv1/2", 64, 64, 1, (7, 180, 320)), ("layer2.x.conv1/2", 128, 128, 1, (7, 90, 160)),
]

# --epilogue: name, C, K, dilation, the epilogues the trunk runs behind it, pixels (None: --pixels)
EPILOGUE_SHAPES = [
    ("layer3.0.conv1", 128, 256, 1, ("bn",), None), ("layer3.x.conv2", 256, 256, 1, ("bn_add", "bn_bn_add"), None),
    ("layer3.1.conv1", 256, 256, 2, ("bn",), None), ("layer4.0.conv1", 256, 512, 2, ("bn",), None),
    ("layer4.x.conv2", 512, 512, 1, ("bn_add", "bn_bn_add"), None), ("layer4.1.conv1", 512, 512, 4, ("bn",), None),
    ("layer1.x.conv1/2", 64, 64, 1, ("bn", "bn_add"), (7, 180, 320)),
    ("layer2.x.conv1/2", 128, 128, 1, ("bn", "bn_add", "bn_bn_add"), (7, 90, 160)),
]


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def _bn(K, dev):
    bn = nn.BatchNorm2d(K)
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.3)
        bn.running_var.uniform_(0.5, 1.5)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.3)
    return bn.to(dev).eval()


def epilogue_table(args, dev):
    from mvdetr_amd.ops import conv_winograd as cw
    from mvdetr_amd.ops.trunk_epilogue import bn_act
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    lines = [f"# convolution + epilogue (relu on), fp32 channel-last, ms over {args.launches} launches, {args.reps} interleaved "
             "repetitions: (a) torch's convolution (MIOpen, cudnn.benchmark) + bn_act in place, (b) conv3x3_winograd_f32 + bn_act "
             "in place, (c) conv3x3_winograd_f32 with the epilogue in its store",
             "# shape               C->K     d  pixels       epilogue    (a) min/med/max          (b) min/med/max          "
             "(c) min/med/max          c<b   c<a   c == b"]
    for name, C, K, d, modes, pixels in EPILOGUE_SHAPES:
        N, H, W = pixels or args.pixels
        torch.manual_seed(C + K + d)
        conv = nn.Conv2d(C, K, 3, 1, d, d, bias=False)
        nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
        conv = conv.to(dev).to(memory_format=torch.channels_last).eval()
        x = torch.randn(N, C, H, W, device=dev).relu_().contiguous(memory_format=torch.channels_last)
        bn, bn2 = _bn(K, dev), _bn(K, dev)
        res = torch.randn(N, K, H, W, device=dev).contiguous(memory_format=torch.channels_last)
        for mode in modes:
            r, rbn = (None if mode == "bn" else res), (bn2 if mode == "bn_bn_add" else None)
            side_a = lambda: bn_act(conv(x), bn, r, rbn, relu=True, inplace=True)  # noqa: E731
            side_b = lambda: bn_act(cw.winograd_conv3x3(x, conv, force=True), bn, r, rbn, relu=True, inplace=True)  # noqa: E731
            side_c = lambda: cw.winograd_conv3x3_bn_act(x, conv, bn, r, rbn, relu=True, force=True)  # noqa: E731
            with torch.no_grad():
                for _ in range(3):
                    side_a()
                    same = torch.equal(side_b(), side_c())
                t = [[], [], []]
                for _ in range(args.reps):
                    for side, fn in zip(t, (side_a, side_b, side_c)):
                        side.append(timed(fn, args.launches))
            cols = "     ".join(f"{min(v):6.3f} {med(v):6.3f} {max(v):6.3f}" for v in t)
            lines.append(f"{name:<20} {C:>4}->{K:<4} {d}  {N}x{H}x{W:<5} {mode + '_relu':<15} {cols}     "
                         f"{sum(c < b for c, b in zip(t[2], t[1]))}/{args.reps}   {sum(c < a for c, a in zip(t[2], t[0]))}/{args.reps}   "
                         f"{same}")
            print(lines[-1], flush=True)
    return lines


def tail_table(args, dev):
    from mvdetr_amd.ops import conv_winograd as cw
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    lines = [f"# conv3x3_winograd_f32, last round as whole units (tail 0) vs as half units in a second launch (tail 2), fp32 "
             f"channel-last, ms per convolution over {args.launches} launches, {args.reps} interleaved repetitions, {cus} CUs; "
             "h = the half-unit launch's time in unit times, from the two medians and the fit (see --help)",
             "# shape               C->K     d  pixels       store           units   R  rem   tail 0 min/med/max       "
             "tail 2 min/med/max       wins   gain us   equal"]
    for name, C, K, d, modes, pixels in EPILOGUE_SHAPES:
        N, H, W = pixels or args.pixels
        torch.manual_seed(C + K + d)
        conv = nn.Conv2d(C, K, 3, 1, d, d, bias=False)
        nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
        conv = conv.to(dev).to(memory_format=torch.channels_last).eval()
        x = torch.randn(N, C, H, W, device=dev).relu_().contiguous(memory_format=torch.channels_last)
        bn, bn2 = _bn(K, dev), _bn(K, dev)
        res = torch.randn(N, K, H, W, device=dev).contiguous(memory_format=torch.channels_last)
        cw.set_winograd_tail(2)
        p = cw.plan(N, H, W, C, K, d, cus)
        for mode in ("none", modes[0]):
            r, rbn = (None if mode in ("none", "bn") else res), (bn2 if mode == "bn_bn_add" else None)
            if mode == "none":
                fn = lambda: cw.winograd_conv3x3(x, conv, force=True)  # noqa: E731
            else:
                fn = lambda: cw.winograd_conv3x3_bn_act(x, conv, bn, r, rbn, relu=True, force=True)  # noqa: E731
            t = [[], []]
            with torch.no_grad():
                outs = []
                for tail in (0, 2):
                    cw.set_winograd_tail(tail)
                    for _ in range(3):
                        y = fn()
                    outs.append(y)
                same = torch.equal(*outs)
                for _ in range(args.reps):
                    for side, tail in zip(t, (0, 2)):
                        cw.set_winograd_tail(tail)
                        side.append(timed(fn, args.launches))
            cw.set_winograd_tail(1)
            cols = "     ".join(f"{min(v):6.3f} {med(v):6.3f} {max(v):6.3f}" for v in t)
            lines.append(f"{name:<20} {C:>4}->{K:<4} {d}  {N}x{H}x{W:<5} {(mode + '_relu') if mode != 'none' else 'plain':<15} "
                         f"{p['units']:>5} {p['R']:>3} {p['rem']:>4}   {cols}     {sum(b < a for a, b in zip(*t))}/{args.reps}   "
                         f"{(med(t[0]) - med(t[1])) * 1e3:7.1f}   {same}")
            print(lines[-1], flush=True)
    return lines


def variant_table(args, dev):
    """--variant: the 4-wave persistent kernel (variant 1) against the 8-wave one (variant 2), the tail in its default mode on
    both sides, plain store and the shape's first fused store, interleaved."""
    from mvdetr_amd.ops import conv_winograd as cw
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    lines = [f"# conv3x3_winograd_f32 (variant 1: 4 waves, 32-channel wave blocks) vs conv3x3_winograd_w16x2_f32 (variant 2: 8 waves, "
             f"16-channel wave blocks), default tail on both, fp32 channel-last, ms per convolution over {args.launches} launches, "
             f"{args.reps} interleaved repetitions",
             "# shape               C->K     d  pixels       store           variant 1 min/med/max    variant 2 min/med/max    "
             "wins   gain us   equal"]
    for name, C, K, d, modes, pixels in EPILOGUE_SHAPES:
        N, H, W = pixels or args.pixels
        torch.manual_seed(C + K + d)
        conv = nn.Conv2d(C, K, 3, 1, d, d, bias=False)
        nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
        conv = conv.to(dev).to(memory_format=torch.channels_last).eval()
        x = torch.randn(N, C, H, W, device=dev).relu_().contiguous(memory_format=torch.channels_last)
        bn, bn2 = _bn(K, dev), _bn(K, dev)
        res = torch.randn(N, K, H, W, device=dev).contiguous(memory_format=torch.channels_last)
        for mode in ("none", modes[0]):
            r, rbn = (None if mode in ("none", "bn") else res), (bn2 if mode == "bn_bn_add" else None)
            if mode == "none":
                fn = lambda: cw.winograd_conv3x3(x, conv, force=True)  # noqa: E731
            else:
                fn = lambda: cw.winograd_conv3x3_bn_act(x, conv, bn, r, rbn, relu=True, force=True)  # noqa: E731
            t = [[], []]
            with torch.no_grad():
                outs = []
                for variant in (1, 2):
                    cw.set_winograd_variant(variant)
                    for _ in range(3):
                        y = fn()
                    outs.append(y)
                same = torch.equal(*outs)
                for _ in range(args.reps):
                    for side, variant in zip(t, (1, 2)):
                        cw.set_winograd_variant(variant)
                        side.append(timed(fn, args.launches))
            cw.set_winograd_variant(0)
            cols = "     ".join(f"{min(v):6.3f} {med(v):6.3f} {max(v):6.3f}" for v in t)
            lines.append(f"{name:<20} {C:>4}->{K:<4} {d}  {N}x{H}x{W:<5} {(mode + '_relu') if mode != 'none' else 'plain':<15} "
                         f"{cols}     {sum(b < a for a, b in zip(*t))}/{args.reps}   {(med(t[0]) - med(t[1])) * 1e3:7.1f}   {same}")
            print(lines[-1], flush=True)
    return lines


def schedule_table(args, dev):
    """--schedule: the 8-wave kernel in lockstep (schedule 1) against the de-phased schedule (2), plain store and the shape's
    first fused store, interleaved."""
    from mvdetr_amd.ops import conv_winograd as cw
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    lines = [f"# conv3x3_winograd_w16x2_f32 (variant 2 on every shape), schedule 1 (lockstep) vs schedule 2 (de-phased), default tail "
             f"on both, fp32 channel-last, ms per convolution over {args.launches} launches, {args.reps} interleaved repetitions",
             "# shape               C->K     d  pixels       store           schedule 1 min/med/max   schedule 2 min/med/max    "
             "wins   gain us   equal"]
    for name, C, K, d, modes, pixels in EPILOGUE_SHAPES:
        N, H, W = pixels or args.pixels
        torch.manual_seed(C + K + d)
        conv = nn.Conv2d(C, K, 3, 1, d, d, bias=False)
        nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
        conv = conv.to(dev).to(memory_format=torch.channels_last).eval()
        x = torch.randn(N, C, H, W, device=dev).relu_().contiguous(memory_format=torch.channels_last)
        bn, bn2 = _bn(K, dev), _bn(K, dev)
        res = torch.randn(N, K, H, W, device=dev).contiguous(memory_format=torch.channels_last)
        cw.set_winograd_variant(2)
        for mode in ("none", modes[0]):
            r, rbn = (None if mode in ("none", "bn") else res), (bn2 if mode == "bn_bn_add" else None)
            if mode == "none":
                fn = lambda: cw.winograd_conv3x3(x, conv, force=True)  # noqa: E731
            else:
                fn = lambda: cw.winograd_conv3x3_bn_act(x, conv, bn, r, rbn, relu=True, force=True)  # noqa: E731
            t = [[], []]
            with torch.no_grad():
                outs = []
                for sch in (1, 2):
                    cw.set_winograd_schedule(sch)
                    for _ in range(3):
                        y = fn()
                    assert cw.last_schedule() == sch and cw.last_variant() == 2
                    outs.append(y)
                same = torch.equal(*outs)
                for _ in range(args.reps):
                    for side, sch in zip(t, (1, 2)):
                        cw.set_winograd_schedule(sch)
                        side.append(timed(fn, args.launches))
            cw.set_winograd_schedule(0)
            cols = "     ".join(f"{min(v):6.3f} {med(v):6.3f} {max(v):6.3f}" for v in t)
            lines.append(f"{name:<20} {C:>4}->{K:<4} {d}  {N}x{H}x{W:<5} {(mode + '_relu') if mode != 'none' else 'plain':<15} "
                         f"{cols}     {sum(b < a for a, b in zip(*t))}/{args.reps}   {(med(t[0]) - med(t[1])) * 1e3:7.1f}   {same}")
            print(lines[-1], flush=True)
        cw.set_winograd_variant(0)
    return lines


def backward_table(args, dev):
    """--backward: dgrad alone, wgrad alone, forward + backward together; Winograd against torch, interleaved."""
    from mvdetr_amd.ops import conv_winograd as cw
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    lines = [f"# the training pieces of a 3x3 convolution, fp32 channel-last, ms over {args.launches} launches, {args.reps} interleaved "
             f"repetitions, {cus} CUs: torch = aten.convolution_backward with the piece's output mask (MIOpen, cudnn.benchmark); "
             "winograd = dgrad: conv3x3_winograd_f32 on Ut, wgrad: conv3x3_winograd_wgrad_f32 + its reduction (S splits), "
             "fwd+bwd: winograd_conv3x3_train(force) + autograd against conv(x) + autograd, both gradients; err = max-abs "
             "deviation from fp64 on the first image's worth of grad_x / on grad_w",
             "# shape               C->K     d  pixels       piece     S   torch min/med/max        winograd min/med/max     "
             "wins  err torch / winograd vs fp64"]
    for name, C, K, d, pixels in SHAPES:
        N, H, W = pixels or args.pixels
        torch.manual_seed(C + K + d)
        conv = nn.Conv2d(C, K, 3, 1, d, d, bias=False)
        nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
        conv = conv.to(dev).to(memory_format=torch.channels_last)
        w = conv.weight.detach()
        x = torch.randn(N, C, H, W, device=dev).relu_().contiguous(memory_format=torch.channels_last)
        gy = torch.randn(N, K, H, W, device=dev).contiguous(memory_format=torch.channels_last)
        xg = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
        back = lambda mask: torch.ops.aten.convolution_backward(gy, x, w, None, (1, 1), (d, d), (d, d), False, (0, 0), 1, mask)  # noqa: E731
        sides = {
            "dgrad": (lambda: back([True, False, False])[0], lambda: cw.winograd_conv3x3_input_grad(gy, w, d)),
            "wgrad": (lambda: back([False, True, False])[1], lambda: cw.winograd_conv3x3_weight_grad(x, gy, d)),
            "fwd+bwd": (lambda: torch.autograd.grad(conv(xg), (xg, conv.weight), gy),
                        lambda: torch.autograd.grad(cw.winograd_conv3x3_train(xg, conv, force=True), (xg, conv.weight), gy)),
        }
        S = cw.wgrad_plan(N, H, W, C, K, d, cus)["S"]
        want_x = torch.nn.grad.conv2d_input((1, C, H, W), w.double(), gy[:1].double(), 1, d, d)
        want_w = torch.nn.grad.conv2d_weight(x.double(), w.shape, gy.double(), 1, d, d)
        for piece, (torch_side, wino_side) in sides.items():
            for _ in range(3):
                ref, got = torch_side(), wino_side()
            if piece == "dgrad":
                err = f"{(ref[:1] - want_x).abs().max().item():.2e} / {(got[:1] - want_x).abs().max().item():.2e}"
            elif piece == "wgrad":
                err = f"{(ref - want_w).abs().max().item():.2e} / {(got - want_w).abs().max().item():.2e}"
            else:
                err = "-"
            t_t, t_w = [], []
            for _ in range(args.reps):
                t_t.append(timed(torch_side, args.launches))
                t_w.append(timed(wino_side, args.launches))
            wins = sum(a < b for a, b in zip(t_w, t_t))
            lines.append(f"{name:<20} {C:>4}->{K:<4} {d}  {N}x{H}x{W:<5} {piece:<8} {S:>3}   {min(t_t):6.3f} {med(t_t):6.3f} {max(t_t):6.3f}     "
                         f"{min(t_w):6.3f} {med(t_w):6.3f} {max(t_w):6.3f}     {wins}/{args.reps}   {err}")
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--pixels", type=int, nargs=3, default=(7, 90, 160), metavar=("N", "H", "W"))
    ap.add_argument("--out")
    ap.add_argument("--epilogue", action="store_true", help="time the convolutions with their epilogues, three sides")
    ap.add_argument("--tail", action="store_true", help="time the last round as whole units against half units")
    ap.add_argument("--variant", action="store_true", help="time the 4-wave persistent kernel against the 8-wave one")
    ap.add_argument("--schedule", action="store_true", help="time the 8-wave kernel in lockstep against the de-phased schedule")
    ap.add_argument("--backward", action="store_true", help="time the data gradient, the weight gradient and forward + backward")
    args = ap.parse_args()
    from mvdetr_amd.ops import conv_winograd as cw
    torch.backends.cudnn.benchmark = True
    dev = torch.device("cuda:0")
    N, H, W = args.pixels
    shapes = SHAPES
    if args.epilogue:
        lines, shapes = epilogue_table(args, dev), []
    elif args.tail:
        lines, shapes = tail_table(args, dev), []
    elif args.variant:
        lines, shapes = variant_table(args, dev), []
    elif args.schedule:
        lines, shapes = schedule_table(args, dev), []
    elif args.backward:
        lines, shapes = backward_table(args, dev), []
    else:
        lines = [f"# torch (MIOpen, cudnn.benchmark) vs conv3x3_winograd_f32, fp32 channel-last, ms per launch "
                 f"over {args.launches} launches, {args.reps} interleaved repetitions; GFLOP = direct form",
                 "# shape               C->K     d  pixels       GFLOP   torch min/med/max        winograd min/med/max     TF/s(direct-equivalent)  "
                 "wins  err torch / winograd vs fp64"]
    for name, C, K, d, pixels in shapes:
        N, H, W = pixels or args.pixels
        torch.manual_seed(C + K + d)
        conv = nn.Conv2d(C, K, 3, 1, d, d, bias=False)
        nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
        conv = conv.to(dev).to(memory_format=torch.channels_last).eval()
        x = torch.randn(N, C, H, W, device=dev).relu_().contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            for _ in range(3):
                ref32, got = conv(x), cw.winograd_conv3x3(x, conv, force=True)
            sub = slice(0, 1)
            want = nn.functional.conv2d(x[sub].double(), conv.weight.double(), None, 1, d, d)
            e_t, e_w = (ref32[sub] - want).abs().max().item(), (got[sub] - want).abs().max().item()
            t_t, t_w = [], []
            for _ in range(args.reps):
                t_t.append(timed(lambda: conv(x), args.launches))
                t_w.append(timed(lambda: cw.winograd_conv3x3(x, conv, force=True), args.launches))
        gflop = 2.0 * N * H * W * C * K * 9 / 1e9
        wins = sum(w < t for w, t in zip(t_w, t_t))
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        lines.append(f"{name:<20} {C:>4}->{K:<4} {d}  {N}x{H}x{W:<5} {gflop:6.1f}  {min(t_t):6.3f} {med(t_t):6.3f} {max(t_t):6.3f}     "
                     f"{min(t_w):6.3f} {med(t_w):6.3f} {max(t_w):6.3f}     {gflop / med(t_w):7.1f}                  {wins}/{args.reps}   "
                     f"{e_t:.2e} / {e_w:.2e}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
