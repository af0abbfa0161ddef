#!/usr/bin/env python3
"""int8 plans (Y3_DTYPE_I8) beside the 16-bit plans: throughput of the benchmark's step, per-conv times, one-image latency.

Throughput: the step bench.py times with --batch 128 --graph (forward_decode -> nms_padded -> pack_detections on a device-resident
batch, captured once, replayed) for THREE plans held in one process -- bf16 as shipped (fused stem), fp16 with the stem setting the
int8 plan has (one launch per conv unless --fused-stem: y3_net_set_stem_fusion_f16 acts on both alike) and int8 -- in alternated
windows; median of the window medians and the spread between a plan's own windows.  int8 against fp16 compares what is behind the cut:
before it both run the same launches.  --per-conv adds y3_net_profile_convs of fp16 and int8 side by side (each launch timed alone,
median of 9), so that a slower layer is named; the int8 copy of the tensor that crosses the cut is not a conv and shows in the step only.
Latency: one 416^2 image, the same step, graph replay, the three plans.

The activation scales are calibrated here on two seeded images (Net.calibrate_i8, absmax); the weights are the synthetic ones.

    python tools/time_i8.py [--batch 128] [--size 416] [--windows 3] [--replays 20] [--per-conv] [--fused-stem] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--windows", type=int, default=3, help="alternated windows per plan (at least three)")
    ap.add_argument("--replays", type=int, default=20, help="graph replays per window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--per-conv", action="store_true")
    ap.add_argument("--fused-stem", action="store_true", help="fp16 and int8 with the fused stem (set_stem_fusion_f16)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import yolo_v3_tf2_amd  # noqa: F401
    from yolo_v3_tf2_amd import _lib, runtime
    from yolo_v3_tf2_amd.core.utils import get_anchors
    from yolo_v3_tf2_amd.graph import load_program
    from yolo_v3_tf2_amd.weights import synthetic_weights

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    program = load_program(os.path.join(ROOT, "config/models/yolov3/model.yaml"), 80)
    weights = synthetic_weights(program, seed=4321)
    anchors = get_anchors(os.path.join(ROOT, "datasets/coco2012/anchors.txt")).astype(np.float32)
    say(f"# tools/time_i8.py  device: {torch.cuda.get_device_name(0)}")
    B, S = a.batch, a.size
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand((B, S, S, 3), device="cuda", generator=gen)

    cal = runtime.Net(program)
    cal.load_weights(weights)
    scales = cal.calibrate_i8(x[:2].contiguous())
    del cal
    torch.cuda.empty_cache()

    def make(dtype):
        net = runtime.Net(program)
        net.load_weights(weights)
        if dtype != _lib.Y3_DTYPE_BF16 and a.fused_stem:
            net.set_stem_fusion_f16(1)
        if dtype == _lib.Y3_DTYPE_I8:
            net.set_act_scales(scales)
        return net, dtype

    plans = {"bf16": make(_lib.Y3_DTYPE_BF16), "f16": make(_lib.Y3_DTYPE_F16), "i8": make(_lib.Y3_DTYPE_I8)}

    def timed(nb, windows, replays):
        xb = x[:nb].contiguous()
        graphs = {}
        for name, (net, dt) in plans.items():
            net.plan(nb, S, dt)

            def step(net=net):
                bb, cc, ss = net.forward_decode(xb, anchors)
                sel, nv = runtime.nms_padded(bb, ss, 100, 0.5, 0.1)
                return runtime.pack_detections(bb, cc, ss, sel, nv), nv
            for _ in range(a.warmup):
                step()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            for _ in range(a.warmup):
                g.replay()
            torch.cuda.synchronize()
            graphs[name] = g
        win = {k: [] for k in plans}
        for _ in range(max(3, windows)):
            for k, g in graphs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(replays):
                    g.replay()
                torch.cuda.synchronize()
                win[k].append((time.perf_counter() - t0) / replays * 1e3)
        return win

    say(f"\n== throughput: {B} x {S}^2, step = forward_decode + nms_padded + pack_detections, graph replay, {max(3, a.windows)} alternated windows of "
        f"{a.replays} replays per plan; fp16 / int8 stem {'fused' if a.fused_stem else 'one launch per conv'}")
    win = timed(B, a.windows, a.replays)
    say("int8 runs from conv %d on; lanes %s" % (plans["i8"][0].i8_first_conv(), ", ".join("%s %d" % (k, getattr(n, "lanes", 1)) for k, (n, _) in plans.items())))
    med = {}
    for k, v in win.items():
        med[k] = float(np.median(v))
        say(f"{k:5s} ms per step: windows {' '.join(f'{t:.3f}' for t in v)} | median {med[k]:.3f} | spread {max(v) - min(v):.3f} | {B / med[k] * 1e3:.0f} images/s")
    every = all(i < f for i, f in zip(win["i8"], win["f16"]))
    say(f"i8 / f16 {med['i8'] / med['f16']:.4f} (same launches before the cut); i8 / bf16 as shipped {med['i8'] / med['bf16']:.4f}; "
        f"int8 below fp16 in every window: {every}")
    if a.per_conv:
        ms = {k: np.median([plans[k][0].profile_convs(x) for _ in range(9)], axis=0) for k in ("f16", "i8")}
        cut = plans["i8"][0].i8_first_conv()
        say("-- per conv (each launch alone, median of 9): slot signature f16 ms, i8 ms, i8 / f16")
        for i, o in enumerate(plans["i8"][0].conv_ops):
            f, q = ms["f16"][i], ms["i8"][i]
            say(f"{i:4d}  {runtime.Net.conv_signature(o, S):36s} {f:8.4f} {q:8.4f}   {q / f if f > 0 else float('nan'):6.3f}{'   <- slower in int8' if i >= cut and q > f else ''}")
        say(f"sum   {'':36s} {ms['f16'].sum():8.4f} {ms['i8'].sum():8.4f}   {ms['i8'].sum() / ms['f16'].sum():6.3f}")
        say(f"behind the cut (convs {cut}..): f16 {ms['f16'][cut:].sum():.4f} ms, i8 {ms['i8'][cut:].sum():.4f} ms, ratio {ms['i8'][cut:].sum() / ms['f16'][cut:].sum():.3f}")
    say(f"\n== latency: 1 x {S}^2, the same step, graph replay, {max(3, a.windows)} alternated windows of {5 * a.replays} replays")
    win1 = timed(1, a.windows, 5 * a.replays)
    for k, v in win1.items():
        say(f"{k:5s} ms per image: windows {' '.join(f'{t:.4f}' for t in v)} | median {float(np.median(v)):.4f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
