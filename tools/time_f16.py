#!/usr/bin/env python3
"""fp16 plans (Y3_DTYPE_F16) beside bf16 plans: throughput of the benchmark's step, and precision on the device.

Throughput: the step bench.py times with --dtype bf16 --batch 128 --graph (forward_decode -> nms_padded -> pack_detections on a device-
resident batch, captured once, replayed) for FOUR plans held in one process -- bf16 as shipped (fused stem), bf16 with the stem
unfused (set_stem_fusion(0)), fp16 as shipped (no fused stem) and fp16 with the fused stem (set_stem_fusion_f16) -- in alternated
windows; median of the window medians and the spread between a plan's own windows.  fp16 against bf16-unfused compares the kernels
(both run the same launches, same tiles, same lanes); fp16 with the fused stem against fp16 is what the switch returns, beside what the
fused stem is worth to bf16.  --per-conv adds y3_net_profile_convs of the four plans (each launch timed alone, median of 9; the convs
inside a fused stem show 0 and their time is conv 1's).

Precision (--precision): girl.png at 416^2 through forward_decode on a bf16 and on an fp16 plan against the fp32 oracle's decode:
largest deviation of a box coordinate and of a score, over all candidates and over those the oracle scores above 0.1.

--zeros repeats the throughput part on all-zero weights and images (no data toggling: what of a difference is power).

    python tools/time_f16.py [--batch 128] [--size 416] [--windows 3] [--replays 20] [--per-conv] [--precision] [--zeros] [--out FILE]"""
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
    ap.add_argument("--precision", action="store_true")
    ap.add_argument("--no-throughput", action="store_true")
    ap.add_argument("--zeros", action="store_true", help="throughput on all-zero weights and images: the same launches with no data toggling in the "
                                                         "matrix pipes (what of a difference between the formats is power, as tools/ab_libs.py --data zeros)")
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
    if a.zeros:
        weights = {k: (v if k.endswith(".var") else v * 0) for k, v in weights.items()}
    anchors = get_anchors(os.path.join(ROOT, "datasets/coco2012/anchors.txt")).astype(np.float32)
    say(f"# tools/time_f16.py  device: {torch.cuda.get_device_name(0)}")

    def make(dtype, stem, stem_f16=None):
        net = runtime.Net(program)
        net.load_weights(weights)
        if stem is not None:
            net.set_stem_fusion(stem)
        if stem_f16 is not None:
            net.set_stem_fusion_f16(stem_f16)
        return net, dtype

    if not a.no_throughput:
        B, S = a.batch, a.size
        plans = {"bf16": make(_lib.Y3_DTYPE_BF16, None), "bf16-unfused-stem": make(_lib.Y3_DTYPE_BF16, 0), "f16": make(_lib.Y3_DTYPE_F16, None),
                 "f16-fused-stem": make(_lib.Y3_DTYPE_F16, None, 1)}
        x = torch.rand((B, S, S, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
        if a.zeros:
            x.zero_()
        graphs = {}
        for name, (net, dt) in plans.items():
            net.plan(B, S, dt)

            def step(net=net):
                bb, cc, ss = net.forward_decode(x, anchors)
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
        lanes = ", ".join("%s %d" % (k, getattr(n, "lanes", 1)) for k, (n, _) in plans.items())
        say(f"\n== throughput{' (ALL-ZERO weights and images)' if a.zeros else ''}: {B} x {S}^2, step = forward_decode + nms_padded + pack_detections, graph replay, {a.windows} alternated windows of "
            f"{a.replays} replays per plan; lanes {lanes}")
        win = {k: [] for k in plans}
        for _ in range(max(3, a.windows)):
            for k, g in graphs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.replays):
                    g.replay()
                torch.cuda.synchronize()
                win[k].append((time.perf_counter() - t0) / a.replays * 1e3)
        med = {}
        for k, v in win.items():
            med[k] = float(np.median(v))
            say(f"{k:18s} ms per step: windows {' '.join(f'{t:.3f}' for t in v)} | median {med[k]:.3f} | spread {max(v) - min(v):.3f} | "
                f"{B / med[k] * 1e3:.0f} images/s")
        say(f"f16 / bf16-unfused-stem {med['f16'] / med['bf16-unfused-stem']:.4f} (the kernels: same launches); "
            f"f16 / bf16 as shipped {med['f16'] / med['bf16']:.4f}; bf16-unfused-stem / bf16 {med['bf16-unfused-stem'] / med['bf16']:.4f} "
            f"(what the fused stem is worth)")
        d16, dbf = med["f16"] - med["f16-fused-stem"], med["bf16-unfused-stem"] - med["bf16"]
        every = all(f < u for f, u in zip(win["f16-fused-stem"], win["f16"]))
        say(f"f16-fused-stem / f16 {med['f16-fused-stem'] / med['f16']:.4f}: {d16:.3f} ms returned of the {dbf:.3f} ms the fused stem returns to bf16 "
            f"({100 * d16 / dbf if dbf > 0 else float('nan'):.0f} %); below f16 in every window: {every}; f16's own window spread "
            f"{max(win['f16']) - min(win['f16']):.3f} ms")
        if a.per_conv:
            del graphs
            ms = {k: np.median([plans[k][0].profile_convs(x) for _ in range(9)], axis=0) for k in plans}
            say("-- per conv (each launch alone, median of 9): slot signature bf16-unfused ms, f16 ms, f16 / bf16-unfused | bf16 ms, f16-fused-stem ms")
            for i, o in enumerate(plans["f16"][0].conv_ops):
                b, f = ms["bf16-unfused-stem"][i], ms["f16"][i]
                say(f"{i:4d}  {runtime.Net.conv_signature(o, S):36s} {b:8.4f} {f:8.4f}   {f / b if b > 0 else float('nan'):6.3f} | "
                    f"{ms['bf16'][i]:8.4f} {ms['f16-fused-stem'][i]:8.4f}")
            say(f"sum   {'':36s} {ms['bf16-unfused-stem'].sum():8.4f} {ms['f16'].sum():8.4f}   {ms['f16'].sum() / ms['bf16-unfused-stem'].sum():6.3f} | "
                f"{ms['bf16'].sum():8.4f} {ms['f16-fused-stem'].sum():8.4f}")
            say("stem (convs 0..2): " + ", ".join(f"{k} {ms[k][:3].sum():.4f} ms" for k in plans))
        del plans

    if a.precision:
        from oracle import oracle as O
        from yolo_v3_tf2_amd.core.utils import load_image_u8
        S = 416
        img = load_image_u8(os.path.join(ROOT, "datasets/coco2012/images/girl.png"))
        batch = torch.empty((1, S, S, 3), dtype=torch.float32, device="cuda")
        runtime.preprocess_image(torch.from_numpy(img).cuda(), batch, 0)
        xh = batch.cpu().numpy()
        rb, rc, rs, rsel, rnv = O.detect(program, weights, xh, anchors)
        say(f"\n== precision: girl.png at {S}^2, forward_decode against the fp32 oracle's decode ({rb.shape[1]} candidates, "
            f"{int((rs > 0.1).sum())} with an oracle score above 0.1, {int(rnv[0])} detections)")
        net = runtime.Net(program)
        net.load_weights(weights)
        for tag, dt in (("bf16", _lib.Y3_DTYPE_BF16), ("f16", _lib.Y3_DTYPE_F16)):
            net.plan(1, S, dt)
            bb, cc, ss = (t.cpu().numpy() for t in net.forward_decode(batch, anchors))
            hot = rs > 0.1
            packed, nv = net.detect(batch, anchors, 100, 0.5, 0.1)
            say(f"{tag:5s} max |dbox| {np.abs(bb - rb).max():.3e} max |dscore| {np.abs(ss - rs).max():.3e} | above 0.1: max |dbox| "
                f"{np.abs(bb - rb)[hot].max():.3e} max |dscore| {np.abs(ss - rs)[hot].max():.3e} class flips {int((cc != rc)[hot].sum())} | "
                f"detections {int(nv[0])} (oracle {int(rnv[0])})")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
