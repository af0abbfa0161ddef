#!/usr/bin/env python3
"""Latency of one detect call at small batches, low-latency plan (split-K convs, y3_net_set_low_latency) against the default plan.

fp32, image sizes 416 and 608, batches 1, 2, 4, 8: Net.detect on a device-resident frame, the two plans alternated in windows inside
ONE process.  Two forms per plan:
  eager  -- every call timed with a pair of device events on the stream (the step as the device sees it);
  graph  -- the call captured with torch.cuda.graph, every replay timed with the host clock around a synchronise (what a caller
            waiting for the detections sees).
Reported per (size, batch, form): median and 99th percentile over all calls of a plan, the median of every window, whether the
low-latency plan was below the default plan in every alternated pair of windows, and the gain beside the default plan's own spread
between its windows.  The split in force per conv is printed for every plan.
    python tools/time_latency.py [--sizes 416 608] [--batches 1 2 4 8] [--calls 1000] [--windows 4] [--per-conv] [--dtype f32] [--out profiles/latency.txt]
--dtype bf16 times bf16 plans, the low-latency one through y3_net_set_low_latency_bf16 (profiles/latency_bf16.txt).
--dtype f16 times fp16 plans, the low-latency one through y3_net_set_low_latency_f16 (profiles/latency_f16.txt).
--dtype i8 times int8 plans, the low-latency one through y3_net_set_low_latency_i8 (profiles/latency_i8.txt); the activation scales are
calibrated here on two seeded frames of each size, as tools/time_i8.py does.
--f16-fused-stem (with --dtype f16) switches the fused stem on in the "on" plan as well (y3_net_set_stem_fusion_f16).
--control makes "on" a SECOND DEFAULT-PLAN net: the same launches from two net objects, i.e. what the protocol reads when nothing differs.
--per-conv adds, for batch 1, the per-conv table of y3_net_profile_convs (each launch timed alone; a split conv is its two launches)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[416, 608])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--calls", type=int, default=1000, help="timed calls per plan and form (after warm-up)")
    ap.add_argument("--windows", type=int, default=4, help="alternated windows the calls are divided into")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--per-conv", action="store_true")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16", "f16", "i8"])
    ap.add_argument("--control", action="store_true", help="'on' is a second default-plan net (two net objects, the same launches)")
    ap.add_argument("--f16-fused-stem", action="store_true", help="fp16: the 'on' plan also fuses the stem")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sfx = {"f32": "", "bf16": "_bf16", "f16": "_f16", "i8": "_i8"}[a.dtype]

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
    weights = synthetic_weights(program)
    anchors = get_anchors(os.path.join(ROOT, "datasets/coco2012/anchors.txt")).astype(np.float32)
    nets = {}
    for name in ("off", "on"):
        net = runtime.Net(program)
        net.load_weights(weights)
        getattr(net, "set_low_latency" + sfx)(name == "on" and not a.control)
        if a.f16_fused_stem and a.dtype == "f16" and name == "on" and not a.control:
            net.set_stem_fusion_f16(True)
        nets[name] = net
    say(f"# tools/time_latency.py  device: {torch.cuda.get_device_name(0)}  { {'f32': 'fp32', 'f16': 'fp16'}.get(a.dtype, a.dtype)}  calls per plan and form: {a.calls} in {a.windows} alternated windows")
    say("# off = default plan, on = " + ("a second net with the default plan (control)" if a.control else "low-latency plan (split-K)" +
                                (" with the fused stem" if a.f16_fused_stem and a.dtype == "f16" else "")) +
        "; times in ms; 'pairs' = windows in which on < off")
    per_window = max(1, a.calls // a.windows)
    for S in a.sizes:
        if a.dtype == "i8":
            cal = runtime.Net(program)
            cal.load_weights(weights)
            scales = cal.calibrate_i8(torch.rand((2, S, S, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0)))
            del cal
            torch.cuda.empty_cache()
            for net in nets.values():
                net.set_act_scales(scales)
        for B in a.batches:
            x = torch.rand((B, S, S, 3), device="cuda")
            for net in nets.values():
                net.plan(B, S, {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16, "f16": _lib.Y3_DTYPE_F16, "i8": _lib.Y3_DTYPE_I8}[a.dtype])
            splits = [getattr(nets["on"], "split_k" + sfx)(i) for i in range(len(nets["on"].conv_ops))]
            say(f"\n== {S} x {S}, batch {B}: {sum(s > 1 for s in splits)} convs split; S per conv: {splits}")
            step = {k: (lambda n=n: n.detect(x, anchors, 100, 0.5, 0.1)) for k, n in nets.items()}
            for k in step:
                for _ in range(a.warmup):
                    step[k]()
            torch.cuda.synchronize()
            # ---- eager, device events
            win = {"off": [], "on": []}
            for _ in range(a.windows):
                for k in ("off", "on"):
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(per_window)]
                    for e0, e1 in ev:
                        e0.record()
                        step[k]()
                        e1.record()
                    torch.cuda.synchronize()
                    win[k].append(np.array([e0.elapsed_time(e1) for e0, e1 in ev]))
            report(say, "eager", win)
            # ---- graph replay, host clock
            graphs = {}
            for k in ("off", "on"):
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    step[k]()
                torch.cuda.current_stream().wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    step[k]()
                graphs[k] = g
                for _ in range(a.warmup):
                    g.replay()
                torch.cuda.synchronize()
            win = {"off": [], "on": []}
            for _ in range(a.windows):
                for k in ("off", "on"):
                    ts = np.empty(per_window)
                    for i in range(per_window):
                        t0 = time.perf_counter()
                        graphs[k].replay()
                        torch.cuda.synchronize()
                        ts[i] = (time.perf_counter() - t0) * 1e3
                    win[k].append(ts)
            report(say, "graph", win)
            del graphs
            if a.per_conv and B == 1:
                ms = {k: np.median([n.profile_convs(x) for _ in range(15)], axis=0) for k, n in nets.items()}
                say(f"-- per conv, batch 1, {S} x {S} (each launch alone, median of 15; a split conv = slices + finish launch)")
                say("slot  signature                              S   off ms   on ms   on/off")
                for i, o in enumerate(nets["on"].conv_ops):
                    sig = runtime.Net.conv_signature(o, S)
                    ratio = ms["on"][i] / ms["off"][i] if ms["off"][i] > 0 else float("nan")
                    say(f"{i:4d}  {sig:36s} {splits[i]:3d}  {ms['off'][i]:7.4f} {ms['on'][i]:7.4f}   {ratio:5.2f}")
                say(f"sum   {'':36s}      {ms['off'].sum():7.4f} {ms['on'].sum():7.4f}   {ms['on'].sum() / ms['off'].sum():5.2f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def report(say, form, win):
    off, on = np.concatenate(win["off"]), np.concatenate(win["on"])
    moff, mon = [float(np.median(w)) for w in win["off"]], [float(np.median(w)) for w in win["on"]]
    pairs = sum(b < a_ for a_, b in zip(moff, mon))
    spread = max(moff) - min(moff)
    gain = float(np.median(off) - np.median(on))
    say(f"{form}: off median {np.median(off):.4f} p99 {np.percentile(off, 99):.4f} | on median {np.median(on):.4f} p99 {np.percentile(on, 99):.4f}"
        f" | on/off {np.median(on) / np.median(off):.3f} | pairs {pairs}/{len(moff)}")
    say(f"       window medians off {' '.join(f'{v:.4f}' for v in moff)} | on {' '.join(f'{v:.4f}' for v in mon)}"
        f" | gain {gain:.4f} ms vs off's own window spread {spread:.4f} ms")


if __name__ == "__main__":
    main()
