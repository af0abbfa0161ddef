#!/usr/bin/env python3
"""YOLOv3-tiny on the device: what one detect costs, and what the max-pool kernel reaches.

fp32 (--dtype bf16 / f16 with --fused-stem: the fused tiny stem, with which the tiny model plans in the 16-bit modes; --dtype i8 with
--fused-stem: the int8 plan with Net.set_pools_i8, calibrated on the spot from two random frames, alternated with the fp16 and bf16 plans under
the same stem switch, and at one image also with set_low_latency_i8; section 3 is left out), config/models/yolov3_tiny/model.yaml with synthetic weights, Net.detect on
device-resident frames, by the protocol of tools/time_latency.py:
  eager  -- every call between a pair of device events on the stream;
  graph  -- the call captured with torch.cuda.graph, every replay timed with the host clock around a synchronise;
in alternated windows inside ONE process, median and 99th percentile over all calls and the median of every window (their spread is the
noise a difference has to clear).
  1. throughput: --batch (64) images of --size (416), images/s from the median step;
  2. latency: one image, the default plan against set_low_latency (split-K convs), alternated;
  3. the pool kernel alone: each of the six pools of the planned net through ops.maxpool2x2 on tensors of the net's own shapes, timed
     with device events over --pool-calls launches, bytes moved (input read once + output written) over the median time, next to a
     device-to-device copy of the SAME byte count (half read, half written) timed the same way in the same process;
  4. byte counts from shapes alone: what conv0's padded output and pool 0 are of the network's activation traffic.
The shares of the step that the pool launches and conv0 take come from a separate run under rocprofv3 --kernel-trace --stats
(--profile-steps N: nothing is timed, N detects are enqueued for the tracer); tools/summarize_prof.py reads its CSV.
    python tools/time_tiny.py [--batch 64] [--size 416] [--calls 200] [--windows 4] [--pool-calls 200] [--out profiles/tiny.txt]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/time_tiny.py --profile-steps 20"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--calls", type=int, default=200, help="timed calls per plan and form (after warm-up)")
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pool-calls", type=int, default=200)
    ap.add_argument("--profile-steps", type=int, default=0, help="enqueue this many detects and exit (for rocprofv3)")
    ap.add_argument("--dtype", choices=("f32", "bf16", "f16", "i8"), default="f32", help="the plans' conv arithmetic; bf16, f16 and i8 need --fused-stem")
    ap.add_argument("--fused-stem", action="store_true", help="the fused tiny stem kernel (Net.set_tiny_stem_fusion) in the measured plan; "
                                                               "sections 1 and 2 then alternate it with the fp32 plan without the switch")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import yolo_v3_tf2_amd  # noqa: F401
    from yolo_v3_tf2_amd import ops, runtime
    from yolo_v3_tf2_amd.core.utils import get_anchors
    from yolo_v3_tf2_amd.graph import AuxOp, load_program
    from yolo_v3_tf2_amd.weights import synthetic_weights

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    program = load_program(os.path.join(ROOT, "config/models/yolov3_tiny/model.yaml"), 80)
    weights = synthetic_weights(program)
    anchors = get_anchors(os.path.join(ROOT, "datasets/coco2012/anchors_tiny.txt")).astype(np.float32)
    B, S = a.batch, a.size

    dtype = runtime.Net._dtype_arg(a.dtype)
    if a.dtype != "f32" and not a.fused_stem:
        ap.error("--dtype bf16 / f16 / i8 needs --fused-stem: the tiny model plans in a 16-bit mode, and before an int8 cut, only with the fused stem")
    i8 = a.dtype == "i8"
    scales = []

    def make(batch, low_latency=False, fused=None, dt=None):
        """fused / dt None: what the command line says; the baseline of an A/B is make(batch, fused=False, dt=0), the fp32 plan without the switch"""
        net = runtime.Net(program)
        net.load_weights(weights)
        net.set_low_latency(low_latency)
        net.set_tiny_stem_fusion(a.fused_stem if fused is None else fused)
        dt = dtype if dt is None else dt
        if dt == runtime.Net._dtype_arg("i8"):
            net.set_low_latency_i8(low_latency)
            net.set_pools_i8(True)
            if not scales:      # absmax calibration from two random frames, once; every int8 net of this run takes the same scales
                scales.extend(net.calibrate_i8(torch.rand((2, S, S, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(1))))
            net.set_act_scales(scales)
        net.plan(batch, S, dt)
        return net

    if a.profile_steps:
        net = make(B)
        x = torch.rand((B, S, S, 3), device="cuda")
        for _ in range(a.profile_steps):
            net.detect(x, anchors, 100, 0.5, 0.1)
        torch.cuda.synchronize()
        return

    say(f"# tools/time_tiny.py  device: {torch.cuda.get_device_name(0)}  {a.dtype}{' fused stem' if a.fused_stem else ''}  YOLOv3-tiny, {len(program.conv_ops())} convs, "
        f"{sum(isinstance(o, AuxOp) for o in program.ops)} aux ops, N = {sum(3 * g * g for g in program.grid_sizes(S))} boxes at {S}")
    say(f"# GFLOP / image at {S}: {program.flops_per_image(S) / 1e9:.3f} (real channel counts)")

    # ---- 4. byte counts from shapes: every tensor an op writes and every tensor an op reads, fp32, per image
    stored = program.stored
    px = lambda t: (S // program.tensors[t].div) ** 2
    written = {o.dst: stored[o.dst] * px(o.dst) * 4 for o in program.ops}
    read = 0
    for o in program.ops:
        for t in ([o.src0, o.src1, o.residual] if hasattr(o, "conv_index") else o.inputs):
            if t is not None and t >= 0:
                read += stored[t] * px(t) * 4
    total = read + sum(written.values())
    c0, p0 = program.conv_ops()[0], [o for o in program.ops if isinstance(o, AuxOp)][0]
    part = written[c0.dst] + written[c0.dst] + written[p0.dst]       # conv0's store, pool 0's read of it, pool 0's store
    say(f"# activation traffic from shapes, per image: {total / 1e6:.1f} MB read + written (weights not counted); conv0's padded output "
        f"written and read by pool 0, plus pool 0's output: {part / 1e6:.1f} MB = {100.0 * part / total:.1f} %")

    def timed(steps, calls, label):
        """steps: {name: callable}; alternated windows, eager (device events) and graph replay (host clock)."""
        per_window = max(1, calls // a.windows)
        for k in steps:
            for _ in range(a.warmup):
                steps[k]()
        torch.cuda.synchronize()
        out = {}
        win = {k: [] for k in steps}
        for _ in range(a.windows):
            for k in steps:
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(per_window)]
                for e0, e1 in ev:
                    e0.record()
                    steps[k]()
                    e1.record()
                torch.cuda.synchronize()
                win[k].append(np.array([e0.elapsed_time(e1) for e0, e1 in ev]))
        out["eager"] = win
        graphs = {}
        for k in steps:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                steps[k]()
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                steps[k]()
            graphs[k] = g
            for _ in range(a.warmup):
                g.replay()
            torch.cuda.synchronize()
        win = {k: [] for k in steps}
        for _ in range(a.windows):
            for k in steps:
                ts = np.empty(per_window)
                for i in range(per_window):
                    t0 = time.perf_counter()
                    graphs[k].replay()
                    torch.cuda.synchronize()
                    ts[i] = (time.perf_counter() - t0) * 1e3
                win[k].append(ts)
        out["graph"] = win
        for form in ("eager", "graph"):
            for k in steps:
                allc = np.concatenate(out[form][k])
                meds = [float(np.median(w)) for w in out[form][k]]
                say(f"{label} {form:5s} {k:12s}: median {np.median(allc):.4f} ms  p99 {np.percentile(allc, 99):.4f}  window medians "
                    f"{' '.join(f'{v:.4f}' for v in meds)} (spread {max(meds) - min(meds):.4f})")
        return out

    # ---- 1. throughput
    net = make(B)
    x = torch.rand((B, S, S, 3), device="cuda")
    say(f"\n== detect, {B} x {S} x {S}, lanes {getattr(net, 'lanes', 1)}")
    steps = {"default": lambda: net.detect(x, anchors, 100, 0.5, 0.1)}
    if i8:                # A/B in one process: the fp16 and bf16 plans under the same stem switch in alternated windows
        others = {k: make(B, dt=runtime.Net._dtype_arg(k)) for k in ("f16", "bf16")}
        say(f"   'default' = i8 with set_pools_i8 and the fused tiny stem (pools_i8 = {net.pools_i8}, cut = conv {net.i8_first_conv()}, tiny_stem_fused = "
            f"{net.tiny_stem_fused}); 'f16', 'bf16' = those plans with the fused tiny stem")
        for k, n in others.items():
            steps[k] = lambda n=n: n.detect(x, anchors, 100, 0.5, 0.1)
    elif a.fused_stem:    # A/B in one process: the fp32 plan without the switch in alternated windows
        base = make(B, fused=False, dt=0)
        say(f"   'default' = {a.dtype} with the fused tiny stem (tiny_stem_fused = {net.tiny_stem_fused}); 'f32_unfused' = the fp32 plan without the switch")
        steps["f32_unfused"] = lambda: base.detect(x, anchors, 100, 0.5, 0.1)
    r = timed(steps, a.calls, "throughput")
    for form in ("eager", "graph"):
        for k in steps:
            med = float(np.median(np.concatenate(r[form][k])))
            say(f"throughput {form} {k}: {B / med * 1e3:.0f} images/s ({med:.4f} ms per step of {B})")
    if i8:
        del others
    elif a.fused_stem:
        del base
    pools = [(o, program.tensors[o.inputs[0]]) for o in program.ops if isinstance(o, AuxOp) and o.kind.startswith("maxpool")]
    del net
    torch.cuda.empty_cache()

    # ---- 2. latency at one image
    if i8:
        nets = {"default": make(1), "low_latency": make(1, True), "f16": make(1, dt=runtime.Net._dtype_arg("f16")), "bf16": make(1, dt=runtime.Net._dtype_arg("bf16"))}
    else:
        nets = {"default": make(1), "low_latency": make(1, True)} if not a.fused_stem else {"default": make(1), "f32_unfused": make(1, fused=False, dt=0)}
    x1 = torch.rand((1, S, S, 3), device="cuda")
    if i8:
        say(f"\n== detect, 1 x {S} x {S}; i8 default, i8 with set_low_latency_i8 (K slices per conv: "
            f"{[nets['low_latency'].split_k_i8(i) for i in range(len(program.conv_ops()))]}), f16 and bf16, all with the fused tiny stem")
    elif "low_latency" in nets:
        say(f"\n== detect, 1 x {S} x {S}; K slices per conv of the low-latency plan: {[nets['low_latency'].split_k(i) for i in range(len(program.conv_ops()))]}")
    else:
        say(f"\n== detect, 1 x {S} x {S}; {a.dtype} with the fused tiny stem against the fp32 plan without the switch")
    timed({k: (lambda n=n: n.detect(x1, anchors, 100, 0.5, 0.1)) for k, n in nets.items()}, max(a.calls, 400), "latency")
    del nets
    torch.cuda.empty_cache()
    if a.dtype not in ("f32", "bf16", "f16"):      # section 3 times the fp32 pool kernel on the six pools' shapes: an int8 plan launches two of them on bytes
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return

    # ---- 3. the pool kernel alone, beside a device-to-device copy of the same byte count
    say(f"\n== ops.maxpool2x2 on the six pools' own shapes, batch {B}, fp32 (stored widths); copy = torch copy_ of (read + written) / 2 bytes, "
        f"moving the same total")

    def event_median(fn, calls):
        for _ in range(10):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))

    tot_pool = tot_copy = 0.0
    for o, tin in pools:
        stride = 2 if o.kind == "maxpool_s2" else 1
        h = S // tin.div
        C = stored[o.inputs[0]]
        src = torch.rand((B, h, h, C), device="cuda")
        dst = torch.empty((B, h // stride, h // stride, C), device="cuda")
        nbytes = (src.numel() + dst.numel()) * 4
        half = torch.empty(nbytes // 8, device="cuda")
        half2 = torch.empty_like(half)
        t_pool = event_median(lambda: ops.maxpool2x2(src, stride, out=dst), a.pool_calls)
        t_copy = event_median(lambda: half2.copy_(half), a.pool_calls)
        tot_pool, tot_copy = tot_pool + t_pool, tot_copy + t_copy
        say(f"pool {h:3d} x {h:3d} x {C:4d} stride {stride}: {nbytes / 1e6:8.1f} MB  pool {t_pool:.4f} ms = {nbytes / t_pool / 1e9:6.2f} TB/s | "
            f"copy {t_copy:.4f} ms = {nbytes / t_copy / 1e9:6.2f} TB/s | pool / copy {t_pool / t_copy:.2f}")
        del src, dst, half, half2
    say(f"six pools: {tot_pool:.4f} ms, the copies {tot_copy:.4f} ms")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
