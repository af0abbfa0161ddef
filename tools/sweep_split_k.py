#!/usr/bin/env python3
"""Per-conv sweep of the split-K factor S (y3_net_set_split_k) on a small-batch fp32 plan: what the constants of y3_choose_split_k
are set from.  For every eligible conv and every S of --splits (clamped to the conv's K tiles) the launch -- slices plus finish
launch -- is timed alone with y3_net_profile_convs, median of --repeats; the table gives per conv the time at every S, the best S,
the S the rule picks and what the rule leaves on the table, then the sums over the conv stack: unsplit, rule, best per conv.
    python tools/sweep_split_k.py [--size 416] [--batches 1 2 4 8] [--dtype f32] [--out profiles/latency_splitk_sweep.txt]
--dtype bf16 sweeps a bf16 plan through y3_net_set_split_k_bf16 (K tiles of 64; profiles/latency_bf16_splitk_sweep.txt).
--dtype f16 sweeps an fp16 plan through y3_net_set_split_k_f16 (K tiles of 64; profiles/latency_f16_splitk_sweep.txt).
--dtype i8 sweeps an int8 plan through y3_net_set_split_k_i8 (K tiles of 128, the convs from the cut on; the activation scales are
calibrated here on two seeded frames of each size, as tools/time_i8.py does; profiles/latency_i8_splitk_sweep.txt)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs="+", default=[416])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--splits", type=int, nargs="+", default=[1, 2, 3, 4, 6, 8, 12, 16])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16", "f16", "i8"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sfx = {"f32": "", "bf16": "_bf16", "f16": "_f16", "i8": "_i8"}[a.dtype]

    import torch
    import yolo_v3_tf2_amd  # noqa: F401
    from yolo_v3_tf2_amd import _lib, runtime
    from yolo_v3_tf2_amd.graph import load_program
    from yolo_v3_tf2_amd.weights import synthetic_weights

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    program = load_program(os.path.join(ROOT, "config/models/yolov3/model.yaml"), 80)
    net = runtime.Net(program)
    weights = synthetic_weights(program)
    net.load_weights(weights)
    n = len(net.conv_ops)
    set_split, get_split, set_ll = getattr(net, "set_split_k" + sfx), getattr(net, "split_k" + sfx), getattr(net, "set_low_latency" + sfx)
    dtype, bk = {"f32": (_lib.Y3_DTYPE_F32, 32), "bf16": (_lib.Y3_DTYPE_BF16, 64), "f16": (_lib.Y3_DTYPE_F16, 64),
                 "i8": (_lib.Y3_DTYPE_I8, 128)}[a.dtype]
    say(f"# tools/sweep_split_k.py  device: {torch.cuda.get_device_name(0)}  { {'f32': 'fp32', 'f16': 'fp16'}.get(a.dtype, a.dtype)}; ms per conv launch alone (split: slices + finish), median of {a.repeats}")
    for S_img in a.size:
        if a.dtype == "i8":
            cal = runtime.Net(program)
            cal.load_weights(weights)
            net.set_act_scales(cal.calibrate_i8(torch.rand((2, S_img, S_img, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))))
            del cal
            torch.cuda.empty_cache()
        for B in a.batches:
            x = torch.rand((B, S_img, S_img, 3), device="cuda")
            for i in range(n):
                set_split(i, -1)
            set_ll(True)
            net.plan(B, S_img, dtype)
            rule = [get_split(i) for i in range(n)]
            set_ll(False)
            ms, eff = {}, {}
            splits = sorted(set(a.splits) | set(rule))      # the rule's own values are always measured
            for S in splits:
                for i, o in enumerate(net.conv_ops):
                    want = min(S, max(1, o.size * o.size * o.cin // bk))
                    try:
                        set_split(i, want if want > 1 else 1)
                    except runtime.Y3Error:
                        set_split(i, 1)
                eff[S] = [get_split(i) for i in range(n)]
                net.profile_convs(x)
                ms[S] = np.median([net.profile_convs(x) for _ in range(a.repeats)], axis=0)
            say(f"\n== {S_img} x {S_img}, batch {B}")
            say("slot  signature                            " + "".join(f"  S={S:<5d}" for S in splits) + "  best  rule   rule-best ms")
            tot = {"unsplit": 0.0, "rule": 0.0, "best": 0.0}
            for i, o in enumerate(net.conv_ops):
                t = {S: float(ms[S][i]) for S in splits}
                # time at the S in force (a clamped or refused request repeats a smaller S: take the first column with that value)
                at = {}
                for S in splits:
                    at.setdefault(eff[S][i], t[S])
                best = min(at, key=at.get)
                t_rule = at[rule[i]]
                tot["unsplit"] += at[1]
                tot["rule"] += t_rule
                tot["best"] += at[best]
                cols = "".join(f"  {t[S]:7.4f}" if eff[S][i] == S else "        -" for S in splits)
                say(f"{i:4d}  {runtime.Net.conv_signature(o, S_img):36s}{cols}  {best:4d}  {rule[i]:4d}   {t_rule - at[best]:+.4f}")
            say(f"sum over the conv stack: unsplit {tot['unsplit']:.4f} ms | rule {tot['rule']:.4f} ms | best S per conv {tot['best']:.4f} ms")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
