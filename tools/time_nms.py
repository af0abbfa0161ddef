#!/usr/bin/env python3
"""nms_kernel on the boxes / scores the bench's own network produces (seeded weights and images), microseconds per call, and
y3_nms_padded against y3_nms_padded_per_class on the SAME decoded tensors, one process, the two rules alternated.
   python tools/time_nms.py [--dtype f32] [--batch 64] [--image-size 416] [--calls 50] [--windows 9] [--classes 80] [--agnostic-only]
First the figures this tool has always printed (nms_padded, nms_padded + pack, eager launches; the DIGEST of the agnostic selection,
which an A/B of two builds under Y3_LIB_PATH compares); --agnostic-only stops there (a build from before the per-class rule).
Then the two rules on two inputs: the decode of `batch` random images by the synthetic weights (10647 boxes per image at 416^2; the class ids are the
decode's own) at S = 0.1, and the NMS stress set of the tests (heavy overlap, exact duplicates, tied scores; uniform class ids) at
S = 0.1.  Per input and rule one HIP graph of `calls` NMS launches is captured; a window is one replay between two device events.
Windows alternate agnostic / per-class; the figure is the median over the windows, in microseconds per call, with their spread
(max - min).  The outputs of the two rules are compared once: with more than one class present they must differ in num_valid or
the run says so."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import yolo_v3_tf2_amd  # noqa: E402,F401
from yolo_v3_tf2_amd import _lib, ops, runtime  # noqa: E402
from yolo_v3_tf2_amd.core.utils import get_anchors  # noqa: E402
from yolo_v3_tf2_amd.graph import load_program  # noqa: E402
from yolo_v3_tf2_amd.weights import synthetic_weights  # noqa: E402
from tests.helpers import nms_stress_set  # noqa: E402  -- the one stress set: the tests' and this tool's


def capture(step, calls):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = step()        # warm-up: the workspace is made here
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            out = step()
    return g, out


def eager(a, bb, cls, sc):
    """100 eager launches of nms_padded, and of nms_padded + pack, behind 5 warm-up calls; the digest of the selection"""
    torch.cuda.synchronize()
    above = (sc > 0.1).sum(dim=1)
    for name, fn in (("nms_padded", lambda: runtime.nms_padded(bb, sc, 100, 0.5, 0.1)),
                     ("nms_padded + pack", lambda: runtime.pack_detections(bb, cls, sc, *runtime.nms_padded(bb, sc, 100, 0.5, 0.1)))):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(100):
            fn()
        e1.record()
        torch.cuda.synchronize()
        print(f"{name}: {e0.elapsed_time(e1) / 100 * 1e3:.1f} us per call ({a.batch} images x {sc.shape[1]} boxes, {a.dtype} network; "
              f"candidates above the score threshold per image: min {int(above.min())} mean {float(above.float().mean()):.0f} max {int(above.max())})")
    sel, nv = runtime.nms_padded(bb, sc, 100, 0.5, 0.1)
    torch.cuda.synchronize()
    print("DIGEST sel", hashlib.sha256(sel.cpu().numpy().tobytes()).hexdigest(), "num_valid", hashlib.sha256(nv.cpu().numpy().tobytes()).hexdigest())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"], help="the plan that decodes the synthetic-weights input")
    ap.add_argument("--agnostic-only", action="store_true", help="only the eager figures and the DIGEST of y3_nms_padded")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--image-size", type=int, default=416)
    ap.add_argument("--calls", type=int, default=50, help="NMS launches per captured graph (one window)")
    ap.add_argument("--windows", type=int, default=9, help="windows per rule, alternated")
    ap.add_argument("--classes", type=int, default=80, help="class count of the stress set's ids")
    ap.add_argument("--max-boxes", type=int, default=100)
    a = ap.parse_args()
    _lib.require_gpu()
    B, S, M, T, thr = a.batch, a.image_size, a.max_boxes, 0.5, 0.1
    program = load_program(os.path.join(ROOT, "config/models/yolov3/model.yaml"), 80)
    anchors = get_anchors(os.path.join(ROOT, "datasets/coco2012/anchors.txt")).astype(np.float32)
    net = runtime.Net(program)
    net.load_weights(synthetic_weights(program, seed=4321))
    net.plan(B, S, {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16}[a.dtype])
    x = torch.from_numpy(np.random.default_rng(1234).random((B, S, S, 3), dtype=np.float32)).cuda()
    decoded = net.forward_decode(x, anchors)
    N = decoded[2].shape[1]
    eager(a, *decoded)
    if a.agnostic_only:
        return
    rng = np.random.default_rng(2025)
    sb, ss = nms_stress_set(rng, B, N)
    stress = (torch.from_numpy(sb).cuda(), torch.from_numpy(rng.integers(0, a.classes, (B, N)).astype(np.int64)).cuda(), torch.from_numpy(ss).cuda())
    for name, (boxes, cls, scores) in (("synthetic weights", decoded), ("stress set", stress)):
        steps = {"agnostic": lambda: ops.nms_padded(boxes, scores, M, T, thr),
                 "per_class": lambda: ops.nms_padded_per_class(boxes, scores, cls, M, T, thr)}
        graphs = {k: capture(f, a.calls) for k, f in steps.items()}
        for g, _ in graphs.values():
            g.replay()      # one untimed replay each: the capture itself ran nothing
        torch.cuda.synchronize()
        cand = (scores > thr).sum(1)
        nv = {k: out[1].cpu().numpy() for k, (_, out) in graphs.items()}
        print(f"{name}: {B} x {N} boxes, S = {thr}, T = {T}, M = {M}; candidates per image {int(cand.min())}..{int(cand.max())}, "
              f"classes among them {len(torch.unique(cls[scores > thr]))}; num_valid agnostic {nv['agnostic'].min()}..{nv['agnostic'].max()} "
              f"(sum {nv['agnostic'].sum()}), per class {nv['per_class'].min()}..{nv['per_class'].max()} (sum {nv['per_class'].sum()})"
              + ("" if not np.array_equal(nv["agnostic"], nv["per_class"]) else "  [the two rules select equally many here]"))
        times = {k: [] for k in graphs}
        for _ in range(a.windows):
            for k, (g, _) in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                g.replay()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.calls)
        for k, v in times.items():
            print(f"  {k:10s} median {np.median(v):8.2f} us per call   min {min(v):8.2f}  max {max(v):8.2f}  (spread {max(v) - min(v):.2f}) over {len(v)} windows of {a.calls} calls")
        print(f"  per_class / agnostic (medians): {np.median(times['per_class']) / np.median(times['agnostic']):.3f}")


if __name__ == "__main__":
    main()
