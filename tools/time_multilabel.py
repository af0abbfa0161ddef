#!/usr/bin/env python3
"""Multi-label detections, measured.
   python tools/time_multilabel.py --kernels [--batch 64] [--image-size 416] [--calls 20]
   python tools/time_multilabel.py --stream [--dtype f32 --batch 64 | --dtype bf16 --batch 128] [--steps 12] [--windows 5]
--kernels: the launches to run under `rocprofv3 --kernel-trace --stats -- python tools/time_multilabel.py --kernels`, a run of its own:
y3_yolo_decode_scores (decode_kernel) next to y3_yolo_decode_candidates_hw (candidates_kernel<false>, cand_scan_kernel,
candidates_kernel<true>) on the same grids -- those the synthetic weights give for `batch` random images, at S = 0.1 and S = 0.005, and
the dense stress recipe of the tests (objectness ~ N(0,2), classes ~ N(-1,2)) at S = 0.1, then the synthetic grids at S = 0.5 (sparse
survivors) -- `calls` times each, with capacity N.  Without the profiler it times the same calls between device events and prints the
candidate counts, which name the inputs in the trace (the launches of one input are consecutive: scores x calls, then candidates x calls).
--stream: detect_stream over `steps` batches of 640x480 uint8 frames, single-label against multi-label (capacity N, per-class NMS in
both), alternated windows in one process, images/s per window with median and spread; then how many boxes carry two or more labels and
how many detections come back at each threshold, on the synthetic batch and on datasets/coco2012/images/girl.png."""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import yolo_v3_tf2_amd  # noqa: E402,F401
from yolo_v3_tf2_amd import _lib, ops, runtime  # noqa: E402
from yolo_v3_tf2_amd.core.utils import get_anchors  # noqa: E402
from yolo_v3_tf2_amd.graph import load_program  # noqa: E402
from yolo_v3_tf2_amd.weights import synthetic_weights  # noqa: E402

THRESHOLDS = (0.005, 0.05, 0.1, 0.3)


def timed(fn, calls):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def kernels(a, net, anchors):
    B, S = a.batch, a.image_size
    x = torch.from_numpy(np.random.default_rng(1234).random((B, S, S, 3), dtype=np.float32)).cuda()
    grids = [g.clone() for g in net.forward(x)]
    rng = np.random.default_rng(7)
    stress = []
    for g in grids:
        t = rng.standard_normal(tuple(g.shape)).astype(np.float32)
        t[..., 4] *= 2.0
        t[..., 5:] = t[..., 5:] * 2.0 - 1.0
        stress.append(torch.from_numpy(t).cuda())
    N = sum(3 * g.shape[1] * g.shape[2] for g in grids)
    for name, gr, thr in (("synthetic weights", grids, 0.1), ("synthetic weights", grids, 0.005), ("stress recipe", stress, 0.1),
                          ("synthetic weights", grids, 0.5)):      # the last: sparse survivors, what a trained network gives
        out = ops.decode_candidates(gr, anchors, 80, thr, N)
        ws = torch.empty(ops.decode_candidates_workspace_bytes([(g.shape[1], g.shape[2]) for g in gr], B, 80), dtype=torch.uint8, device="cuda")
        dec = ops._decode_scores(gr, anchors, 80)
        t_dec = timed(lambda: ops._decode_scores(gr, anchors, 80, out=dec), a.calls)
        t_cand = timed(lambda: ops.decode_candidates(gr, anchors, 80, thr, N, out=out, ws=ws), a.calls)
        tot = out[4].cpu().numpy()
        print(f"{name}, S = {thr}: {B} x {N} boxes x 80 classes; candidates per image {tot.min()}..{tot.max()} (mean {tot.mean():.0f}), "
              f"truncated at capacity N: {int((tot > N).sum())} images; between events: decode_scores {t_dec:.1f} us, "
              f"decode_candidates (three launches) {t_cand:.1f} us, ratio {t_cand / t_dec:.2f}")


def label_counts(net, x, anchors, what):
    grids = net.forward(x)
    N = sum(3 * g.shape[1] * g.shape[2] for g in grids)
    B = x.shape[0]
    for thr in THRESHOLDS:
        c = ops.decode_candidates(grids, anchors, 80, thr, N * 80)
        tot, src = c[4].cpu().numpy(), c[3].cpu().numpy()
        per_box = np.stack([np.bincount(src[b, :tot[b]], minlength=N) for b in range(B)])
        rows = {}
        for on in (False, True):
            net.multi_label = on
            rows[on] = int(net.detect(x, anchors, 100, 0.5, thr)[1].sum())
        net.multi_label = False
        print(f"  {what}, S = {thr}: boxes with a label {int((per_box >= 1).sum())}, with two or more {int((per_box >= 2).sum())}, candidates "
              f"{int(tot.sum())} ({int((tot > N).sum())} of {B} images above the capacity N = {N}); detections returned (M = 100, per-class NMS): "
              f"single-label {rows[False]}, multi-label {rows[True]}")


def stream(a, net, anchors):
    B, S = a.batch, a.image_size
    rng = np.random.default_rng(2024)
    frames = [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(B)]
    net.nms_per_class = True

    def window(on):
        net.multi_label = on
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)      # truncated images are counted below, not here
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in net.detect_stream([frames] * a.steps, anchors, 100, 0.5, a.score):
                pass
            torch.cuda.synchronize()
        return a.steps * B / (time.perf_counter() - t0)

    window(False), window(True)
    res = {False: [], True: []}
    for _ in range(a.windows):
        for on in (False, True):
            res[on].append(window(on))
    for on, v in res.items():
        print(f"detect_stream {a.dtype} {B} per batch, S = {a.score}, {'multi-label' if on else 'single-label'}: median {np.median(v):.1f} images/s  "
              f"min {min(v):.1f}  max {max(v):.1f}  (spread {max(v) - min(v):.1f}) over {len(v)} windows of {a.steps} batches")
    print(f"multi-label / single-label (medians): {np.median(res[True]) / np.median(res[False]):.3f}")
    net.multi_label = False
    x = torch.from_numpy(np.random.default_rng(1234).random((min(B, 8), S, S, 3), dtype=np.float32)).cuda()
    label_counts(net, x, anchors, f"synthetic batch of {x.shape[0]}")
    from PIL import Image
    girl = np.array(Image.open(os.path.join(ROOT, "datasets/coco2012/images/girl.png")).convert("RGB"), np.uint8)
    batch = torch.zeros((1, S, S, 3), device="cuda")
    runtime.preprocess_image(torch.from_numpy(girl).cuda(), batch, 0)
    label_counts(net, batch, anchors, "girl.png")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--image-size", type=int, default=416)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--score", type=float, default=0.1)
    a = ap.parse_args()
    _lib.require_gpu()
    program = load_program(os.path.join(ROOT, "config/models/yolov3/model.yaml"), 80)
    anchors = get_anchors(os.path.join(ROOT, "datasets/coco2012/anchors.txt")).astype(np.float32)
    net = runtime.Net(program)
    net.load_weights(synthetic_weights(program, seed=4321))
    net.plan(a.batch, a.image_size, {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16}[a.dtype])
    print(f"# tools/time_multilabel.py {' '.join(sys.argv[1:])}")
    if a.kernels:
        kernels(a, net, anchors)
    if a.stream:
        stream(a, net, anchors)


if __name__ == "__main__":
    main()
