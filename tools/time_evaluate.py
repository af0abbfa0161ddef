#!/usr/bin/env python3
"""Scoring a weight file over frames in host memory: images/s of three routes on the same seeded frames, synthetic weights and
synthetic ground truth (8 boxes per image), the five NMS score thresholds of config/evaluate_config.yaml.

  (a) evaluate   Net.evaluate_stream: one y3_net_detect per batch at the lowest threshold, the counters of all five
                 thresholds (plain and one-class) counted on the GPU, one read-back at the end
  (b) detect     Net.detect_stream on the same frames at the lowest threshold: what (a) adds the counting to
  (c) per-thr    the loop evaluate() runs without on_device: per threshold and per batch DetectModel.predict (a blocking
                 upload, the network, a read-back of the full [B,N,*] tensors), arrange_predict_output and the host
                 counters, plain and one-class.  It starts from the batch as float32 [B,416,416,3] -- the host-side decode and
                 resize of the data set are NOT included, so this route is an upper bound of that path.  Images/s counts
                 every image once, although the network sees it five times.

64-image batches (128 with --dtype bf16) of 640x480x3 uint8 frames at 416^2.  IMAGE DECODE IS EXCLUDED everywhere.  Every route
is warmed up; a timed window ends in a synchronise; the routes alternate, --rounds rounds; median and spread (max - min).

  python tools/time_evaluate.py [--dtype f32|bf16] [--batches 16] [--out FILE]
  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/time_evaluate.py --trace [--dtype ...]
  python tools/time_evaluate.py --summarize DIR [--dtype ...] [--out FILE]      (appends to FILE)
"""
import argparse
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S = 416
BATCH = {"f32": 64, "bf16": 128}
GT_PER_IMAGE = 8


def thresholds():
    import yaml
    with open(os.path.join(ROOT, "config", "evaluate_config.yaml")) as f:
        return [float(t) for t in yaml.safe_load(f)["evaluate_nms_score_thresholds"]]


def frames_and_truth(B, seed):
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(B)]
    gts = []
    for _ in range(B):
        c, s = rng.uniform(0.2, 0.8, (GT_PER_IMAGE, 2)), rng.uniform(0.1, 0.3, (GT_PER_IMAGE, 2))
        gts.append((np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32), rng.integers(0, 80, GT_PER_IMAGE).astype(np.int32)))
    return frames, gts


def setup(a):
    import yolo_v3_tf2_amd  # noqa: F401
    from yolo_v3_tf2_amd import _lib
    from yolo_v3_tf2_amd.core.parse_model import YoloModel
    from yolo_v3_tf2_amd.core.utils import get_anchors
    from yolo_v3_tf2_amd.graph import load_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    _lib.require_gpu()       # a measurement path that finds no GPU fails
    program = load_program(os.path.join(ROOT, "config/models/yolov3/model.yaml"), 80)
    anchors = get_anchors(os.path.join(ROOT, "datasets/coco2012/anchors.txt")).astype(np.float32)
    model = YoloModel(program)
    model.set_weights_dict(synthetic_weights(program, seed=4321))
    net = model._device_net()
    net.plan(BATCH[a.dtype], S, {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16}[a.dtype])
    return model, net, anchors


def measure(a):
    import torch
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd.evaluate_detections import EvaluateDetections, counters_from_row
    from yolo_v3_tf2_amd.evaluate_yolov3 import arrange_predict_output
    from yolo_v3_tf2_amd.inference import DetectModel
    model, net, anchors = setup(a)
    B, T = BATCH[a.dtype], thresholds()
    frames, gts = frames_and_truth(B, a.seed)
    # the batch route (c) starts from: what the data set hands evaluate(), resized by the same kernel the other routes use
    blob, descs = runtime.pack_images(frames, 1)
    resized = torch.empty((B, S, S, 3), device="cuda")
    runtime.preprocess_batch(torch.from_numpy(blob).cuda(), descs, resized)
    batch_host = resized.cpu().numpy()
    gt_y = np.stack([np.concatenate([b, np.ones((len(b), 1), np.float32), c[:, None].astype(np.float32)], 1) for b, c in gts])

    def evaluate(k):
        return net.evaluate_stream([frames] * k, [gts] * k, anchors, 100, 0.5, T, 80, one_class="both")

    def detect(k):
        for _ in net.detect_stream([frames] * k, anchors, 100, 0.5, min(T)):
            pass

    def per_threshold(k):
        rows = []
        for t in T:
            det = DetectModel(model, anchors, 80, 100, 0.5, t)
            ev, ev1 = EvaluateDetections(80, 0.5), EvaluateDetections(80, 0.5)
            for _ in range(k):
                pb, pc, gb, gc = arrange_predict_output(*det.predict(batch_host), gt_y)
                for b_, c_, g_, gc_ in zip(pb, pc, gb, gc):
                    ev.evaluate(b_, c_, g_, gc_)
                    ev1.evaluate(b_, np.zeros_like(c_), g_, np.zeros_like(gc_))
            rows.append((ev.counters, ev1.counters))
        return rows

    # the routes must agree before any of them is timed
    plain, one = evaluate(1)
    for t, (c, c1) in enumerate(per_threshold(1)):
        for got, ref in ((counters_from_row(plain[t], 80), c), (counters_from_row(one[t], 80), c1)):
            assert all(np.array_equal(got[k], ref[k]) for k in ref), (T[t], "evaluate_stream differs from the per-threshold route")
    first = counters_from_row(plain[0], 80)
    routes = {"evaluate": evaluate, "detect": detect, "per_threshold": per_threshold}
    rates = {n: [] for n in routes}
    for fn in routes.values():
        fn(1)
    for r in range(a.rounds):
        for name in (list(routes) if r % 2 == 0 else list(routes)[::-1]):
            k = a.batches if name != "per_threshold" else max(1, a.batches // 4)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            routes[name](k)
            torch.cuda.synchronize()
            rates[name].append(k * B / (time.perf_counter() - t0))
    med = {n: float(np.median(v)) for n, v in rates.items()}
    lines = [f"# tools/time_evaluate.py --dtype {a.dtype} --batches {a.batches}: {B} x 640x480x3 uint8 frames per batch -> {S}^2, {a.dtype} plan, "
             f"thresholds {T}, {GT_PER_IMAGE} ground-truth boxes per image, synthetic weights; image decode excluded",
             f"# at {T[0]}: preds {int(first['preds'].sum())} tp {int(first['tp'].sum())} fp {int(first['fp'].sum())} fn {int(first['fn'].sum())} per batch; "
             f"{a.rounds} alternating rounds, median images/s (spread = max - min)"]
    for name, what in (("evaluate", "(a) Net.evaluate_stream, all thresholds, plain + one-class"),
                       ("detect", "(b) Net.detect_stream at the lowest threshold"),
                       ("per_threshold", "(c) per-threshold loop: DetectModel.predict + host counters")):
        v = rates[name]
        lines.append(f"{what:<62s} {med[name]:10.1f} images/s  (spread {max(v) - min(v):.1f}; {' '.join(f'{x:.0f}' for x in v)})")
    lines.append(f"(a) / (b) = {med['evaluate'] / med['detect']:.3f}     (a) / (c) = {med['evaluate'] / med['per_threshold']:.2f}")
    emit(a, lines)


def trace(a):
    """For a rocprofv3 --kernel-trace --stats run: evaluate_stream alone."""
    _, net, anchors = setup(a)
    frames, gts = frames_and_truth(BATCH[a.dtype], a.seed)
    net.evaluate_stream([frames] * a.batches, [gts] * a.batches, anchors, 100, 0.5, thresholds(), 80, one_class="both")
    print(f"trace run done: {a.batches} batches of {BATCH[a.dtype]} frames, {a.dtype}")


def summarize(a):
    files = glob.glob(os.path.join(a.summarize, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {a.summarize}")
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(files[0])))
    ev = np.array([e - s for s, e, n in rows if "evaluate_kernel" in n], np.float64)
    nms = [s for s, e, n in rows if "nms_kernel" in n]
    assert len(ev) == 2 * len(nms) and len(nms) >= 3, (len(ev), len(nms))
    per_batch = np.diff(nms)[1:]          # start of one batch's NMS to the next one's: a whole batch of kernels; the first is warm-up
    busy = [sum(e - s for s, e, n in rows if nms[i] <= s < nms[i + 1]) for i in range(1, len(nms) - 1)]
    lines = [f"# rocprofv3 --kernel-trace --stats of `tools/time_evaluate.py --trace --dtype {a.dtype}`: {len(nms)} batches of {BATCH[a.dtype]} frames; "
             "tracing slows the host: kernel times, not rates",
             f"evaluate_kernel, one launch ({BATCH[a.dtype]} images, 5 thresholds)     median {np.median(ev) / 1e3:8.2f} us   min {ev.min() / 1e3:.2f}   max {ev.max() / 1e3:.2f}   "
             f"({len(ev)} launches)",
             f"evaluate_kernel per batch (two launches: plain, one-class)  {2 * np.median(ev) / 1e3:8.2f} us",
             f"all kernels of a batch, summed                             {np.median(busy) / 1e3:8.2f} us   -> evaluate_kernel is "
             f"{2 * np.median(ev) / np.median(busy) * 100:.3f} % of the kernel time of a batch",
             f"batch period under the tracer                              {np.median(per_batch) / 1e3:8.2f} us"]
    emit(a, lines)


def emit(a, lines):
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f32", choices=sorted(BATCH))
    ap.add_argument("--batches", type=int, default=16, help="batches per timed window of routes (a) and (b); (c) runs a quarter of them")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default="", help="append the report to this file")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarize", default="", help="directory of a rocprofv3 --kernel-trace run of --trace")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a)
    return trace(a) if a.trace else measure(a)


if __name__ == "__main__":
    main()
