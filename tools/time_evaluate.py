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

--ap: what COCO-style average precision (Net.evaluate_stream(ap=True): one y3_match_detections per batch, the AP integral on the
host at the end) adds to route (a).  Windows of ap=None and ap=True alternate in one process:
  python tools/time_evaluate.py --ap [--dtype f32|bf16] [--batches 16] [--rounds 5] [--out FILE]
and the two kernels side by side, no network: 64 images of 100 packed rows, 80 classes, 0 / 10 / 100 ground-truth boxes per image,
evaluate_kernel at the five score thresholds and ap_match_kernel at one and at ten IoU thresholds, LAUNCHES launches each
  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/time_evaluate.py --ap --trace
  python tools/time_evaluate.py --ap --summarize DIR [--out FILE]
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


def measure_ap(a):
    """evaluate_stream images/s with ap=True against ap=None, alternated windows in one process."""
    import torch
    _, net, anchors = setup(a)
    B, T = BATCH[a.dtype], thresholds()
    frames, gts = frames_and_truth(B, a.seed)
    routes = {"ap=None": lambda k: net.evaluate_stream([frames] * k, [gts] * k, anchors, 100, 0.5, T, 80, one_class="both"),
              "ap=True": lambda k: net.evaluate_stream([frames] * k, [gts] * k, anchors, 100, 0.5, T, 80, one_class="both", ap=True)}
    plain, with_ap = routes["ap=None"](1), routes["ap=True"](1)
    assert np.array_equal(plain[0], with_ap[0][0]) and np.array_equal(plain[1], with_ap[0][1]), "the counters must not depend on ap"
    rates = {n: [] for n in routes}
    for r in range(a.rounds):
        for name in (list(routes) if r % 2 == 0 else list(routes)[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            routes[name](a.batches)
            torch.cuda.synchronize()
            rates[name].append(a.batches * B / (time.perf_counter() - t0))
    med = {n: float(np.median(v)) for n, v in rates.items()}
    ap = with_ap[1]
    lines = [f"# tools/time_evaluate.py --ap --dtype {a.dtype} --batches {a.batches}: {B} x 640x480x3 uint8 frames per batch -> {S}^2, {a.dtype} plan, "
             f"score thresholds {T}, ten IoU thresholds 0.5 .. 0.95, {GT_PER_IMAGE} ground-truth boxes per image, synthetic weights; image decode excluded",
             f"# the AP of this synthetic pairing: mAP {ap['mAP']:.4f}, AP50 {ap['map'][0]:.4f}, images {ap['images']}; "
             f"{a.rounds} alternating rounds, median images/s (spread = max - min); ap=True includes the host's AP integral at the end of each window"]
    for name in routes:
        v = rates[name]
        lines.append(f"Net.evaluate_stream, {name:<8s} {med[name]:10.1f} images/s  (spread {max(v) - min(v):.1f}; {' '.join(f'{x:.0f}' for x in v)})")
    lines.append(f"ap=True / ap=None = {med['ap=True'] / med['ap=None']:.4f}")
    emit(a, lines)


AP_TRACE_GT = (0, 10, 100)
AP_TRACE_K = (1, 10)
AP_TRACE_IMAGES, AP_TRACE_ROWS = 64, 100


def ap_trace_inputs(gt_per_image, seed):
    """64 images of 100 packed rows in descending score: jittered copies of the image's ground-truth boxes with their classes
    (random boxes where there is no ground truth), 80 classes."""
    rng = np.random.default_rng(seed)
    B, M, G = AP_TRACE_IMAGES, AP_TRACE_ROWS, max(gt_per_image, 1)
    c, s = rng.uniform(0.2, 0.8, (B, G, 2)), rng.uniform(0.1, 0.3, (B, G, 2))
    gb = np.concatenate([c - s / 2, c + s / 2], 2).astype(np.float32)
    gc = rng.integers(0, 80, (B, G)).astype(np.int32)
    pick = rng.integers(0, G, (B, M))
    boxes = np.take_along_axis(gb, pick[..., None], 1) + rng.normal(0, 0.01, (B, M, 4)).astype(np.float32)
    classes = np.take_along_axis(gc, pick, 1)
    packed = np.zeros((B, M, 7), np.int32)
    packed[..., :4] = boxes.view(np.int32)
    packed[..., 4] = (-np.sort(-rng.uniform(0, 1, (B, M)).astype(np.float32), axis=1)).view(np.int32)
    packed[..., 5] = classes
    packed[..., 6] = np.arange(M)
    return packed, np.full(B, M, np.int32), gb, gc, np.full(B, gt_per_image, np.int32)


def trace_ap(a):
    """For a rocprofv3 --kernel-trace --stats run: per ground-truth count and per number of IoU thresholds, a.launches pairs of
    evaluate_kernel and ap_match_kernel on the same rows, in a fixed order that summarize_ap relies on."""
    import torch
    import yolo_v3_tf2_amd  # noqa: F401
    from yolo_v3_tf2_amd import _lib, runtime
    from yolo_v3_tf2_amd.evaluate_detections import AP_IOU_THRESHOLDS
    _lib.require_gpu()
    T = thresholds()
    for g in AP_TRACE_GT:
        data = [torch.from_numpy(x).cuda() for x in ap_trace_inputs(g, a.seed)]
        for K in AP_TRACE_K:
            counters, records, totals = None, None, None
            for _ in range(a.launches):
                counters = runtime.evaluate_detections(*data, 80, 0.5, T, counters=counters)
                records, totals = runtime.match_detections(*data, 80, AP_IOU_THRESHOLDS[:K], records=records, gt_totals=totals)
            torch.cuda.synchronize()
            masks = records.cpu().numpy().view(np.uint32)[..., 1] >> 16
            print(f"gt {g:3d} K {K:2d}: rows matched at 0.5: {int((masks & 1).sum())} of {masks.size}", flush=True)
    print(f"trace run done: {len(AP_TRACE_GT) * len(AP_TRACE_K)} configurations of {a.launches} launch pairs")


def summarize_ap(a):
    files = glob.glob(os.path.join(a.summarize, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {a.summarize}")
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(files[0])))
    ev = np.array([e - s for s, e, n in rows if "evaluate_kernel" in n], np.float64)
    ap = np.array([e - s for s, e, n in rows if "ap_match_kernel" in n], np.float64)
    cfgs = len(AP_TRACE_GT) * len(AP_TRACE_K)
    assert len(ev) == len(ap) and len(ev) % cfgs == 0 and len(ev) >= 3 * cfgs, (len(ev), len(ap))
    ev, ap = ev.reshape(cfgs, -1)[:, 1:] / 1e3, ap.reshape(cfgs, -1)[:, 1:] / 1e3      # the first launch of a configuration is warm-up
    lines = [f"# rocprofv3 --kernel-trace --stats of `tools/time_evaluate.py --ap --trace`: {AP_TRACE_IMAGES} images x {AP_TRACE_ROWS} packed rows, 80 classes; "
             f"evaluate_kernel at 5 score thresholds, ap_match_kernel at K IoU thresholds (one wave each); {ev.shape[1]} launches each, "
             "median us (min .. max)",
             "# gt boxes/image   K   evaluate_kernel            ap_match_kernel            ratio of medians"]
    for i, (g, K) in enumerate((g, K) for g in AP_TRACE_GT for K in AP_TRACE_K):
        lines.append(f"  {g:14d}  {K:2d}   {np.median(ev[i]):7.2f} ({ev[i].min():.2f} .. {ev[i].max():.2f})   "
                     f"{np.median(ap[i]):7.2f} ({ap[i].min():.2f} .. {ap[i].max():.2f})   {np.median(ap[i]) / np.median(ev[i]):6.2f}")
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
    ap.add_argument("--ap", action="store_true", help="measure what average precision adds: see the module docstring")
    ap.add_argument("--launches", type=int, default=21, help="--ap --trace: launch pairs per configuration (the first is warm-up)")
    a = ap.parse_args()
    if a.ap:
        return summarize_ap(a) if a.summarize else trace_ap(a) if a.trace else measure_ap(a)
    if a.summarize:
        return summarize(a)
    return trace(a) if a.trace else measure(a)


if __name__ == "__main__":
    main()
