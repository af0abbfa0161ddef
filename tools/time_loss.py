#!/usr/bin/env python3
"""The validation loss on the GPU: what its two kernels cost and what Net.evaluate_stream(loss=True) costs end to end.

  kernels     64 images at 416^2 (grids 13 / 26 / 52), 80 classes, random logits, 0 / 10 / 100 ground-truth boxes per image:
              microseconds per launch of y3_yolo_assign_targets and y3_yolo_loss, next to y3_yolo_decode_scores on the same grids
              in the same run (the yardstick: the loss reads channel 4 of every row and the full rows of the assigned ones only,
              decode_scores reads every logit).  KERNEL DURATIONS come from the rocprofv3 route below (--trace, then
              --summarize): quote those.  The plain run also reports the period of --launches back-to-back launches between two
              device events; for kernels of a few microseconds that is the rate at which the host can enqueue them through
              Python, an upper bound of the kernel time, and is labelled so.
  end to end  Net.evaluate_stream with and without loss=True on the frames of tools/time_evaluate.py (640x480x3 uint8 -> 416^2, five
              thresholds, plain + one-class counters), fp32 at 64 and bf16 at 128 images per batch, alternating, median images/s.
              loss=True takes the composed route, which writes and re-reads the raw grids (232 MB per 64 images).

  python tools/time_loss.py [--out FILE] [--batches 16] [--rounds 3]          (appends to profiles/loss_stage.txt by default)
  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/time_loss.py --trace
  python tools/time_loss.py --summarize DIR [--out FILE]      (appends to FILE)
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_evaluate import BATCH, S, emit, frames_and_truth, setup, thresholds  # noqa: E402

KERNEL_BATCH, NC, GRIDS = 64, 80, (13, 26, 52)
BOXES = (0, 10, 100)


def file_anchors():
    import yolo_v3_tf2_amd  # noqa: F401
    from yolo_v3_tf2_amd import _lib
    from yolo_v3_tf2_amd.core.utils import get_anchors
    _lib.require_gpu()       # a measurement path that finds no GPU fails
    return get_anchors(os.path.join(ROOT, "datasets/coco2012/anchors.txt")).astype(np.float32)


def ground_truth(rng, B, k):
    """k boxes per image: centres U(0.05, 0.95), sides log-uniform in [0.02, 0.6], corners inside the image."""
    gts = []
    for _ in range(B):
        c, s = rng.uniform(0.05, 0.95, (k, 2)), np.exp(rng.uniform(np.log(0.02), np.log(0.6), (k, 2)))
        gts.append((np.clip(np.concatenate([c - s / 2, c + s / 2], 1), 0, 0.999).astype(np.float32), rng.integers(0, NC, k).astype(np.int32)))
    return gts


def kernel_inputs(seed, k):
    import torch
    from yolo_v3_tf2_amd import runtime
    gen = torch.Generator(device="cuda").manual_seed(seed)
    grids = [torch.randn((KERNEL_BATCH, g, g, 3, 5 + NC), device="cuda", generator=gen) * 1.5 for g in GRIDS]
    gb, gc, cnt = (torch.from_numpy(a).cuda() for a in runtime.pack_ground_truth(ground_truth(np.random.default_rng(seed), KERNEL_BATCH, k)))
    return grids, gb, gc, cnt


def kernel_steps(anchors, k, seed):
    """-> {name: callable that enqueues one launch} on one set of buffers."""
    import torch
    from yolo_v3_tf2_amd import runtime
    grids, gb, gc, cnt = kernel_inputs(seed, k)
    import ctypes as C
    from yolo_v3_tf2_amd import _lib
    cells = torch.empty(gc.shape, dtype=torch.int32, device="cuda")
    loss = torch.empty((KERNEL_BATCH, 3, 4), dtype=torch.float64, device="cuda")
    # decode_scores into buffers made once, like the other two: no allocation inside a timed window
    N = sum(3 * g * g for g in GRIDS)
    bboxes = torch.empty((KERNEL_BATCH, N, 4), device="cuda")
    cls, scores = torch.empty((KERNEL_BATCH, N), dtype=torch.int64, device="cuda"), torch.empty((KERNEL_BATCH, N), device="cuda")
    ptrs, gs = (C.c_void_p * 3)(*[g.data_ptr() for g in grids]), (C.c_int32 * 3)(*GRIDS)
    a = np.ascontiguousarray(anchors, np.float32)
    lib = _lib.load()

    def decode_scores():
        _lib.check(lib.y3_yolo_decode_scores(ptrs, gs, KERNEL_BATCH, NC, a.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(bboxes.data_ptr()),
                                             C.c_void_p(cls.data_ptr()), C.c_void_p(scores.data_ptr()), _lib.stream_ptr()), "y3_yolo_decode_scores")

    # assign_targets comes first: it fills the cells yolo_loss reads
    return {"assign_targets": lambda: runtime.assign_targets(gb, gc, cnt, anchors, GRIDS, NC, cells=cells),
            "yolo_loss": lambda: runtime.yolo_loss(grids, anchors, NC, gb, gc, cells, loss=loss),
            "decode_scores": decode_scores}


def time_kernels(a, anchors):
    import torch
    lines = [f"# launch period (NOT kernel duration: it includes the host's enqueue through Python): {KERNEL_BATCH} images, grids {GRIDS}, {NC} classes, "
             f"logits N(0, 1.5); device events around {a.launches} back-to-back launches, {a.rounds} alternating rounds: median us per launch (min .. max)"]
    for k in BOXES:
        steps = kernel_steps(anchors, k, a.seed + k)
        us = {n: [] for n in steps}
        for fn in steps.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for r in range(a.rounds):
            for name in (list(steps) if r % 2 == 0 else list(steps)[::-1]):
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(a.launches):
                    steps[name]()
                end.record()
                end.synchronize()
                us[name].append(start.elapsed_time(end) * 1e3 / a.launches)
        med = {n: float(np.median(v)) for n, v in us.items()}
        for name, v in us.items():
            lines.append(f"{k:3d} boxes per image  {name:<16s} {med[name]:9.2f} us  ({min(v):.2f} .. {max(v):.2f})")
        lines.append(f"{k:3d} boxes per image  yolo_loss / decode_scores = {med['yolo_loss'] / med['decode_scores']:.3f}")
    emit(a, lines)


def time_streams(a):
    import argparse as ap
    import torch
    lines = [f"# end to end: Net.evaluate_stream on {a.batches} batches of 640x480x3 uint8 frames -> {S}^2, thresholds {thresholds()}, plain + "
             f"one-class counters, 8 ground-truth boxes per image; {a.rounds} alternating rounds, median images/s (min .. max)"]
    for dtype in ("f32", "bf16"):
        _, net, anchors = setup(ap.Namespace(dtype=dtype))
        B, T = BATCH[dtype], thresholds()
        frames, gts = frames_and_truth(B, a.seed)

        def run(k, loss):
            return net.evaluate_stream([frames] * k, [gts] * k, anchors, 100, 0.5, T, 80, one_class="both", loss=loss)

        plain = run(1, False)
        with_loss, sums = run(1, True)
        assert all(np.array_equal(x, y) for x, y in zip(plain, with_loss)), "loss=True changed the counters"
        rates = {False: [], True: []}
        for r in range(a.rounds):
            for loss in ((False, True) if r % 2 == 0 else (True, False)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(a.batches, loss)
                torch.cuda.synchronize()
                rates[loss].append(a.batches * B / (time.perf_counter() - t0))
        med = {k: float(np.median(v)) for k, v in rates.items()}
        for loss in (False, True):
            v = rates[loss]
            lines.append(f"{dtype:<5s} {B:4d} per batch  loss={str(loss):<5s} {med[loss]:10.1f} images/s  ({min(v):.1f} .. {max(v):.1f})")
        lines.append(f"{dtype:<5s} loss=True / loss=False = {med[True] / med[False]:.3f}   (val_loss of the batch {sums['sum'].sum() / max(sums['images'], 1):.4f}, "
                     f"{sums['images']} images, {sums['errors']} errors)")
        del net
        torch.cuda.empty_cache()
    emit(a, lines)


def trace(a):
    """For a rocprofv3 --kernel-trace --stats run: the three kernels alone, --launches launches each per box count."""
    import torch
    anchors = file_anchors()
    for k in BOXES:
        for fn in kernel_steps(anchors, k, a.seed + k).values():
            for _ in range(a.launches):
                fn()
        torch.cuda.synchronize()
    print(f"trace run done: {a.launches} launches per kernel and box count {BOXES}")


def summarize(a):
    files = glob.glob(os.path.join(a.summarize, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {a.summarize}")
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(files[0])))
    lines = [f"# rocprofv3 --kernel-trace --stats of `tools/time_loss.py --trace --launches {a.launches}`: kernel durations, {KERNEL_BATCH} images, grids {GRIDS}, "
             f"{NC} classes; tracing slows the host: kernel times, not rates"]
    for name in ("assign_targets_kernel", "yolo_loss_kernel", "decode_kernel"):
        d = np.array([e - s for s, e, n in rows if name in n], np.float64) / 1e3
        # the trace run launches nothing else: exactly --launches launches of each kernel per box count, in the order of BOXES
        if len(d) != a.launches * len(BOXES):
            raise SystemExit(f"{name}: {len(d)} launches in the trace, expected {a.launches} x {len(BOXES)} (same --launches as the --trace run?)")
        for k, part in zip(BOXES, np.array_split(d, len(BOXES))):
            lines.append(f"{k:3d} boxes per image  {name:<22s} median {np.median(part):8.2f} us   min {part.min():.2f}   max {part.max():.2f}   ({len(part)} launches)")
    emit(a, lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=16, help="batches per timed window of the end-to-end part")
    ap.add_argument("--launches", type=int, default=50, help="back-to-back launches per timed window of the kernel part")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_stage.txt"), help="append the report to this file")
    ap.add_argument("--skip-streams", action="store_true", help="kernels only")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarize", default="", help="directory of a rocprofv3 --kernel-trace run of --trace")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a)
    if a.trace:
        return trace(a)
    anchors = file_anchors()
    emit(a, [f"# tools/time_loss.py --batches {a.batches} --launches {a.launches} --rounds {a.rounds}"])
    time_kernels(a, anchors)
    if not a.skip_streams:
        time_streams(a)


if __name__ == "__main__":
    main()
