#!/usr/bin/env python3
"""Sliced inference of 1920x1080 frames: frames/s of three routes on the same seeded uint8 frames, 416^2 canvas, 2 x 3 windows
overlapping by 64 pixels + the whole-frame overview (7 tile images per frame), fp32 and bf16, 8 frames per batch.

  untiled    (a) Net.detect_stream(letterbox=True): the frame shrunk 4.6 x onto the canvas, one image per frame
  host       (b) what the feature replaces: every window cropped in NumPy (the overlapping pixels are packed and uploaded several
                 times), Net.detect_stream(letterbox=True) on the 56 crops, then the boxes mapped to the frame and merged in NumPy
                 (tiles.merge_tile_detections_ref on identity geometries: detect_stream has already un-letterboxed the rows)
  tiled      (c) Net.detect_stream(letterbox=True) with net.tiles = (2, 3, 64, True): frames uploaded once, windows cut by
                 preprocess_batch_kernel, merge_tiles_kernel + the existing NMS and pack on the device
  resident   Net.detect on 56 tile images already on the device, as frames/s (images/s / 7): what 7 x the images cost, the bound of (c)

IMAGE DECODE IS EXCLUDED.  Every route is warmed up; a timed window ends in a synchronise and lasts about --window seconds; the routes
alternate within one process, --rounds rounds; median and spread (max - min) per route.  Then the latency of ONE frame (7 tile images:
upload, preprocess_tiles, y3_net_detect, y3_merge_tile_detections, read-back, every call made by hand and ended by a synchronise) with
the low-latency plan off and on.

  python tools/time_tiled.py [--out profiles/tiled.txt]
  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/time_tiled.py --kernels-only
  python tools/time_tiled.py --summarize DIR [--out profiles/tiled_kernels.txt]
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

S, FRAME, TILES, B, M, IOU, SCORE = 416, (1080, 1920, 3), (2, 3, 64, True), 8, 100, 0.5, 0.1
T = TILES[0] * TILES[1] + int(TILES[3])
DTYPES = ("f32", "bf16")


def frames(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, FRAME, dtype=np.uint8) for _ in range(n)]


def timed(fn, k):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(k)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def make_net(program, weights, dtype, batch, low_latency=False):
    from yolo_v3_tf2_amd import _lib, runtime
    net = runtime.Net(program)
    net.load_weights(weights)
    if low_latency:
        (net.set_low_latency if dtype == "f32" else net.set_low_latency_bf16)(True)
    net.plan(batch, S, {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16}[dtype])
    return net


def host_route(net, imgs, anchors, windows, k=1):
    """(b) for k batches of the same frames -> the merged (packed, num_valid) per frame of the last batch.  The windows are cropped anew
    for every batch, inside the stream's generator, so the cropping overlaps the device like the packing of the other routes does."""
    from yolo_v3_tf2_amd import runtime, tiles as TL
    crop = lambda: [np.ascontiguousarray(f[y0:y0 + ch, x0:x0 + cw]) for f in imgs for y0, x0, ch, cw in windows]
    identity = np.tile(np.array([S, S, 0, 0], np.int32), (len(imgs) * T, 1))      # rows already in crop coordinates
    tiled_windows, frame_hw, merged = np.tile(windows, (len(imgs), 1)), [f.shape[:2] for f in imgs], None
    for packed, nv in net.detect_stream((crop() for _ in range(k)), anchors, M, IOU, SCORE, letterbox=True, max_batch=len(imgs) * T,
                                        max_blob_bytes=runtime.packed_nbytes(crop())):
        merged = TL.merge_tile_detections_ref(packed, nv, tiled_windows, identity, frame_hw, len(imgs), T, S, IOU, SCORE)
    return merged


def run_dtype(dtype, a, anchors, program, weights, lines):
    import torch
    from yolo_v3_tf2_amd import input_stage, runtime, tiles as TL
    imgs = frames(B, a.seed)
    windows = TL.tile_grid(FRAME[0], FRAME[1], *TILES)
    net_a, net_c = make_net(program, weights, dtype, B), make_net(program, weights, dtype, B * T)
    blob, descs = runtime.pack_images(imgs, 1, letterbox=True)
    tdescs, _ = input_stage.tile_descs(imgs, descs, *TILES)
    resident = torch.empty((B * T, S, S, 3), device="cuda")
    input_stage.preprocess_tiles(torch.from_numpy(blob).cuda(), tdescs, resident)

    def untiled(k):
        for _ in net_a.detect_stream([imgs] * k, anchors, M, IOU, SCORE, letterbox=True):
            pass

    def host(k):
        host_route(net_c, imgs, anchors, windows, k)

    def tiled(k):
        net_c.tiles = TILES
        try:
            for _ in net_c.detect_stream([imgs] * k, anchors, M, IOU, SCORE, letterbox=True):
                pass
        finally:
            net_c.tiles = None      # routes (b) and the resident one run on the same net, untiled

    def resident56(k):
        for _ in range(k):
            net_c.detect(resident, anchors, M, IOU, SCORE)

    routes = {"untiled": untiled, "host": host, "tiled": tiled, "resident": resident56}
    # (b) and (c) before either is timed: the same counts, the same boxes up to the last bits (the host route un-letterboxes an axis that
    # fills the canvas as x * 416 / 416, the device merge copies it)
    want = host_route(net_c, imgs, anchors, windows)
    net_c.tiles = TILES
    (got,) = list(net_c.detect_stream([imgs], anchors, M, IOU, SCORE, letterbox=True))
    net_c.tiles = None
    plain = list(net_a.detect_stream([imgs], anchors, M, IOU, SCORE, letterbox=True))[0]
    same_nv = np.array_equal(got[1], want[1])
    err = float(np.abs(got[0][..., :5].view(np.float32) - want[0][..., :5].view(np.float32)).max()) if same_nv else float("nan")
    per_window, rates = {}, {n: [] for n in routes}
    for n, fn in routes.items():
        fn(2)
        per_window[n] = max(2, int(np.ceil(a.window / (timed(fn, 2) / 2))))
    for r in range(a.rounds):
        for n in (list(routes) if r % 2 == 0 else list(routes)[::-1]):
            rates[n].append(per_window[n] * B / timed(routes[n], per_window[n]))
    med = {n: float(np.median(v)) for n, v in rates.items()}
    lines.append(f"\n## {dtype}, {B} frames of {FRAME[1]}x{FRAME[0]} per batch, {T} tile images per frame, {S}^2 canvas, frames/s (median, spread = max - min, rounds)")
    names = {"untiled": "(a) untiled letterboxed", "host": "(b) host crops + NumPy merge", "tiled": "(c) detect_stream, net.tiles set",
             "resident": "    resident Net.detect / 7"}
    for n in routes:
        lines.append(f"{names[n]:<30s} {med[n]:9.1f}  (spread {max(rates[n]) - min(rates[n]):.1f}; {', '.join(f'{x:.1f}' for x in rates[n])}; "
                     f"{per_window[n]} batches per window)")
    worst_c, best_b = min(rates["tiled"]), max(rates["host"])
    lines.append(f"(c) / (b) {med['tiled'] / med['host']:.2f}; slowest (c) window {worst_c:.1f} vs fastest (b) window {best_b:.1f}: "
                 f"(c) >= (b) in every window: {worst_c >= best_b}")
    lines.append(f"(a) / (c) {med['untiled'] / med['tiled']:.2f} (7 tile images per frame); (c) / resident bound {med['tiled'] / med['resident']:.2f}")
    lines.append(f"valid rows per frame: untiled {plain[1].tolist()}, tiled {got[1].tolist()}; (b) and (c) agree in num_valid: {same_nv}, "
                 f"largest difference of a box or score word {err:.3g}")
    lines.append(f"uploaded per batch: (b) {sum(w[2] * w[3] * 3 for w in windows) * B / 1e6:.1f} MB of crops, (c) {blob.size / 1e6:.1f} MB of frames")
    print("\n".join(lines[-8:]), flush=True)
    del net_a, net_c
    torch.cuda.empty_cache()


def latency(dtype, a, anchors, program, weights, lines):
    """One frame, 7 tile images, every call by hand, host clock around work that ends in a synchronise."""
    import torch
    from yolo_v3_tf2_amd import input_stage, ops, runtime
    img = frames(1, a.seed)
    pinned = torch.empty(runtime.packed_nbytes(img), dtype=torch.uint8, pin_memory=True)
    blob, descs = runtime.pack_images(img, 1, out=pinned.numpy(), letterbox=True)
    tdescs, windows = input_stage.tile_descs(img, descs, *TILES)
    geoms = input_stage.tile_letterbox_geometries(tdescs, S)
    blob_dev = torch.empty_like(pinned, device="cuda")
    batch = torch.empty((T, S, S, 3), device="cuda")
    out = (torch.empty((1, M, 7), dtype=torch.int32, device="cuda"), torch.empty((1,), dtype=torch.int32, device="cuda"))
    ws = torch.empty(ops.merge_tiles_workspace_bytes(1, T, M), dtype=torch.uint8, device="cuda")
    host_rows = torch.empty((1, M, 7), dtype=torch.int32, pin_memory=True)
    res = {}
    nets = {ll: make_net(program, weights, dtype, T, low_latency=ll) for ll in (False, True)}

    def once(net):
        blob_dev.copy_(pinned, non_blocking=True)
        input_stage.preprocess_tiles(blob_dev, tdescs, batch)
        packed, nv = net.detect(batch, anchors, M, IOU, SCORE)
        ops.merge_tile_detections(packed, nv, windows, geoms, [FRAME[:2]], S, IOU, SCORE, out=out, ws=ws)
        host_rows.copy_(out[0], non_blocking=True)
        torch.cuda.synchronize()

    for net in nets.values():
        for _ in range(5):
            once(net)
    for r in range(a.rounds):
        for ll in ((False, True) if r % 2 == 0 else (True, False)):
            t = []
            for _ in range(a.latency_reps):
                t0 = time.perf_counter()
                once(nets[ll])
                t.append((time.perf_counter() - t0) * 1e3)
            res.setdefault(ll, []).append(float(np.median(t)))
    for ll in (False, True):
        v = res[ll]
        lines.append(f"{dtype} one frame -> merged rows on the host, 7 tile images, low-latency plan {'on ' if ll else 'off'}: {np.median(v):7.3f} ms "
                     f"(spread {max(v) - min(v):.3f}; medians of {a.latency_reps} calls per round: {', '.join(f'{x:.3f}' for x in v)})")
    print("\n".join(lines[-2:]), flush=True)


def kernels_only(a, anchors, program, weights):
    """For a rocprofv3 --kernel-trace run: phase 1 the untiled stream, a synchronise, phase 2 the tiled stream; bf16, 8 frames per batch."""
    import torch
    imgs = frames(B, a.seed)
    net_a, net_c = make_net(program, weights, "bf16", B), make_net(program, weights, "bf16", B * T)
    for _ in net_a.detect_stream([imgs] * (a.kernel_reps + 2), anchors, M, IOU, SCORE, letterbox=True):
        pass
    torch.cuda.synchronize()
    net_c.tiles = TILES
    for _ in net_c.detect_stream([imgs] * (a.kernel_reps + 2), anchors, M, IOU, SCORE, letterbox=True):
        pass
    torch.cuda.synchronize()
    print(f"kernels-only run done: {a.kernel_reps + 2} untiled batches, then {a.kernel_reps + 2} tiled batches of {B} frames, bf16")


def summarize(a):
    files = glob.glob(os.path.join(a.summarize, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {a.summarize}")
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"])
                  for r in csv.DictReader(open(files[0])))
    # one kernel name serves both phases: only the untiled phase launches unletterbox_kernel, and the tiled phase begins at the first
    # preprocess_batch_kernel launch after the last of those
    last_untiled = max(s for s, _, n in rows if "unletterbox_kernel" in n)
    first_tiled = next(s for s, _, n in rows if "preprocess_batch_kernel" in n and s > last_untiled)
    groups = {k: [] for k in ("preprocess_batch_kernel (8 frames -> 8 images)", "nms_kernel, untiled (8 x 10647 boxes)",
                              "preprocess_batch_kernel (8 frames -> 56 images)", "nms_kernel, per tile (56 x 10647 boxes)", "merge_tiles_kernel (56 x 100 rows)",
                              "nms_kernel, merge (8 x 700 candidates)", "pack_kernel, merge", "unletterbox_kernel, untiled")}
    after_merge = 0
    for s, d, n in rows:
        if "preprocess_batch_kernel" in n:
            groups[f"preprocess_batch_kernel (8 frames -> {56 if s >= first_tiled else 8} images)"].append(d)
        elif "merge_tiles_kernel" in n:
            groups["merge_tiles_kernel (56 x 100 rows)"].append(d)
            after_merge = 2
        elif "unletterbox_kernel" in n:
            groups["unletterbox_kernel, untiled"].append(d)
        elif "nms_kernel" in n:
            if after_merge == 2:
                groups["nms_kernel, merge (8 x 700 candidates)"].append(d)
                after_merge = 1
            else:
                groups["nms_kernel, per tile (56 x 10647 boxes)" if s >= first_tiled else "nms_kernel, untiled (8 x 10647 boxes)"].append(d)
        elif "pack_kernel" in n and after_merge == 1:
            groups["pack_kernel, merge"].append(d)
            after_merge = 0
    lines = ["# rocprofv3 --kernel-trace --stats of `tools/time_tiled.py --kernels-only`: bf16, 8 frames of 1920x1080x3 uint8 per batch, 416^2 canvas,",
             "# untiled letterboxed stream, then the tiled stream (2 x 3 windows, overlap 64, + overview: 56 tile images per batch).  Kernel durations,",
             "# median over the launches after the first two batches of each phase; tracing slows the host, the kernels are not affected.",
             f"{'kernel':<52s} {'launches':>8s} {'median us':>10s} {'min us':>8s} {'max us':>8s}"]
    for k, v in groups.items():
        v = v[2:]
        if v:
            lines.append(f"{k:<52s} {len(v):>8d} {np.median(v) / 1e3:10.2f} {min(v) / 1e3:8.2f} {max(v) / 1e3:8.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window")
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--out", default="")
    ap.add_argument("--dtype", default="", help="f32 or bf16 only (default: both)")
    ap.add_argument("--latency-reps", type=int, default=30)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--summarize", default="", help="directory of a rocprofv3 --kernel-trace run of --kernels-only")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a)
    import yolo_v3_tf2_amd  # noqa: F401
    from yolo_v3_tf2_amd import _lib
    from yolo_v3_tf2_amd.core.utils import get_anchors
    from yolo_v3_tf2_amd.graph import load_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    _lib.require_gpu()       # a measurement path that finds no GPU fails
    program = load_program(os.path.join(ROOT, "config/models/yolov3/model.yaml"), 80)
    weights = synthetic_weights(program, seed=4321)
    anchors = get_anchors(os.path.join(ROOT, "datasets/coco2012/anchors.txt")).astype(np.float32)
    if a.kernels_only:
        return kernels_only(a, anchors, program, weights)
    lines = ["# tools/time_tiled.py: sliced inference of 1920x1080x3 uint8 frames, 2 x 3 windows overlapping by 64 pixels + overview, 416^2 canvas,",
             f"# synthetic weights, {M} boxes, IoU {IOU}, score {SCORE}; one process, routes alternated, {a.rounds} rounds of ~{a.window} s; image decode excluded."]
    for dtype in DTYPES:
        if a.dtype in ("", dtype):
            run_dtype(dtype, a, anchors, program, weights, lines)
    lines.append("\n## latency of one frame (host clock around upload, preprocess_tiles, y3_net_detect, y3_merge_tile_detections, read-back, synchronise)")
    for dtype in DTYPES:
        if a.dtype in ("", dtype):
            latency(dtype, a, anchors, program, weights, lines)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
