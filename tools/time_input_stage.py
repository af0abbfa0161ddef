#!/usr/bin/env python3
"""Frames in host memory -> detections: images/s of three routes on the same seeded uint8 frames.

  resident   Net.detect on a batch already on the device: the ceiling, the quantity bench.py's headline reports
  per-image  per image torch.from_numpy(u8).cuda() + preprocess_image, then Net.detect, then a blocking read-back of its
             outputs: the call pattern of inference.py before the batched stage.  (inference.py also read the full
             [B,N,*] boxes / classes / scores back; that is NOT included, so this route is an upper bound of that path.)
  pipelined  Net.detect_stream: pack into pinned memory, one copy + preprocess_batch on a copy stream, overlapped with the
             previous batch's detect; only the packed rows come back

at 64 x 416^2 fp32 and 128 x 416^2 bf16, on two frame sets drawn from default_rng(seed): 640x480x3 frames, and a ragged set
(100x37 ... 1920x1080, some with four channels).  IMAGE DECODE IS EXCLUDED: every route starts from decoded uint8 arrays.
Every shape is warmed up; a timed window ends in a synchronise and lasts about --window seconds; the routes alternate,
--rounds rounds; median and spread (max - min) per route.

  python tools/time_input_stage.py [--out profiles/input_stage.json]
  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/time_input_stage.py --kernels-only
  python tools/time_input_stage.py --summarize DIR [--out profiles/input_stage_kernel_stats.txt]
  rocprofv3 --kernel-trace --memory-copy-trace -d DIR2 -o run --output-format csv -- python tools/time_input_stage.py --trace-pipelined
  python tools/time_input_stage.py --summarize-trace DIR2 [--out profiles/input_stage_pipeline_trace.txt]

--letterbox (with any of the above): the frames keep their aspect ratio (zero padding, Y3_IMAGE_LETTERBOX) and the detections
come back in frame coordinates; --kernels-only then also runs unletterbox_kernel on 64 x 100 valid rows per repetition.
--letterbox --rect: the net is planned for runtime.rect_canvas of the frame size (--frame HxW, default 480x640) instead of the
416^2 square, with the anchors rescaled to that canvas (runtime.rect_anchors); the uniform frame set only.
--letterbox --compare-rect [--out profiles/rect_canvas.txt]: the square and the rect plan in ONE process, pipelined route,
windows alternated; images/s of both, their ratio, the FLOP ratio beside it and the per-conv times of both plans.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBS = 8.0          # MI355X HBM3E, specification (MI355X_MICROARCH.md)
HBM_MEASURED_TBS = 6.29     # float4 copy measured there
S = 416
CONFIGS = (("f32", 64), ("bf16", 128))
RAGGED_SHAPES = [(100, 37, 3), (480, 640, 3), (1080, 1920, 3), (375, 500, 4), (720, 1280, 3), (416, 416, 3), (812, 667, 4), (240, 320, 3)]


def frames(kind, n, seed, frame=(480, 640)):
    """kind "640x480": n frames of `frame` (H, W), three channels; "ragged": the mixed set."""
    rng = np.random.default_rng(seed)
    shapes = [(*frame, 3)] * n if kind == "640x480" else [RAGGED_SHAPES[i % len(RAGGED_SHAPES)] for i in range(n)]
    return [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]


def algorithmic_bytes(images, canvas=(S, S)):
    """Source bytes read + Hc*Wc*12 written, per image, summed."""
    return int(sum(im.nbytes + canvas[0] * canvas[1] * 12 for im in images))


def timed(fn, batches_per_window):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(batches_per_window)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run_config(dtype, B, a, anchors, program, weights, canvas=(S, S), frame=(480, 640)):
    """canvas: the plan's (H, W) -- the 416^2 square, or (--rect) runtime.rect_canvas of `frame` with `anchors` rescaled to it by
    the caller; a rectangular canvas runs the uniform frame set only."""
    import torch
    from yolo_v3_tf2_amd import _lib, runtime
    net = runtime.Net(program)
    net.load_weights(weights)
    Hc, Wc = canvas
    rect = Hc != Wc
    net.plan(B, canvas if rect else Hc, {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16}[dtype])
    out = {}
    for kind in (("640x480",) if rect else ("640x480", "ragged")):
        imgs = frames(kind, B, a.seed, frame)
        lb = a.letterbox
        blob, descs = runtime.pack_images(imgs, 1, letterbox=lb)
        geoms = runtime.letterbox_geometries(descs, canvas)
        resident_batch = torch.empty((B, Hc, Wc, 3), device="cuda")
        runtime.preprocess_batch(torch.from_numpy(blob).cuda(), descs, resident_batch)

        def detect(batch):
            packed, nv = net.detect(batch, anchors, 100, 0.5, 0.1)
            if lb:
                runtime.unletterbox_detections(packed, nv, geoms, canvas)
            return packed, nv

        def resident(k):
            for _ in range(k):
                detect(resident_batch)

        def per_image(k):
            for _ in range(k):
                batch = torch.empty((B, Hc, Wc, 3), device="cuda")
                for slot, u8 in enumerate(imgs):
                    runtime.preprocess_image(torch.from_numpy(u8).cuda(), batch, slot, letterbox=lb)
                packed, nv = detect(batch)
                packed.cpu().numpy(), nv.cpu().numpy()

        def pipelined(k):
            for _ in net.detect_stream([imgs] * k, anchors, 100, 0.5, 0.1, mode=1, depth=2, letterbox=lb):
                pass

        routes = {"resident": resident, "per_image": per_image, "pipelined": pipelined}
        # the three routes must agree before any of them is timed
        ref = detect(resident_batch)
        ref = (ref[0].cpu().numpy(), ref[1].cpu().numpy())
        got = list(net.detect_stream([imgs], anchors, 100, 0.5, 0.1, letterbox=lb))[0]
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), "pipelined route differs from the resident one"
        per_window = {}
        for name, fn in routes.items():          # warm-up, then size the window from a short timing
            fn(2)
            per_window[name] = max(3, int(np.ceil(a.window / (timed(fn, 3) / 3))))
        rates = {name: [] for name in routes}
        for r in range(a.rounds):
            order = list(routes) if r % 2 == 0 else list(routes)[::-1]
            for name in order:
                k = per_window[name]
                rates[name].append(k * B / timed(routes[name], k))
        t0 = time.perf_counter()
        for _ in range(5):
            runtime.pack_images(imgs, 1, out=blob, letterbox=lb)
        pack_ms = (time.perf_counter() - t0) / 5 * 1e3
        res = {"images_per_batch": B, "source_mbytes_per_batch": round(blob.size / 1e6, 2), "batches_per_window": per_window,
               "host_pack_ms_per_batch": round(pack_ms, 2), "host_pack_images_per_s": round(B / pack_ms * 1e3, 1)}
        if lb:      # the one host call the letterbox route adds per batch, next to the packing it follows
            t0 = time.perf_counter()
            for _ in range(200):
                runtime.letterbox_geometries(descs, canvas)
            res["host_geometry_ms_per_batch"] = round((time.perf_counter() - t0) / 200 * 1e3, 4)
        for name, v in rates.items():
            res[name] = {"images_per_s_median": round(float(np.median(v)), 1), "spread": round(float(max(v) - min(v)), 1),
                         "rounds": [round(float(x), 1) for x in v]}
        res["pipelined_over_per_image"] = round(res["pipelined"]["images_per_s_median"] / res["per_image"]["images_per_s_median"], 3)
        res["pipelined_over_resident"] = round(res["pipelined"]["images_per_s_median"] / res["resident"]["images_per_s_median"], 3)
        res["pipelined_minus_per_image_over_per_image_spread"] = round(
            (res["pipelined"]["images_per_s_median"] - res["per_image"]["images_per_s_median"]) / max(res["per_image"]["spread"], 1e-9), 1)
        out[kind] = res
        print(f"{dtype} {B} x {Hc}x{Wc}, {kind if kind == 'ragged' else f'{frame[1]}x{frame[0]}'} frames{' letterboxed' if lb else ''} (decode excluded): " + ", ".join(
            f"{n} {res[n]['images_per_s_median']:.0f} img/s (spread {res[n]['spread']:.0f})" for n in routes) +
            f"; pipelined / per-image {res['pipelined_over_per_image']:.2f}, pipelined / resident {res['pipelined_over_resident']:.2f}; "
            f"host packing alone {res['host_pack_images_per_s']:.0f} img/s" +
            (f", geometry call {res['host_geometry_ms_per_batch'] * 1e3:.1f} us per batch" if lb else ""), flush=True)
    return out


def compare_rect(a, anchors, program, weights):
    """Square letterbox plan against the rect_canvas plan of the same frames: one process, the pipelined route of both,
    windows alternated (the square run of the same session is the yardstick); then the per-conv times of both plans."""
    import torch
    from yolo_v3_tf2_amd import _lib, runtime
    lines = ["# tools/time_input_stage.py --letterbox --compare-rect: Net.detect_stream (depth 2, letterbox=True) on uniform uint8 frames,",
             f"# square {S}^2 plan against the runtime.rect_canvas plan, one process, windows alternated, {a.rounds} rounds of ~{a.window} s each,",
             "# median (spread = max - min); image decode excluded.  FLOP ratio = y3_net_flops_per_image(rect) / (square): the bound of the gain.",
             "# The rect plan takes the tile table of the square plan (tuning/<mode>_b<batch>_s416.json); no tile was tuned for it."]
    for frame in ((480, 640), (1080, 1920)):
        canvas = runtime.rect_canvas(*frame, S)
        for dtype, B in CONFIGS:
            if a.dtype not in ("", dtype):
                continue
            imgs = [np.random.default_rng(a.seed).integers(0, 256, (*frame, 3), dtype=np.uint8)] * B
            plans = {}
            for name, size, anc in (("square", S, anchors), ("rect", canvas, runtime.rect_anchors(anchors, S, canvas))):
                net = runtime.Net(program)
                net.load_weights(weights)
                net.plan(B, size, {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16}[dtype])
                plans[name] = (net, anc)

            def route(name):
                net, anc = plans[name]
                def fn(k):
                    for _ in net.detect_stream([imgs] * k, anc, 100, 0.5, 0.1, mode=1, depth=2, letterbox=True):
                        pass
                return fn
            routes = {n: route(n) for n in plans}
            per_window, rates = {}, {n: [] for n in plans}
            for n, fn in routes.items():
                fn(2)
                per_window[n] = max(3, int(np.ceil(a.window / (timed(fn, 3) / 3))))
            for r in range(a.rounds):
                for n in (list(routes) if r % 2 == 0 else list(routes)[::-1]):
                    rates[n].append(per_window[n] * B / timed(routes[n], per_window[n]))
            med = {n: float(np.median(v)) for n, v in rates.items()}
            flops = {n: plans[n][0].flops_per_image() for n in plans}
            fr = flops["rect"] / flops["square"]
            gain, bound = med["rect"] / med["square"], 1.0 / fr
            lines.append(f"\n## {frame[1]}x{frame[0]} frames, {dtype}, {B} per batch: square {S}x{S} vs rect {canvas[0]}x{canvas[1]}")
            for n in plans:
                lines.append(f"{n:<7s} {med[n]:9.1f} images/s  (spread {max(rates[n]) - min(rates[n]):.1f}; rounds {', '.join(f'{x:.1f}' for x in rates[n])})")
            lines.append(f"rect / square images/s {gain:.3f}   FLOP ratio rect / square {fr:.3f} (bound of the gain: x {bound:.3f})   "
                         f"share of the possible gain realised {(gain - 1) / (bound - 1) * 100:.0f} %")
            ms = {}
            for n, (net, _) in plans.items():
                Hc, Wc = net.canvas
                x = torch.rand((B, Hc, Wc, 3), device="cuda")
                net.profile_convs(x)
                ms[n] = np.median([net.profile_convs(x) for _ in range(3)], axis=0)
            lines.append(f"per-conv ms (profile_convs, one lane, median of 3; 0 = runs inside the fused stem launch); sum square {ms['square'].sum():.3f}, rect {ms['rect'].sum():.3f}")
            lines.append(f"{'conv':>4s} {'k':>1s} {'s':>1s} {'cin':>5s} {'cout':>5s} {'div':>3s} {'square ms':>10s} {'rect ms':>9s} {'rect/square':>11s} {'vs FLOP ratio':>13s}")
            for i, o in enumerate(plans["square"][0].conv_ops):
                q = ms["rect"][i] / ms["square"][i] if ms["square"][i] > 0 else 0.0
                lines.append(f"{i:4d} {o.size:1d} {o.stride:1d} {o.cin:5d} {o.cout:5d} {o.out_div:3d} {ms['square'][i]:10.4f} {ms['rect'][i]:9.4f} {q:11.3f} {q / fr:13.3f}")
            del plans, routes
            torch.cuda.empty_cache()
            print("\n".join(lines[-80:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


def kernels_only(a):
    """For a rocprofv3 --kernel-trace run: the batch kernel and the per-image kernel on the same resident frames."""
    import torch
    from yolo_v3_tf2_amd import runtime
    for kind in ("640x480", "ragged"):
        imgs = frames(kind, 64, a.seed)
        blob, descs = runtime.pack_images(imgs, 1, letterbox=a.letterbox)
        blob_dev = torch.from_numpy(blob).cuda()
        singles = [torch.from_numpy(u8).cuda() for u8 in imgs]
        batch = torch.empty((64, S, S, 3), device="cuda")
        if a.letterbox:     # 64 x 100 valid rows of boxes inside the unit square, the shape y3_net_detect hands over
            geoms = runtime.letterbox_geometries(descs, S)
            rows = np.zeros((64, 100, 7), np.int32)
            rows[..., :5] = np.random.default_rng(a.seed).random((64, 100, 5), dtype=np.float32).view(np.int32)
            rows_dev, packed = torch.from_numpy(rows).cuda(), torch.empty((64, 100, 7), dtype=torch.int32, device="cuda")
            nv = torch.full((64,), 100, dtype=torch.int32, device="cuda")
        for _ in range(a.kernel_reps + 2):      # the first two repetitions are warm-up; the summary drops them
            runtime.preprocess_batch(blob_dev, descs, batch)
            torch.cuda.synchronize()
            for slot, t in enumerate(singles):
                runtime.preprocess_image(t, batch, slot, letterbox=a.letterbox)
            torch.cuda.synchronize()
            if a.letterbox:
                packed.copy_(rows_dev)
                runtime.unletterbox_detections(packed, nv, geoms, S)
                torch.cuda.synchronize()
    print(f"kernels-only run done{' (letterboxed)' if a.letterbox else ''} (image decode excluded; frames resident on the device)")


def trace_pipelined(a, anchors, program, weights):
    """For a rocprofv3 kernel + memory-copy trace: the pipelined route alone, bf16, 128 ragged frames per batch."""
    from yolo_v3_tf2_amd import _lib, runtime
    net = runtime.Net(program)
    net.load_weights(weights)
    net.plan(128, S, _lib.Y3_DTYPE_BF16)
    imgs = frames("ragged", 128, a.seed)
    for _ in net.detect_stream([imgs] * 24, anchors, 100, 0.5, 0.1, letterbox=a.letterbox):
        pass
    print("pipelined trace run done: 24 batches of 128 ragged frames, bf16 (image decode excluded)")


def summarize_trace(a):
    """What bounds the pipelined route: per batch (one nms_kernel launch each), the wall time between batches, the time
    with at least one kernel running, and the host-to-device copy, over the last 16 batches of --trace-pipelined."""
    def load(pattern):
        files = glob.glob(os.path.join(a.summarize_trace, "**", pattern), recursive=True)
        return list(csv.DictReader(open(files[0]))) if files else []
    kern = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in load("*kernel_trace.csv"))
    copies = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Direction", "")) for r in load("*memory_copy_trace.csv")]
    marks = [e for _, e, n in kern if "nms_kernel" in n]
    assert len(marks) >= 20, len(marks)
    t0, t1, nb = marks[-17], marks[-1], 16
    busy, cur_s, cur_e = 0, None, None
    for s_, e, _ in kern:
        if e <= t0 or s_ >= t1:
            continue
        s_, e = max(s_, t0), min(e, t1)
        if cur_e is None or s_ > cur_e:
            busy += (cur_e - cur_s) if cur_e is not None else 0
            cur_s, cur_e = s_, e
        else:
            cur_e = max(cur_e, e)
    busy += (cur_e - cur_s) if cur_e is not None else 0
    pre = sum(e - s_ for s_, e, n in kern if "preprocess_batch_kernel" in n and t0 <= s_ < t1)
    h2d = [(e - s_) for s_, e, d in copies if t0 <= s_ < t1 and "HOST_TO_DEVICE" in d.upper() and e - s_ > 200000]
    nbytes = sum(-(-im.nbytes // 16) * 16 for im in frames("ragged", 128, a.seed))
    wall = (t1 - t0) / nb
    lines = ["# rocprofv3 --kernel-trace --memory-copy-trace of `tools/time_input_stage.py --trace-pipelined`: Net.detect_stream, bf16,",
             "# 128 ragged uint8 frames per batch, the last 16 of 24 batches; image decode excluded.  Tracing slows the host: shares, not rates.",
             f"wall time per batch                          {wall / 1e6:8.3f} ms  ({128 / (wall / 1e9):.0f} images/s under the tracer)",
             f"time with at least one kernel running        {busy / nb / 1e6:8.3f} ms  ({busy / (t1 - t0) * 100:.1f} % of the wall time)",
             f"  of which preprocess_batch_kernel           {pre / nb / 1e6:8.3f} ms",
             f"no kernel running                            {(t1 - t0 - busy) / nb / 1e6:8.3f} ms"]
    if h2d:
        lines.append(f"host-to-device copy of the pixel blob        {np.median(h2d) / 1e6:8.3f} ms  ({nbytes / 1e6:.1f} MB: {nbytes / np.median(h2d):.1f} GB/s; "
                     f"{len(h2d)} copies, on the copy stream, overlapped with the previous batch's kernels)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


def summarize(a):
    files = glob.glob(os.path.join(a.summarize, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {a.summarize}")
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"])
                  for r in csv.DictReader(open(files[0])))
    batch = [d for _, d, n in rows if "preprocess_batch_kernel" in n]
    single = [d for _, d, n in rows if "resize_kernel" in n]
    unlb = [d for _, d, n in rows if "unletterbox_kernel" in n]
    reps = a.kernel_reps + 2
    assert len(batch) == 2 * reps and len(single) == 2 * reps * 64, (len(batch), len(single))
    lines = ["# rocprofv3 --kernel-trace --stats of `tools/time_input_stage.py --kernels-only`: 64 uint8 frames -> 64 x 416^2 x 3 fp32,",
             "# frames resident on the device, image decode excluded.  Algorithmic bytes = source bytes read + 416*416*12 written per image." +
             ("  LETTERBOXED (--letterbox)." if a.letterbox else ""),
             f"# HBM peak {HBM_PEAK_TBS} TB/s (specification), {HBM_MEASURED_TBS} TB/s measured with a float4 copy (MI355X_MICROARCH.md).",
             f"# median over {a.kernel_reps} repetitions after 2 warm-up repetitions",
             f"{'frames':<10s} {'kernel':<34s} {'launches':>8s} {'us per 64 images':>17s} {'us per image':>13s} {'GB/s':>9s} {'% of 8 TB/s':>12s}"]
    for i, kind in enumerate(("640x480", "ragged")):
        nbytes = algorithmic_bytes(frames(kind, 64, a.seed))
        b = np.array(batch[i * reps:(i + 1) * reps][2:], np.float64)
        s = np.array(single[i * reps * 64:(i + 1) * reps * 64], np.float64).reshape(reps, 64)[2:].sum(axis=1)
        for name, launches, v in (("preprocess_batch_kernel (1 launch)", 1, b), ("resize_kernel (64 launches, summed)", 64, s)):
            us = float(np.median(v)) / 1e3
            gbs = nbytes / (us * 1e-6) / 1e9
            lines.append(f"{kind:<10s} {name:<34s} {launches:>8d} {us:17.2f} {us / 64:13.3f} {gbs:9.1f} {gbs / (HBM_PEAK_TBS * 1e3) * 100:12.2f}")
        lines.append(f"# {kind}: {nbytes / 1e6:.2f} MB algorithmic; batch kernel time / summed per-image kernel time = {float(np.median(b) / np.median(s)):.3f}")
        if a.letterbox:
            assert len(unlb) == 2 * reps, len(unlb)
            u = np.array(unlb[i * reps:(i + 1) * reps][2:], np.float64)
            lines.append(f"{kind:<10s} {'unletterbox_kernel (64 x 100 rows)':<34s} {1:>8d} {float(np.median(u)) / 1e3:17.2f}")
    lines.append("# kernel time only: the 64 launches of the per-image route also pay 64 launch gaps, which this table leaves out")
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
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--trace-pipelined", action="store_true")
    ap.add_argument("--letterbox", action="store_true", help="aspect-preserving resize + zero pad, detections in frame coordinates")
    ap.add_argument("--rect", action="store_true", help="with --letterbox: plan runtime.rect_canvas of the frame size instead of the square")
    ap.add_argument("--frame", default="480x640", help="HxW of the uniform frame set (default 480x640)")
    ap.add_argument("--compare-rect", action="store_true", help="with --letterbox: square plan against the rect plan, alternated, one process")
    ap.add_argument("--summarize-trace", default="", help="directory of a rocprofv3 kernel + memory-copy trace of --trace-pipelined")
    ap.add_argument("--summarize", default="", help="directory of a rocprofv3 --kernel-trace run of --kernels-only")
    a = ap.parse_args()
    frame = tuple(int(v) for v in a.frame.lower().split("x"))
    if frame != (480, 640) and not a.rect:
        ap.error("--frame applies to --rect runs (the square runs keep the 640x480 set their records were made with)")
    if (a.rect or a.compare_rect) and not a.letterbox:
        ap.error("--rect / --compare-rect need --letterbox")
    if a.summarize:
        return summarize(a)
    if a.summarize_trace:
        return summarize_trace(a)
    import yolo_v3_tf2_amd  # noqa: F401
    from yolo_v3_tf2_amd import _lib
    from yolo_v3_tf2_amd.core.utils import get_anchors
    from yolo_v3_tf2_amd.graph import load_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    _lib.require_gpu()       # a measurement path that finds no GPU fails
    if a.kernels_only:
        return kernels_only(a)
    program = load_program(os.path.join(ROOT, "config/models/yolov3/model.yaml"), 80)
    weights = synthetic_weights(program, seed=4321)
    anchors = get_anchors(os.path.join(ROOT, "datasets/coco2012/anchors.txt")).astype(np.float32)
    if a.trace_pipelined:
        return trace_pipelined(a, anchors, program, weights)
    if a.compare_rect:
        return compare_rect(a, anchors, program, weights)
    doc = {"what": "images/s from decoded uint8 frames in host memory to packed detections on the host; image decode excluded",
           "image_size": S, **({"rect": True, "frame": list(frame)} if a.rect else {}), "rounds": a.rounds, "window_s": a.window, "seed": a.seed, **({"letterbox": True} if a.letterbox else {}),
           "routes": {"resident": "Net.detect on a batch already on the device", "per_image": "per image .cuda() + preprocess_image, Net.detect, blocking read-back",
                      "pipelined": "Net.detect_stream (depth 2)"}}
    for dtype, B in CONFIGS:
        if a.dtype in ("", dtype):
            if a.rect:
                from yolo_v3_tf2_amd import runtime
                canvas = runtime.rect_canvas(*frame, S)
                doc[f"{dtype}_b{B}"] = run_config(dtype, B, a, runtime.rect_anchors(anchors, S, canvas), program, weights, canvas, frame)
            else:
                doc[f"{dtype}_b{B}"] = run_config(dtype, B, a, anchors, program, weights)
    line = json.dumps(doc)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(line)


if __name__ == "__main__":
    main()
