#!/usr/bin/env python3
"""What int8 costs in accuracy, measured on the CPU (no GPU, no library): the NumPy restatement of the int8 scheme
(yolo_v3_tf2_amd/quant.py, bit-identical to the device by tests/test_i8_gpu.py) against the fp32 oracle.

  * calibration from the fp32 oracle's activations on the same input: absmax, or a percentile of |x|, per tensor;
  * the network behind the cut (quant.forward_i8) fed the fp16 oracle's boundary tensor, as the device feeds it;
  * head-logit relative L2 against the fp32 oracle; with --image: the largest score deviation and the class flips among the
    candidates the fp32 oracle scores above 0.1.

    python tools/i8_accuracy.py                      # synthetic network, 2 x 96^2, input seed 1234: the figures of DESIGN.md section 7, "int8 plans"
    python tools/i8_accuracy.py --image datasets/coco2012/images/girl.png --size 416
    python tools/i8_accuracy.py --model tiny         # YOLOv3-tiny (Net.set_pools_i8): the figures of DESIGN.md, "YOLOv3-tiny in int8"

--model tiny: the fp32 side is a node walker over the tiny program from the oracle's layers and the package's NumPy max-pool (the oracle's
own forward has no pool), the fp16 side the same walker with fp16 weights and every conv output rounded to fp16; calibration also takes
the tensors the int8 aux ops write, and every class of quant.scale_classes its largest scale.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import yolo_v3_tf2_amd  # noqa: E402,F401
from oracle import oracle as O  # noqa: E402
from yolo_v3_tf2_amd import quant  # noqa: E402


def round_f16(a):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(a, np.float32).astype(np.float16).astype(np.float32)


def rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))


def calibrate_cpu(program, kept, percentile):
    """Scales from the fp32 activations `kept` {tensor id: array}, as Net.calibrate_i8 forms them on the device."""
    scales = [0.0] * len(program.tensors)
    for t, x in kept.items():
        a = np.abs(x).ravel()
        if percentile >= 100.0:
            m = float(a.max())
        else:
            k = min(a.size, max(1, int(np.ceil(a.size * percentile / 100.0))))
            m = float(np.partition(a, k - 1)[k - 1])
        scales[t] = quant.scale_from_absmax(m)
    return quant.equalize_concat(program, scales)


def walk(program, weights, x, f16=False):
    """{tensor id: fp32 NHWC} of every node of a program with max-pools, at the real widths.  f16: what an fp16 plan stores -- the
    weights of every conv but the Cin = 3 one and every conv output rounded to fp16 (pools, up-sample and concat select or move)."""
    from yolo_v3_tf2_amd.maxpool import maxpool2x2_ref
    vals = {program.input_tensor: np.ascontiguousarray(x, np.float32)}
    for n in program.nodes:
        a = vals[n.inputs[0]]
        if n.kind == "conv":
            w = {k: v for k, v in weights.items() if k.startswith(f"conv{n.conv_index}.")}
            if f16 and a.shape[-1] != 3:
                w[f"conv{n.conv_index}.w"] = round_f16(w[f"conv{n.conv_index}.w"])
            y = O.conv_block(a, w, n.conv_index, n.size, n.stride, n.bn, n.leaky)
            y = round_f16(y) if f16 else y
        elif n.kind == "maxpool":
            y = maxpool2x2_ref(a, n.stride)
        elif n.kind == "add":
            y = O.add(a, vals[n.inputs[1]])
            y = round_f16(y) if f16 else y
        elif n.kind == "upsample":
            y = O.upsample2x(a)
        elif n.kind == "concat":
            y = O.concat(a, vals[n.inputs[1]])
        elif n.kind == "yolo":
            y = a.reshape(a.shape[0], a.shape[1], a.shape[2], 3, a.shape[3] // 3)
        else:
            raise ValueError(n.kind)
        vals[n.output] = y
    return vals


def measure_pooled(program, weights, x, percentiles=(100.0, 99.99)):
    """measure() for a program with max-pools (YOLOv3-tiny, Net.set_pools_i8): -> {"f32": fp32 head grids, percentile: (int8 grids,
    [rel L2 per head])}."""
    cut = quant.first_i8_conv(program)
    convs = program.conv_ops()
    aux, _ = quant.i8_aux_ops(program, cut)
    crossing = quant.crossing_tensors(program, cut)
    need = {o.dst for o in convs[cut:] if not quant.writes_f32(program, o)} | {o.dst for o in aux} | set(crossing)
    v32 = walk(program, weights, x)
    v16 = walk(program, weights, x, f16=True)
    g32 = [v32[t].reshape(v32[t].shape[0], v32[t].shape[1], v32[t].shape[2], 3, -1) for t in program.outputs]
    out = {"f32": g32}
    for pc in percentiles:
        scales = calibrate_cpu(program, {t: v32[t] for t in need}, pc)
        boundary = {t: quant.quantize(v16[t], scales[t]) for t in crossing}
        t8 = quant.forward_i8(program, weights, scales, boundary, cut)
        grids = [t8[t].reshape(g.shape) for t, g in zip(program.outputs, g32)]
        out[pc] = (grids, [rel_l2(a, b) for a, b in zip(grids, g32)])
    return out


def measure(program, weights, x, percentiles=(100.0, 99.99)):
    """-> {"f32": fp32 oracle grids, percentile: (int8 grids, [rel L2 per head])}."""
    convs = program.conv_ops()
    cut = quant.first_i8_conv(program)
    behind = {o.dst for o in convs[cut:]}
    crossing = sorted({t for o in convs[cut:] for t in (o.src0, o.src1, o.residual) if t >= 0 and t not in behind})
    need = {o.dst for o in convs[cut:] if not quant.writes_f32(program, o)} | set(crossing)
    g32, kept32 = O.forward(program, weights, x, keep=need)
    original = O.round_bf16
    O.round_bf16 = round_f16                     # the oracle's 16-bit mode with fp16 roundings: what runs before the cut
    try:
        _, kept16 = O.forward(program, weights, x, keep=set(crossing), bf16=True)
    finally:
        O.round_bf16 = original
    out = {"f32": g32}
    for pc in percentiles:
        scales = calibrate_cpu(program, kept32, pc)
        boundary = {t: quant.quantize(kept16[t], scales[t]) for t in crossing}
        t8 = quant.forward_i8(program, weights, scales, boundary, cut)
        grids = [t8[t].reshape(g.shape) for t, g in zip(program.outputs, g32)]
        out[pc] = (grids, [rel_l2(a, b) for a, b in zip(grids, g32)])
    return out


def scores_of(grids, anchors, nc):
    _, conf, probs = O.yolo_decode(grids, anchors, nc)
    s = conf * probs
    return s.max(axis=-1), s.argmax(axis=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image", default=None)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--seed", type=int, default=4321, help="synthetic weights")
    ap.add_argument("--model", choices=("yolov3", "tiny"), default="yolov3")
    args = ap.parse_args()
    from yolo_v3_tf2_amd.core.utils import get_anchors
    from yolo_v3_tf2_amd.graph import load_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    tiny = args.model == "tiny"
    program = load_program(os.path.join(ROOT, "config/models/yolov3_tiny/model.yaml" if tiny else "config/models/yolov3/model.yaml"), 80)
    weights = synthetic_weights(program, seed=args.seed)
    if args.image:
        img = O.resize_bilinear(O.decode_image_rgb01(args.image), args.size, args.size)
        x = img[None]
    else:
        x = np.random.default_rng(1234).random((2, args.size, args.size, 3), dtype=np.float32)
    r = (measure_pooled if tiny else measure)(program, weights, x)
    anchors = get_anchors(os.path.join(ROOT, "datasets/coco2012/anchors_tiny.txt" if tiny else "datasets/coco2012/anchors.txt")).astype("float32")
    s32, c32 = scores_of(r["f32"], anchors, 80)
    cand = s32 > 0.1
    for pc in (100.0, 99.99):
        grids, rel = r[pc]
        s8, c8 = scores_of(grids, anchors, 80)
        dev = float(np.abs(s8 - s32)[cand].max()) if cand.any() else 0.0
        flips = int((c8 != c32)[cand].sum())
        name = "absmax" if pc >= 100.0 else f"percentile {pc}"
        print(f"int8 ({name}) vs fp32 oracle, {x.shape[0]} x {args.size}^2: head-logit rel L2 " + " ".join(f"{v:.3e}" for v in rel) +
              f"; {int(cand.sum())} candidates above 0.1: largest score deviation {dev:.3e}, class flips {flips}")


if __name__ == "__main__":
    main()
