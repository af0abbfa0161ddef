#!/usr/bin/env python3
"""Write the activation scales an int8 plan needs (dtype: i8 + i8_calibration: FILE in the inference / evaluation YAML) from a directory
of images: every image is resized to the network size as inference does, the fp32 plan runs with its activations kept, and per tensor
the largest |x| over all batches (or the given percentile of |x|, the largest over the batches) divided by 127 is the scale; the two
sources of a concat conv take the larger of theirs, and in a pooled net (YOLOv3-tiny, Net.set_pools_i8) every tensor an aux op writes is
measured too and every class of quant.scale_classes takes its largest scale (runtime.Net.calibrate_i8, quant.py).  Needs a GPU.

    python tools/calibrate_i8.py --images DIR --weights FILE.safetensors --out cal.json [--size 416] [--batch 8] [--percentile 100]
                                 [--model config/models/yolov3/model.yaml] [--classes 80]        (--weights synthetic: seeded random ones)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", required=True)
    ap.add_argument("--weights", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--percentile", type=float, default=100.0)
    ap.add_argument("--model", default=os.path.join(ROOT, "config/models/yolov3/model.yaml"))
    ap.add_argument("--classes", type=int, default=80)
    a = ap.parse_args()

    import torch
    import yolo_v3_tf2_amd  # noqa: F401
    from yolo_v3_tf2_amd import quant, runtime, weights as W
    from yolo_v3_tf2_amd.core.utils import load_image_u8
    from yolo_v3_tf2_amd.graph import load_program

    program = load_program(a.model, a.classes)
    if a.weights == "synthetic":
        w = W.synthetic_weights(program, seed=4321)
    elif a.weights.endswith(".weights"):
        w = W.read_darknet_weights(a.weights, program)
    else:
        w = W.load_weights(a.weights)
    files = sorted(f for f in os.listdir(a.images) if f.lower().endswith((".png", ".jpg", ".jpeg")))
    if not files:
        raise SystemExit(f"no .png / .jpg images in {a.images}")
    net = runtime.Net(program)
    net.load_weights(w)
    net.set_pools_i8(True)      # a pooled net (YOLOv3-tiny): also the scales of the tensors its aux ops write; a net without aux ops: no difference
    worst = [0.0] * len(program.tensors)
    for i in range(0, len(files), a.batch):
        chunk = files[i:i + a.batch]
        batch = torch.empty((len(chunk), a.size, a.size, 3), dtype=torch.float32, device="cuda")
        for k, f in enumerate(chunk):
            runtime.preprocess_image(torch.from_numpy(load_image_u8(os.path.join(a.images, f))).cuda(), batch, k)
        s = net.calibrate_i8(batch, a.percentile)
        worst = [max(u, v) for u, v in zip(worst, s)]
    worst = quant.equalize_concat(program, worst)
    net.set_act_scales(worst)
    net.save_calibration(a.out)
    print(f"{a.out}: {sum(v > 0 for v in worst)} tensor scales from {len(files)} images at {a.size}^2, percentile {a.percentile}")


if __name__ == "__main__":
    main()
