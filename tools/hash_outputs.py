#!/usr/bin/env python3
"""SHA-256 of what the conv program produces (three head grids, the fused decode outputs, the packed detections and num_valid of
net.detect) for a seeded batch: two builds of the library (Y3_LIB_PATH) that print the same digests are bit-identical on that plan.
   python tools/hash_outputs.py --dtype bf16 --batch 128          (--dtype f32 | bf16 | f16 | f32x3 | f32x2 | i8; --lanes N overrides the table's;
                                                                   --low-latency: the low-latency plan of an f32, bf16 or f16 net)
--dtype i8: the activation scales are calibrated first on two images of the seeded batch (Net.calibrate_i8, as tools/time_i8.py does)."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import yolo_v3_tf2_amd  # noqa: E402,F401
from yolo_v3_tf2_amd import _lib, runtime  # noqa: E402
from yolo_v3_tf2_amd.core.utils import get_anchors  # noqa: E402
from yolo_v3_tf2_amd.graph import load_program  # noqa: E402
from yolo_v3_tf2_amd.weights import synthetic_weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--image-size", type=int, default=416)
    ap.add_argument("--lanes", type=int, default=0, help="concurrent sub-batches (0: what plan() takes from the tuning table)")
    ap.add_argument("--low-latency", action="store_true", help="the split-K plan of --dtype f32 / bf16 / f16 / i8 (set_low_latency / set_low_latency_bf16 / set_low_latency_f16 / set_low_latency_i8)")
    a = ap.parse_args()
    dtype = runtime.Net._dtype_arg(a.dtype)
    if a.low_latency and dtype not in (_lib.Y3_DTYPE_F32, _lib.Y3_DTYPE_BF16, _lib.Y3_DTYPE_F16, _lib.Y3_DTYPE_I8):
        ap.error("--low-latency: only f32, bf16, f16 and i8 plans split K")
    p = load_program(os.path.join(ROOT, "config/models/yolov3/model.yaml"), 80)
    net = runtime.Net(p)
    net.load_weights(synthetic_weights(p, seed=4321))
    if a.low_latency:   # before plan(): the switch of the chosen dtype
        {_lib.Y3_DTYPE_BF16: net.set_low_latency_bf16, _lib.Y3_DTYPE_F16: net.set_low_latency_f16,
         _lib.Y3_DTYPE_I8: net.set_low_latency_i8}.get(dtype, net.set_low_latency)(True)
    x = torch.from_numpy(np.random.default_rng(77).random((a.batch, a.image_size, a.image_size, 3), dtype=np.float32)).cuda()
    if dtype == _lib.Y3_DTYPE_I8:
        net.calibrate_i8(x[:2].contiguous())
    net.plan(a.batch, a.image_size, dtype)
    if a.lanes:   # after plan(): it sets the lane count from the tuning table
        net.set_lanes(a.lanes)
    anchors = get_anchors(os.path.join(ROOT, "datasets/coco2012/anchors.txt")).astype(np.float32)
    outs = list(net.forward(x)) + list(net.forward_decode(x, anchors)) + list(net.detect(x, anchors, 100, 0.5, 0.1))
    torch.cuda.synchronize()
    for i, t in enumerate(outs):
        print(f"DIGEST {i} {tuple(t.shape)} {hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()}")


if __name__ == "__main__":
    main()
