"""The network at class counts other than 80, shared by tests/test_class_counts_host.py and tests/test_class_counts_gpu.py: one
program, one set of synthetic weights (seed 4321, as the 80-class fixtures of tests/conftest.py) and one oracle forward of two
random 64 x 64 images per class count, each made once and left unchanged."""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, "config/models/yolov3/model.yaml")
SEED = 4321
IMAGE_SEED = 77
S = 64


@functools.lru_cache(maxsize=None)
def program(nc):
    from yolo_v3_tf2_amd.graph import load_program
    return load_program(MODEL, nc)


@functools.lru_cache(maxsize=None)
def weights(nc):
    from yolo_v3_tf2_amd.weights import synthetic_weights
    w = synthetic_weights(program(nc), seed=SEED)
    for v in w.values():
        v.setflags(write=False)
    return w


def images(B=2, hw=(S, S)):
    x = np.random.default_rng(IMAGE_SEED).random((B, hw[0], hw[1], 3), dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def oracle_grids(nc):
    """(images [2, 64, 64, 3], the oracle's three grids [2, g, g, 3, 5 + nc] for g = 2, 4, 8)."""
    from oracle import oracle as O
    x = images()
    ref = O.forward(program(nc), weights(nc), x)
    for g in ref:
        g.setflags(write=False)
    return x, ref


def head_ops(p):
    """The three convs that write the net's outputs, coarsest grid first."""
    by_dst = {o.dst: o for o in p.conv_ops()}
    return [by_dst[t] for t in p.outputs]


def head_route(nc):
    """The rule of heads_can_decode (csrc/y3_forward.cpp): the head convs decode their own tile only when their 3 * (5 + nc)
    channels pad (to 32) to exactly 256, i.e. nc in 70..80; every other class count writes fp32 grids and runs the stand-alone
    decode (the composed route)."""
    cout = 3 * (5 + nc)
    return "fused" if (cout + 31) // 32 * 32 == 256 else "composed"
