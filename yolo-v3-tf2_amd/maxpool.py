"""The 2x2 max-pool of YOLOv3-tiny, restated in NumPy (include/y3.h, y3_maxpool2x2; csrc/maxpool.hip is the device's).

Keras MaxPooling2D(pool_size=2, strides=s, padding='same') (reference: core/parse_model.py:78-99) on NHWC data:

  * s = 2, even extents: out[y, x] = max over in[2y .. 2y+1, 2x .. 2x+1] (no padding is needed);
  * s = 1: 'same' pads one row below and one column to the right, and the padding never wins a max, so
    out[y, x] = max over in[y .. min(y+1, H-1), x .. min(x+1, W-1)].

TensorFlow's own kernel is not pinned by any test of this project (it is not installed); this file is the statement the
device is held to.  A NaN in a window and the sign of a zero result are unspecified.  No GPU and no library needed."""
from __future__ import annotations

import numpy as np


def maxpool2x2_ref(x: np.ndarray, stride: int) -> np.ndarray:
    """x [B,H,W,C] -> [B,H/stride,W/stride,C]; stride 2 needs even H and W."""
    x = np.asarray(x)
    if x.ndim != 4 or stride not in (1, 2):
        raise ValueError("maxpool2x2_ref: x must be [B,H,W,C] and stride 1 or 2")
    H, W = x.shape[1], x.shape[2]
    if stride == 2:
        if H % 2 or W % 2:
            raise ValueError(f"maxpool2x2_ref: a stride-2 pool needs even extents (got {H} x {W})")
        return np.maximum(np.maximum(x[:, 0::2, 0::2], x[:, 0::2, 1::2]), np.maximum(x[:, 1::2, 0::2], x[:, 1::2, 1::2]))
    below = np.minimum(np.arange(H) + 1, H - 1)
    right = np.minimum(np.arange(W) + 1, W - 1)
    rows = np.maximum(x, x[:, below])
    return np.maximum(rows, rows[:, :, right])
