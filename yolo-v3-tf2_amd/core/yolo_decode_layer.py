"""Host mirror of reference core/yolo_decode_layer.py -- same name and signature, HIP underneath."""
from ..runtime import yolo_decode as _decode


def yolo_decode(model_output_grids, anchors_table, nclasses):
    """model_output_grids: 3 x [B,g,g,3,5+nclasses] CUDA tensors; anchors_table [3,3,2] (normalised w,h,
    row s for grid s) -- or two grids and [2,3,2] for a two-head model (YOLOv3-tiny).  Returns (all_grids_bboxes [B,N,4], all_grids_confidence [B,N,1],
    all_grids_class_probs [B,N,nclasses]) -- reference: core/yolo_decode_layer.py:15-36."""
    return _decode([_to_device(g) for g in model_output_grids], anchors_table, nclasses)


def yolo_decode_hw_host(model_output_grids, anchors_table, nclasses):
    """NumPy float32 restatement of y3_yolo_decode_hw (include/y3.h), no GPU: grids 3 x [B,gh,gw,3,5+nclasses] ->
    (bboxes [B,N,4], confidence [B,N,1], class_probs [B,N,nclasses]), N = 3 * sum gh * gw, rows in the order
    n = off_s + (row * gw + col) * 3 + a.  Every operation rounded to float32 on its own, as the kernel does it:
    sigmoid(t) = 1 / (1 + exp(-t)); x = (sigmoid(tx) + col) / gw, y = (sigmoid(ty) + row) / gh -- each axis by its own
    extent, which for gh == gw is the reference's division by cast([H, W]) (core/yolo_decode_layer.py:5-8) and for
    gh != gw deliberately is not (the reference would divide x by the number of rows); w = exp(tw) * anchor_w,
    h = exp(th) * anchor_h; box = (x - w/2, y - h/2, x + w/2, y + h/2)."""
    import numpy as np
    f32 = np.float32
    one, two = f32(1.0), f32(2.0)
    sigmoid = lambda t: (one / (one + np.exp(-t, dtype=f32))).astype(f32)
    anchors = np.asarray(anchors_table, f32).reshape(-1, 3, 2)      # a row per grid: three, or two for YOLOv3-tiny
    boxes, confs, probs = [], [], []
    for s, grid in enumerate(model_output_grids):
        g = np.asarray(grid, f32)
        B, gh, gw = g.shape[0], g.shape[1], g.shape[2]
        if g.shape[3:] != (3, 5 + nclasses):
            raise ValueError(f"grid {s} must be [B,gh,gw,3,{5 + nclasses}]")
        col = np.arange(gw, dtype=f32)[None, None, :, None]
        row = np.arange(gh, dtype=f32)[None, :, None, None]
        x = ((sigmoid(g[..., 0]) + col).astype(f32) / f32(gw)).astype(f32)
        y = ((sigmoid(g[..., 1]) + row).astype(f32) / f32(gh)).astype(f32)
        w = (np.exp(g[..., 2], dtype=f32) * anchors[s, :, 0]).astype(f32)
        h = (np.exp(g[..., 3], dtype=f32) * anchors[s, :, 1]).astype(f32)
        hw, hh = (w / two).astype(f32), (h / two).astype(f32)
        bb = np.stack([x - hw, y - hh, x + hw, y + hh], axis=-1).astype(f32)
        boxes.append(bb.reshape(B, -1, 4))
        confs.append(sigmoid(g[..., 4]).reshape(B, -1, 1))
        probs.append(sigmoid(g[..., 5:]).reshape(B, -1, nclasses))
    return np.concatenate(boxes, 1), np.concatenate(confs, 1), np.concatenate(probs, 1)


def _to_device(t):
    """Host arrays are accepted like the reference accepts NumPy inputs; they are copied to the GPU."""
    import numpy as np
    import torch
    if isinstance(t, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(t, np.float32)).cuda()
    return t.contiguous()
