"""Sliced inference, restated on the host in NumPy: the window grid (y3_tile_grid) and the merge of the tiles' detections
(y3_merge_tile_detections; csrc/tiles.hip and the existing NMS and pack kernels), which the library is held to bit for bit.
No reference counterpart; no GPU, no library call.

A frame is cut into rows x cols overlapping windows, optionally followed by the whole frame as an overview tile.  Every window
goes through the network as an image of its own; its packed rows, still normalised to the network canvas, are mapped to the frame
and the union of all tiles' rows goes through the padded NMS once more.  Each stage is a greedy rule in which no box is affected
by a box scored below it, and the per-tile cap keeps a prefix in score order, so the merged result at a higher score threshold is
the rows with score > t of the merged result at the lowest one (merged_rows_above; DESIGN.md, "Sliced inference")."""
import numpy as np

from .nms_per_class import nms_padded_per_class_ref

MAX_TILES = 64      # y3_tile_grid / y3_merge_tile_detections


def _axis(e, k, ov):
    """One axis of the grid, integers only: (origins [k], window length)."""
    length = -(-(e + (k - 1) * ov) // k)
    return [0 if k == 1 else (i * (e - length)) // (k - 1) for i in range(k)], length


def tile_grid(height, width, rows, cols, overlap_px=0, overview=False):
    """-> int32 [T,4] = (y0, x0, ch, cw): rows x cols windows of a height x width frame in row-major order and, with overview,
    the whole frame (0, 0, height, width) last; T = rows * cols + (1 if overview else 0).  Per axis, with extent e, count k and
    ov = overlap_px: len = ceil_div(e + (k - 1) * ov, k), origin of window i = floor(i * (e - len) / (k - 1)), 0 when k == 1.
    ValueError for what y3_tile_grid refuses: height or width < 1, rows or cols outside [1,8], ov < 0, ov > min(height, width),
    T > 64."""
    h, w, r, c, ov = int(height), int(width), int(rows), int(cols), int(overlap_px)
    T = r * c + (1 if overview else 0)
    if h < 1 or w < 1 or not 1 <= r <= 8 or not 1 <= c <= 8 or ov < 0 or ov > min(h, w) or T > MAX_TILES:
        raise ValueError(f"tile_grid: refused ({h} x {w}, {r} x {c} windows, overlap {ov}, {T} tiles)")
    ys, lh = _axis(h, r, ov)
    xs, lw = _axis(w, c, ov)
    out = [(y, x, lh, lw) for y in ys for x in xs]
    if overview:
        out.append((0, 0, h, w))
    return np.array(out, np.int32).reshape(T, 4)


def _axis_to_frame(x, canvas, lb_len, lb_off, win_off, win_len, frame_len):
    """tile_axis of csrc/tiles.hip on a float32 array: canvas -> window -> frame, every operation rounded on its own."""
    f = np.float32
    u = x if (lb_len == canvas and lb_off == 0) else (x * f(canvas) - f(lb_off)) / f(lb_len)
    if win_off == 0 and win_len == frame_len:
        return u
    return (f(win_off) + u * f(win_len)) / f(frame_len)


def tile_candidates(packed, num_valid, tiles, geoms, frame_hw, n_frames, n_tiles, canvas):
    """What merge_tiles_kernel writes: (boxes [F,T*M,4] float32, scores [F,T*M] float32, classes [F,T*M] int64), candidate
    n = t * M + r; rows r >= num_valid (clamped to [0,M]) are box 0, score 0, class 0."""
    packed = np.ascontiguousarray(packed, np.int32)
    F, T = int(n_frames), int(n_tiles)
    M = packed.shape[1]
    if packed.shape != (F * T, M, 7):
        raise ValueError(f"tile_candidates: packed must be int32 [{F * T},M,7]")
    nv = np.clip(np.asarray(num_valid, np.int64).reshape(F * T), 0, M)
    tiles = np.asarray(tiles, np.int64).reshape(F * T, 4)
    geoms = np.asarray(geoms, np.int64).reshape(F * T, 4)
    frame_hw = np.asarray(frame_hw, np.int64).reshape(F, 2)
    Hc, Wc = (int(canvas),) * 2 if np.ndim(canvas) == 0 else (int(v) for v in canvas)
    boxes = np.zeros((F * T, M, 4), np.float32)
    scores = np.zeros((F * T, M), np.float32)
    classes = np.zeros((F * T, M), np.int64)
    rows = packed[:, :, :5].view(np.float32)
    with np.errstate(all="ignore"):
        for gi in range(F * T):
            n = int(nv[gi])
            (y0, x0, ch, cw), (sh, sw, top, left), (h, w) = (int(v) for v in tiles[gi]), (int(v) for v in geoms[gi]), \
                (int(v) for v in frame_hw[gi // T])
            for k in (0, 2):
                boxes[gi, :n, k] = _axis_to_frame(rows[gi, :n, k], Wc, sw, left, x0, cw, w)
                boxes[gi, :n, k + 1] = _axis_to_frame(rows[gi, :n, k + 1], Hc, sh, top, y0, ch, h)
            scores[gi, :n] = rows[gi, :n, 4]
            classes[gi, :n] = packed[gi, :n, 5]
    return boxes.reshape(F, T * M, 4), scores.reshape(F, T * M), classes.reshape(F, T * M)


def nms_padded_agnostic_ref(boxes, scores, M, T, S):
    """The class-agnostic padded NMS for T > 0: the per-class restatement with every class id equal, which is that rule with its
    one changed predicate always true.  (T <= 0 selects a quirk of TF's tiles that only oracle/ restates.)"""
    return nms_padded_per_class_ref(boxes, scores, np.zeros(np.shape(scores), np.int64), M, T, S)


def merge_tile_detections_ref(packed, num_valid, tiles, geoms, frame_hw, n_frames, n_tiles, canvas, iou_threshold, score_threshold,
                              per_class=False, agnostic_nms=None):
    """Host restatement of y3_merge_tile_detections.  packed int32 [F*T,M,7] and num_valid [F*T]: the tiles' rows as
    y3_net_detect leaves them (tile t of frame f is image f * T + t; boxes normalised to the canvas, not un-letterboxed);
    tiles [F*T,4] = (y0, x0, ch, cw); geoms [F*T,4] = (sh, sw, top, left); frame_hw [F,2]; canvas an int S or (H, W)
    -> (packed int32 [F,M,7], num_valid int32 [F]): the padded NMS (per class with per_class=True) over tile_candidates with
    max_output_size M, then the rows packed as y3_pack_detections packs them, the index word being t * M + r.
    agnostic_nms: the class-agnostic rule to use, f(boxes, scores, M, T, S) -> (sel, nv); by default nms_padded_agnostic_ref."""
    boxes, scores, classes = tile_candidates(packed, num_valid, tiles, geoms, frame_hw, n_frames, n_tiles, canvas)
    M = np.shape(packed)[1]
    if per_class:
        sel, nv = nms_padded_per_class_ref(boxes, scores, classes, M, iou_threshold, score_threshold)
    else:
        sel, nv = (agnostic_nms or nms_padded_agnostic_ref)(boxes, scores, M, iou_threshold, score_threshold)
    out = np.zeros((int(n_frames), M, 7), np.int32)
    for f, n in enumerate(nv):
        idx = sel[f, :n]
        out[f, :n, :4] = boxes[f, idx].view(np.int32)
        out[f, :n, 4] = scores[f, idx].view(np.int32)
        out[f, :n, 5] = classes[f, idx].astype(np.int32)
        out[f, :n, 6] = idx
    return out, np.asarray(nv, np.int32)


def merged_rows_above(packed, num_valid, threshold):
    """The rows with score > threshold of merged (or any packed) results, kept in order and zero padded: what the merge gives at
    that higher score threshold when the tiles were detected at it as well (the one-pass property)."""
    packed = np.asarray(packed, np.int32)
    out, nv = np.zeros_like(packed), np.zeros(len(packed), np.int32)
    for f, n in enumerate(np.asarray(num_valid)):
        rows = packed[f, :n]
        keep = rows[rows[:, 4].view(np.float32) > np.float32(threshold)]
        out[f, :len(keep)], nv[f] = keep, len(keep)
    return out, nv
