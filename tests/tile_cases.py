"""Shared recipes of tests/test_tiles_host.py and tests/test_tiles_gpu.py (sliced inference): frames and windows for the input
stage, hand-made packed rows for the merge, and a brute-force statement of the two-stage rule.  NumPy only; nothing here needs
the library or a GPU."""
import numpy as np

from yolo_v3_tf2_amd.core.utils import letterbox_geometry

LETTERBOX = 0x100       # Y3_IMAGE_LETTERBOX

# ------------------------------------------------------------------------------------------------ input stage
FRAME_SHAPES = [(97, 131, 3), (64, 48, 4), (1, 1, 3)]
CANVASES = [(64, 64), (64, 96)]
# per frame shape, windows (y0, x0, ch, cw): 1 x 1 (inside and in the last corner), the four corners, odd sizes, the whole frame
WINDOWS = {
    (97, 131, 3): [(0, 0, 1, 1), (96, 130, 1, 1), (50, 60, 1, 1), (0, 0, 33, 47), (0, 84, 33, 47), (64, 0, 33, 47), (64, 84, 33, 47),
                   (13, 29, 61, 5), (40, 3, 2, 127), (0, 0, 97, 131), (1, 1, 96, 130), (0, 0, 97, 1), (96, 0, 1, 131)],
    (64, 48, 4): [(0, 0, 1, 1), (63, 47, 1, 1), (0, 0, 64, 48), (10, 7, 32, 32), (0, 24, 64, 24), (32, 0, 32, 48)],
    (1, 1, 3): [(0, 0, 1, 1)],
}


def frame(shape, mode, seed):
    """mode 0: float32 in [0,1); 1, 2: uint8."""
    rng = np.random.default_rng(seed)
    return rng.random(shape, dtype=np.float32) if mode == 0 else rng.integers(0, 256, shape, dtype=np.uint8)


def input_case(mode, letterbox, seed=0):
    """-> (frames, windows per frame): the three frames in pixel mode `mode` and their WINDOWS."""
    frames = [frame(s, mode, seed + i) for i, s in enumerate(FRAME_SHAPES)]
    return frames, [WINDOWS[s] for s in FRAME_SHAPES]


def crops(frames, windows):
    """The contiguous copies preprocess_batch is given: window k of frame i, in the order the tiles are staged."""
    return [np.ascontiguousarray(f[y0:y0 + ch, x0:x0 + cw]) for f, ws in zip(frames, windows) for y0, x0, ch, cw in ws]


def fits(ch, cw, canvas):
    """Does the letterbox of a ch x cw image fit the canvas?  (A 2 x 127 strip on 64 x 64 does; rounding can say otherwise.)"""
    sh, sw, top, left = letterbox_geometry(ch, cw, *canvas)
    return top >= 0 and left >= 0 and top + sh <= canvas[0] and left + sw <= canvas[1]


# ------------------------------------------------------------------------------------------------ merge
T_IOU, S_LOW = 0.5, 0.05


def window_geoms(windows, canvas, letterbox):
    """int32 [n,4] (sh, sw, top, left) of windows taken as images of their own; the whole canvas without letterbox."""
    if not letterbox:
        return np.tile(np.array([canvas[0], canvas[1], 0, 0], np.int32), (len(windows), 1))
    return np.stack([letterbox_geometry(ch, cw, *canvas) for _, _, ch, cw in windows]).astype(np.int32)


def to_tile(box, window, geom, frame_hw, canvas):
    """A frame-normalised (xmin, ymin, xmax, ymax) box -> the canvas-normalised coordinates a tile's detection of it would have
    (float64 then rounded: the inverse of the merge's mapping up to rounding)."""
    y0, x0, ch, cw = (float(v) for v in window)
    sh, sw, top, left = (float(v) for v in geom)
    h, w = (float(v) for v in frame_hw)
    b = np.asarray(box, np.float64)
    out = np.empty(4)
    out[0::2] = ((b[0::2] * w - x0) / cw * sw + left) / canvas[1]
    out[1::2] = ((b[1::2] * h - y0) / ch * sh + top) / canvas[0]
    return out.astype(np.float32)


def merge_case(F, T, M, seed, letterbox=True, canvas=(64, 96), nclasses=3, poison=True):
    """Hand-made tile detections -> dict(packed [F*T,M,7] int32, nv [F*T] int32, windows, geoms, frame_hw, F, T, M, canvas).
    Per frame a set of well-formed objects (xmin < xmax, ymin < ymax, inside the frame); every tile reports the objects that
    overlap its window, clipped to it, with a per-tile jitter of the score -- so most objects appear in two or more tiles and
    the merge has duplicates to drop -- sorted by descending score and cut at M as the per-tile NMS leaves them.  Tile 1 of
    every frame is EMPTY (num_valid 0), the last tile of frame 0 reports num_valid = M + 7 (over-range; clamped) when its rows
    fill the tile, and the last tile of the last frame a negative count.  poison: rows behind num_valid hold 0x7F7F7F7F words
    instead of zeros: nothing may read them.  Frame shapes alternate; the windows are a hand-written grid + the whole frame
    last, so that the whole-axis and identity branches of the mapping are taken."""
    rng = np.random.default_rng(seed)
    shapes = [(97, 131), (64, 48), (200, 120)]
    packed = np.zeros((F * T, M, 7), np.int32)
    if poison:
        packed[...] = 0x7F7F7F7F
    nv = np.zeros(F * T, np.int32)
    windows = np.zeros((F * T, 4), np.int32)
    frame_hw = np.zeros((F, 2), np.int32)
    for f in range(F):
        h, w = shapes[f % len(shapes)]
        frame_hw[f] = h, w
        wins = _hand_grid(h, w, T)
        windows[f * T:(f + 1) * T] = wins
    geoms = window_geoms(windows, canvas, letterbox)
    for f in range(F):
        h, w = frame_hw[f]
        n_obj = 2 * M + 3 if (f + seed) % 2 == 0 else max(3, M // 3 + 2)     # a crowded frame (both caps bind), then a sparse one
        c = rng.uniform(0.05, 0.95, (n_obj, 2))
        s = rng.uniform(0.04, 0.3, (n_obj, 2))
        obj = np.clip(np.concatenate([c - s / 2, c + s / 2], 1), 0.0, 1.0)
        obj_score = rng.uniform(0.06, 0.99, n_obj)
        obj_cls = rng.integers(0, nclasses, n_obj)
        if n_obj > 4:       # two objects on top of each other, of one class and of two: the two NMS rules part here
            obj[1], obj_cls[1] = obj[0], obj_cls[0]
            obj[3], obj_cls[3] = obj[2], (obj_cls[2] + 1) % nclasses
        for t in range(T):
            gi = f * T + t
            if t == 1:
                continue
            y0, x0, ch, cw = windows[gi]
            lo = np.array([x0 / w, y0 / h, x0 / w, y0 / h])
            hi = np.array([(x0 + cw) / w, (y0 + ch) / h, (x0 + cw) / w, (y0 + ch) / h])
            rows = []
            for k in range(n_obj):
                b = np.clip(obj[k], lo, hi)
                if b[2] - b[0] <= 0 or b[3] - b[1] <= 0:
                    continue
                sc = np.float32(obj_score[k] * rng.uniform(0.9, 1.0)) if k % 5 else np.float32(obj_score[k])   # every fifth: EQUAL scores in all its tiles
                rows.append((sc, to_tile(b, windows[gi], geoms[gi], frame_hw[f], canvas), int(obj_cls[k])))
            rows.sort(key=lambda r: -r[0])
            rows = rows[:M]
            for r, (sc, b, c_) in enumerate(rows):
                packed[gi, r, :4] = b.view(np.int32)
                packed[gi, r, 4] = np.float32(sc).view(np.int32)
                packed[gi, r, 5] = c_
                packed[gi, r, 6] = 1000 + r        # the tile's own index word: not carried into the merged rows
            nv[gi] = len(rows)
        last = f * T + T - 1
        if f == 0 and T > 1 and nv[last] == M:
            nv[last] = M + 7
        if f == F - 1 and f > 0 and T > 2:
            nv[last] = -3
    return dict(packed=packed, nv=nv, windows=windows, geoms=geoms, frame_hw=frame_hw, F=F, T=T, M=M, canvas=canvas)


def _hand_grid(h, w, T):
    """T windows of an h x w frame: the whole frame LAST (and alone for T == 1); before it a near-square grid of overlapping
    windows, cycled when T - 1 exceeds it, with whole-width strips among them (x axis whole, y axis not)."""
    if T == 1:
        return np.array([[0, 0, h, w]], np.int32)
    base = []
    k = max(1, int(np.ceil(np.sqrt(T - 1))))
    lh, lw = -(-(h + (k - 1) * 8) // k), -(-(w + (k - 1) * 8) // k)
    lh, lw = min(lh, h), min(lw, w)
    for i in range(k):
        for j in range(k):
            y0 = 0 if k == 1 else i * (h - lh) // (k - 1)
            x0 = 0 if k == 1 else j * (w - lw) // (k - 1)
            base.append((y0, x0, lh, lw))
    base.insert(2, (h // 3, 0, h // 2, w))      # a whole-width strip
    wins = [base[i % len(base)] for i in range(T - 1)] + [(0, 0, h, w)]
    return np.array(wins, np.int32)


def empty_case(F, T, M, canvas=(64, 64)):
    """All-empty frames: every num_valid 0, the rows poisoned."""
    case = merge_case(F, T, M, 1, canvas=canvas)
    case["nv"][:] = 0
    return case


def identity_case(M=100, seed=3):
    """One frame whose every tile is the whole frame on an identity geometry (stretched onto a canvas): the mapping copies, so
    the same object in two tiles is an EXACT duplicate, equal scores included -- the lower index wins."""
    case = merge_case(1, 4, M, seed, letterbox=False, canvas=(64, 64))
    h, w = case["frame_hw"][0]
    case["windows"][:] = (0, 0, h, w)
    case["packed"][2], case["nv"][2] = case["packed"][0], case["nv"][0]      # tile 2 repeats tile 0 word for word
    return case


# ------------------------------------------------------------------------------------------------ brute force
def _iou(a, b):
    """TF's _bbox_overlap on two boxes in fp32, every operation rounded on its own (the order of iou_tf in csrc/nms.hip)."""
    f = np.float32
    with np.errstate(all="ignore"):
        ix0, ix1 = max(a[1], b[1]), min(a[3], b[3])
        iy0, iy1 = max(a[0], b[0]), min(a[2], b[2])
        ia = f(max(f(ix1 - ix0), f(0))) * f(max(f(iy1 - iy0), f(0)))
        aa = f(f(a[2] - a[0]) * f(a[3] - a[1]))
        ba = f(f(b[2] - b[0]) * f(b[3] - b[1]))
        return f(ia / f(f(f(aa + ba) - ia) + f(1e-8)))


def brute_force_nms(boxes, scores, classes, M, T, S, per_class):
    """The padded NMS as a plain double loop, for inputs whose box [0,0] is well formed (no canonicalisation) -> (sel, nv)."""
    B, N = scores.shape
    sel, nv = np.zeros((B, M), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        order = sorted((i for i in range(N) if scores[b, i] > np.float32(S)), key=lambda i: (-float(scores[b, i]), i))
        kept = []
        for i in order:
            if nv[b] >= M:
                break
            if any((not per_class or classes[b, k] == classes[b, i]) and _iou(boxes[b, k], boxes[b, i]) >= np.float32(T) for k in kept):
                continue
            kept.append(i)
            if (boxes[b, i] > 0).any():
                sel[b, nv[b]] = i
                nv[b] += 1
    return sel, nv


def rows_from(boxes, scores, classes, sel, nv, M):
    """y3_pack_detections on the host."""
    out = np.zeros((len(nv), M, 7), np.int32)
    for b, n in enumerate(nv):
        idx = sel[b, :n]
        out[b, :n, :4] = boxes[b, idx].view(np.int32)
        out[b, :n, 4] = scores[b, idx].view(np.int32)
        out[b, :n, 5] = classes[b, idx]
        out[b, :n, 6] = idx
    return out
