"""Per-class NMS, restated on the host in NumPy: what y3_nms_padded_per_class (csrc/nms.hip, the PER_CLASS instantiation of
nms_kernel) is held to, bit for bit.  No reference counterpart; no GPU, no library call.

The rule is the five steps of the class-agnostic padded NMS (oracle/y3_oracle.c) with one predicate changed:

  1. boxes and scores with score <= S are masked out (they become all-zero boxes: never selected, IoU 0 with everything);
  2. the coordinate canonicalisation is decided by box [0,0] of the batch after masking, and applied batch-wide;
  3. descending sort by score, ties by lower original index, -0 == +0;
  4. greedy suppression in sorted order: a candidate is suppressed by an earlier kept candidate iff THEIR CLASS IDS ARE EQUAL
     and IoU >= T -- the fp32 IoU of TF's _bbox_overlap, IoU(kept, candidate), every operation rounded on its own;
  5. a survivor is selected iff any of its coordinates is > 0; the first M selected boxes OVER ALL CLASSES TOGETHER are returned
     as original indices in sorted order, the rest of the row is zero, num_valid = min(count, M).

T <= 0 selects a quirk of TF's tiles in the agnostic rule; it has no meaning here and is refused."""
import numpy as np

_EPS = np.float32(1e-8)


def iou_tf(a, b):
    """IoU(a, b) of boxes (y1, x1, y2, x2) in fp32, in the association order of iou_tf in csrc/nms.hip.  a: [..., 4] float32 (one
    box or many), b: [4] float32; NumPy rounds every elementwise fp32 operation on its own, as the kernel does."""
    i_xmin, i_xmax = np.fmax(a[..., 1], b[1]), np.fmin(a[..., 3], b[3])
    i_ymin, i_ymax = np.fmax(a[..., 0], b[0]), np.fmin(a[..., 2], b[2])
    zero = np.float32(0.0)
    i_area = np.fmax(i_xmax - i_xmin, zero) * np.fmax(i_ymax - i_ymin, zero)
    a_area = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    b_area = (b[2] - b[0]) * (b[3] - b[1])
    u_area = a_area + b_area - i_area + _EPS
    return i_area / u_area


def nms_padded_per_class_ref(boxes, scores, classes, M, T, S):
    """boxes [B,N,4] float32, scores [B,N] float32, classes [B,N] integers in [0, 2^31), max_output_size M, IoU threshold T > 0,
    score threshold S -> (selected indices [B,M] int32, zero padded; num_valid [B] int32)."""
    boxes = np.ascontiguousarray(boxes, np.float32)
    scores = np.ascontiguousarray(scores, np.float32)
    classes = np.asarray(classes)
    B, N = scores.shape
    if boxes.shape != (B, N, 4) or classes.shape != (B, N):
        raise ValueError("nms_padded_per_class_ref: boxes [B,N,4], scores [B,N], classes [B,N]")
    M, T, S = int(M), np.float32(T), np.float32(S)
    if not T > 0:
        raise ValueError("nms_padded_per_class_ref: iou_threshold must be > 0")
    cls32 = classes.astype(np.int64).astype(np.int32)      # the kernel compares the ids as int32
    m00 = np.float32(1.0 if scores[0, 0] > S else 0.0)
    b00 = boxes[0, 0] * m00
    swap_y, swap_x = not b00[0] <= b00[2], not b00[1] <= b00[3]
    sel, nv = np.zeros((B, M), np.int32), np.zeros(B, np.int32)
    with np.errstate(all="ignore"):
        for b in range(B):
            cand = np.flatnonzero(scores[b] > S)                        # step 1; ascending index
            cand = cand[np.argsort(-(scores[b, cand] + np.float32(0.0)), kind="stable")]     # step 3
            bx = boxes[b, cand]
            if swap_y:
                bx = bx[:, [2, 1, 0, 3]]
            if swap_x:
                bx = bx[:, [0, 3, 2, 1]]
            kept_box, kept_cls, n_kept, n_sel = np.zeros((len(cand), 4), np.float32), np.zeros(len(cand), np.int32), 0, 0
            for j, idx in enumerate(cand):
                if n_sel >= M:
                    break
                same = kept_cls[:n_kept] == cls32[b, idx]
                if same.any() and (iou_tf(kept_box[:n_kept][same], bx[j]) >= T).any():      # step 4
                    continue
                kept_box[n_kept], kept_cls[n_kept] = bx[j], cls32[b, idx]
                n_kept += 1
                if (bx[j] > 0).any():                                   # step 5
                    sel[b, n_sel] = idx
                    n_sel += 1
            nv[b] = n_sel
    return sel, nv
