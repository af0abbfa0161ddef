"""Multi-label detections, restated on the host in NumPy: what y3_yolo_decode_candidates_hw (csrc/candidates.hip) and
y3_net_detect in multi-label mode are held to, bit for bit.  No reference counterpart; no GPU, no library call.

The rule (include/y3.h; DESIGN.md "Multi-label detections"): every pair (box n, class c) with conf[n] * prob[n,c] > S is a
candidate of its own -- one fp32 multiply, a strict compare (a NaN score is no candidate) -- numbered per image in the order
(n ascending, c ascending); the first min(total, K) candidates are stored, the rows behind them are zero, total is uncapped.  The
existing padded NMS (per class, or class-agnostic) then runs over the [B,K] candidates, the existing pack over its selection, and
the index word of every valid packed row is rewritten from the candidate k to its source box n.

The restatement takes conf / probs, not logits: expf differs between the device and NumPy, so the claim is "equal to the
composed device route y3_yolo_decode_hw -> candidates_ref", as csrc/decode_box.h promises for the fused heads."""
import numpy as np

from .nms_per_class import nms_padded_per_class_ref
from .tiles import nms_padded_agnostic_ref


def candidates_ref(bboxes, conf, probs, S, K):
    """bboxes [B,N,4], conf [B,N,1] or [B,N], probs [B,N,nc] float32 (yolo_decode's arrays), score threshold S, capacity K >= 1
    -> (cand_boxes [B,K,4] f32, cand_cls [B,K] i64, cand_scores [B,K] f32, cand_src [B,K] i32, totals [B] i32)."""
    bboxes = np.ascontiguousarray(bboxes, np.float32)
    probs = np.ascontiguousarray(probs, np.float32)
    B, N, nc = probs.shape
    conf = np.ascontiguousarray(conf, np.float32).reshape(B, N, 1)
    K = int(K)
    if bboxes.shape != (B, N, 4) or K < 1:
        raise ValueError("candidates_ref: bboxes [B,N,4], conf [B,N(,1)], probs [B,N,nc], K >= 1")
    with np.errstate(all="ignore"):
        score = conf * probs                                   # [B,N,nc]: one fp32 multiply per pair
        keep = score > np.float32(S)                           # strict; False for NaN
    boxes = np.zeros((B, K, 4), np.float32)
    cls, scores = np.zeros((B, K), np.int64), np.zeros((B, K), np.float32)
    src, totals = np.zeros((B, K), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        n, c = np.nonzero(keep[b])                             # row-major: n ascending, then c ascending
        totals[b] = len(n)
        n, c = n[:K], c[:K]
        boxes[b, :len(n)], cls[b, :len(n)], scores[b, :len(n)], src[b, :len(n)] = bboxes[b, n], c, score[b, n, c], n
    return boxes, cls, scores, src, totals


def pack_candidates_ref(cand, sel, nv):
    """y3_pack_detections over the candidates, then y3_candidate_sources: rows {box, score, class, source box n} as int32 words
    [B,M,7], zero behind num_valid."""
    boxes, cls, scores, src, _ = cand
    sel = np.asarray(sel)
    out = np.zeros((len(sel), sel.shape[1], 7), np.int32)
    for b, n in enumerate(np.asarray(nv)):
        idx = sel[b, :n]
        out[b, :n, :4] = boxes[b, idx].view(np.int32)
        out[b, :n, 4] = scores[b, idx].view(np.int32)
        out[b, :n, 5] = cls[b, idx].astype(np.int32)
        out[b, :n, 6] = src[b, idx]
    return out


def detect_multi_label_ref(bboxes, conf, probs, S, K, max_boxes, iou_threshold, per_class=True, agnostic_nms=None):
    """The multi-label detections of decoded heads -> (packed int32 [B,M,7], num_valid int32 [B], totals int32 [B]): candidates_ref,
    the padded NMS over the [B,K] candidates at (max_boxes, iou_threshold, S) -- nms_padded_per_class_ref, or with per_class=False
    the class-agnostic rule agnostic_nms(boxes, scores, M, T, S) -> (sel, nv), by default tiles.nms_padded_agnostic_ref (T > 0) --
    then pack_candidates_ref.  Every quirk of the NMS is inherited: the canonicalisation is decided by candidate 0 of image 0."""
    cand = candidates_ref(bboxes, conf, probs, S, K)
    if per_class:
        sel, nv = nms_padded_per_class_ref(cand[0], cand[2], cand[1], max_boxes, iou_threshold, S)
    else:
        sel, nv = (agnostic_nms or nms_padded_agnostic_ref)(cand[0], cand[2], int(max_boxes), iou_threshold, S)
    return pack_candidates_ref(cand, sel, nv), np.asarray(nv, np.int32), cand[4]


def rows_above(packed, num_valid, threshold):
    """The rows with score > threshold of packed results, kept in order and zero padded: the detections at that higher score
    threshold (the one-pass property; holds for images whose total did not exceed the capacity at the lower threshold)."""
    from .tiles import merged_rows_above
    return merged_rows_above(packed, num_valid, threshold)


def label_counts(totals_per_box):
    """int [B,N] candidates per box -> (boxes with at least one label, boxes with two or more)."""
    t = np.asarray(totals_per_box)
    return int((t >= 1).sum()), int((t >= 2).sum())
