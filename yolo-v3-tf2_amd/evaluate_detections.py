"""Evaluation consumer of the detect 5-tuple (SURVEY.md 8f "n4") -- host side, NumPy.

Counterpart of reference evaluate_detections.py:16-165 (`EvaluateDetections`): per-class pred / gt / TP / FP / FN
counters from IoU matching of one image's predictions against its ground truth.  Semantics kept, including the
vectorised quirk of the reference: every prediction is matched against the *initial* (empty) assignment vector
(reference: evaluate_detections.py:107-112), so two predictions that pick the same ground-truth box both count as
true positives; the assignment vector only feeds the false-negative count.

`sweep_counters` restates, in NumPy, what the device kernel behind y3_evaluate_detections computes (csrc/evaluate.hip): the
counters of every NMS score threshold of a sweep from ONE set of packed detections, taken at the lowest threshold.
"""
from __future__ import annotations

import numpy as np


class EvaluateDetections:
    def __init__(self, nclasses, iou_thresh):
        self.nclasses = nclasses
        self.iou_thresh = iou_thresh
        z = lambda: np.zeros(nclasses, np.int64)
        self.counters = {"preds": z(), "gts": z(), "tp": z(), "fp": z(), "fn": z(), "errors": 0, "examples": 0}

    @staticmethod
    def iou_alg(box_1, box_2):
        """box_1 [4], box_2 [G,4] (xmin,ymin,xmax,ymax) -> [G]; no epsilon in the union (evaluate_detections.py:39-49)"""
        box_1 = np.asarray(box_1, np.float32)[None]
        box_2 = np.asarray(box_2, np.float32)
        ow = np.maximum(np.minimum(box_1[..., 2], box_2[..., 2]) - np.maximum(box_1[..., 0], box_2[..., 0]), 0)
        oh = np.maximum(np.minimum(box_1[..., 3], box_2[..., 3]) - np.maximum(box_1[..., 1], box_2[..., 1]), 0)
        inter = ow * oh
        a1 = (box_1[..., 2] - box_1[..., 0]) * (box_1[..., 3] - box_1[..., 1])
        a2 = (box_2[..., 2] - box_2[..., 0]) * (box_2[..., 3] - box_2[..., 1])
        return inter / (a1 + a2 - inter)

    def evaluate(self, pred_bboxes, pred_classes, gt_bboxes, gt_classes):
        pred_bboxes = np.asarray(pred_bboxes, np.float32).reshape(-1, 4)
        pred_classes = np.asarray(pred_classes).astype(np.int64).reshape(-1)
        gt_bboxes = np.asarray(gt_bboxes, np.float32).reshape(-1, 4)
        gt_classes = np.asarray(gt_classes).astype(np.int64).reshape(-1)
        c = self.counters
        if (gt_classes < 0).any() or (gt_classes >= self.nclasses).any():
            c["errors"] += 1            # reference: skips samples with a bad class id (evaluate_detections.py:66-70)
            return c
        assigned = np.zeros(len(gt_classes), bool)
        if len(pred_classes) and len(gt_classes):
            iou = np.stack([self.iou_alg(p, gt_bboxes) for p in pred_bboxes])      # [P,G]
            best = iou.argmax(axis=1)                                              # first maximum
            max_iou = iou[np.arange(len(best)), best]
            decisions = (max_iou > self.iou_thresh) & (gt_classes[best] == pred_classes) & ~assigned[best]
            np.logical_or.at(assigned, best, decisions)
        else:
            decisions = np.zeros(len(pred_classes), bool)
        np.add.at(c["tp"], pred_classes, decisions.astype(np.int64))
        np.add.at(c["fp"], pred_classes, (~decisions).astype(np.int64))
        np.add.at(c["fn"], gt_classes, (~assigned).astype(np.int64))
        np.add.at(c["gts"], gt_classes, 1)
        np.add.at(c["preds"], pred_classes, 1)
        c["examples"] += 1
        return c

    @staticmethod
    def gather_nms_output(bboxes_padded, class_indices_padded, scores_padded, selected_indices_padded,
                          num_valid_detections):
        """reference: evaluate_detections.py:168-176"""
        sel = np.asarray(selected_indices_padded)[:int(num_valid_detections)]
        return np.asarray(bboxes_padded)[sel], np.asarray(class_indices_padded)[sel], np.asarray(scores_padded)[sel]

    def recall_precision(self):
        tp, fp, fn = (self.counters[k].sum() for k in ("tp", "fp", "fn"))
        return tp / max(tp + fn, 1), tp / max(tp + fp, 1)


COUNTER_KEYS = ("preds", "gts", "tp", "fp", "fn")    # the per-class blocks of a counters row, in order; then errors, examples


def counters_from_row(row, nclasses):
    """One row [5*nclasses + 2] of sweep_counters / y3_evaluate_detections -> the dict EvaluateDetections.counters has."""
    row = np.asarray(row, np.int64).reshape(-1)
    if row.size != 5 * nclasses + 2:
        raise ValueError(f"a counters row of {nclasses} classes has {5 * nclasses + 2} entries, got {row.size}")
    c = {k: row[i * nclasses:(i + 1) * nclasses].copy() for i, k in enumerate(COUNTER_KEYS)}
    c["errors"], c["examples"] = int(row[5 * nclasses]), int(row[5 * nclasses + 1])
    return c


def sweep_counters(packed, num_valid, gt_boxes, gt_classes, gt_count, nclasses, iou_threshold, score_thresholds,
                   one_class=False):
    """Host restatement of y3_evaluate_detections (include/y3.h), no GPU: packed [B,M,7] int32 words and num_valid [B] as
    Net.detect leaves them at the LOWEST score threshold of the sweep, padded ground truth (gt_boxes [B,G,4] f32, gt_classes
    [B,G] i32, gt_count [B]) -> int64 [T, 5*nclasses + 2]: per threshold preds, gts, tp, fp, fn (each [nclasses]), errors,
    examples.  The greedy padded NMS never lets a box be affected by boxes scored below it, so the detections at threshold t
    are the rows r < num_valid with score[r] > t (strict, fp32), and on those rows the counters are EvaluateDetections.evaluate
    exactly.  one_class: every class id is taken as 0.  A prediction class outside [0,nclasses) among the rows of a threshold
    (EvaluateDetections would raise) makes the image an error image at that threshold, like a bad ground-truth class does."""
    packed = np.ascontiguousarray(packed, np.int32)
    if packed.ndim != 3 or packed.shape[2] != 7:
        raise ValueError("packed must be [B,M,7] int32 words")
    B, M = packed.shape[:2]
    gt_boxes = np.ascontiguousarray(gt_boxes, np.float32).reshape(B, -1, 4)
    G = gt_boxes.shape[1]
    gt_classes = np.asarray(gt_classes).astype(np.int64).reshape(B, G)
    num_valid = np.clip(np.asarray(num_valid).astype(np.int64).reshape(B), 0, M)
    gt_count = np.clip(np.asarray(gt_count).astype(np.int64).reshape(B), 0, G)
    thresholds = np.asarray(score_thresholds, np.float32).reshape(-1)
    iou_thresh = np.float32(iou_threshold)
    nc = int(nclasses)
    out = np.zeros((len(thresholds), 5 * nc + 2), np.int64)
    boxes = packed[..., :4].copy().view(np.float32)
    scores = packed[..., 4].copy().view(np.float32)
    for b in range(B):
        n, g = int(num_valid[b]), int(gt_count[b])
        pb, pc, ps = boxes[b, :n], packed[b, :n, 5].astype(np.int64), scores[b, :n]
        gb, gc = gt_boxes[b, :g], gt_classes[b, :g]
        if one_class:
            pc, gc = np.zeros_like(pc), np.zeros_like(gc)
        if ((gc < 0) | (gc >= nc)).any():
            out[:, 5 * nc] += 1
            continue
        best = np.zeros(n, np.int64)
        decisions = np.zeros(n, bool)
        if n and g:
            with np.errstate(invalid="ignore", divide="ignore"):
                ow = np.maximum(np.minimum(pb[:, None, 2], gb[None, :, 2]) - np.maximum(pb[:, None, 0], gb[None, :, 0]), np.float32(0))
                oh = np.maximum(np.minimum(pb[:, None, 3], gb[None, :, 3]) - np.maximum(pb[:, None, 1], gb[None, :, 1]), np.float32(0))
                inter = ow * oh
                a1 = ((pb[:, 2] - pb[:, 0]) * (pb[:, 3] - pb[:, 1]))[:, None]
                a2 = ((gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1]))[None, :]
                iou = inter / (a1 + a2 - inter)                                  # [n,g] fp32
                best = iou.argmax(axis=1)                                        # first maximum; a NaN counts as the maximum
                decisions = (iou[np.arange(n), best] > iou_thresh) & (gc[best] == pc)
        for t, thr in enumerate(thresholds):
            active = ps > thr
            c = pc[active]
            if ((c < 0) | (c >= nc)).any():
                out[t, 5 * nc] += 1
                continue
            d = decisions[active]
            assigned = np.zeros(g, bool)
            assigned[best[active][d]] = True
            row = out[t]
            row[0 * nc:1 * nc] += np.bincount(c, minlength=nc)
            row[1 * nc:2 * nc] += np.bincount(gc, minlength=nc)
            row[2 * nc:3 * nc] += np.bincount(c[d], minlength=nc)
            row[3 * nc:4 * nc] += np.bincount(c[~d], minlength=nc)
            row[4 * nc:5 * nc] += np.bincount(gc[~assigned], minlength=nc)
            row[5 * nc + 1] += 1
    return out
