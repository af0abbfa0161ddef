"""Evaluation consumer of the detect 5-tuple (SURVEY.md 8f "n4") -- host side, NumPy.

Counterpart of reference evaluate_detections.py:16-165 (`EvaluateDetections`): per-class pred / gt / TP / FP / FN
counters from IoU matching of one image's predictions against its ground truth.  Semantics kept, including the
vectorised quirk of the reference: every prediction is matched against the *initial* (empty) assignment vector
(reference: evaluate_detections.py:107-112), so two predictions that pick the same ground-truth box both count as
true positives; the assignment vector only feeds the false-negative count.

`sweep_counters` restates, in NumPy, what the device kernel behind y3_evaluate_detections computes (csrc/evaluate.hip): the
counters of every NMS score threshold of a sweep from ONE set of packed detections, taken at the lowest threshold.

`match_detections` restates y3_match_detections (csrc/ap_match.hip), the per-image greedy matching behind COCO-style average
precision, and `average_precision` integrates a data set's records on the host.  Neither has a reference counterpart.
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


# ------------------------------------------------------------------------------------------------
# COCO-style average precision.  No reference counterpart: the reference stops at the counters above, whose quirk (two
# predictions on one ground-truth box are both TP) makes them incomparable with a published mAP.  The matching rule is this
# project's statement of the COCO matching -- greedy in score order, a ground-truth box matched at most once per IoU threshold;
# no crowd flags, no area ranges, max_boxes as the per-image cap -- and is not checked against pycocotools.
AP_IOU_THRESHOLDS = np.linspace(0.5, 0.95, 10).astype(np.float32)      # mAP@[.5:.95]
INVALID_RECORD = np.uint32(0xFFFFFFFF)                                 # word 1 of a record row that holds no detection


def match_detections(packed, num_valid, gt_boxes, gt_classes, gt_count, nclasses, iou_thresholds, one_class=False,
                     return_matches=False):
    """Host restatement of y3_match_detections (include/y3.h; csrc/ap_match.hip), no GPU, bit for bit: packed [B,M,7] int32 words
    and num_valid [B], padded ground truth as for sweep_counters, iou_thresholds [K] fp32 -> (records uint32 [B,M,2], gt_totals
    int64 [nclasses + 2]).  Per image and per threshold t_k the rows are walked in ROW order (Net.detect writes them in descending
    score; nothing is sorted here): row r takes the ground-truth row of its class, not yet taken at this threshold, with the
    largest fp32 IoU >= t_k (a NaN never qualifies), the HIGHER row on a tie; bit k of the row's mask is set.
    records[b,r] = (score bits, class | mask << 16) for r < num_valid of a counted image, (0, 0xFFFFFFFF) for every other row.
    gt_totals[c] = ground-truth rows of class c, gt_totals[nclasses] = error images (a ground-truth class or the class of a
    row r < num_valid outside [0,nclasses), after one_class; nothing else of them is counted), gt_totals[nclasses + 1] = images
    counted.  return_matches: a third result, int64 [B,M,K], the ground-truth row each row took per threshold (-1: none), which
    the device does not report."""
    packed = np.ascontiguousarray(packed, np.int32)
    if packed.ndim != 3 or packed.shape[2] != 7:
        raise ValueError("packed must be [B,M,7] int32 words")
    B, M = packed.shape[:2]
    gt_boxes = np.ascontiguousarray(gt_boxes, np.float32).reshape(B, -1, 4)
    G = gt_boxes.shape[1]
    gt_classes = np.asarray(gt_classes).astype(np.int64).reshape(B, G)
    num_valid = np.clip(np.asarray(num_valid).astype(np.int64).reshape(B), 0, M)
    gt_count = np.clip(np.asarray(gt_count).astype(np.int64).reshape(B), 0, G)
    thresholds = np.asarray(iou_thresholds, np.float32).reshape(-1)
    nc = int(nclasses)
    records = np.zeros((B, M, 2), np.uint32)
    records[..., 1] = INVALID_RECORD
    totals = np.zeros(nc + 2, np.int64)
    matches = np.full((B, M, len(thresholds)), -1, np.int64)
    boxes = packed[..., :4].copy().view(np.float32)
    for b in range(B):
        n, g = int(num_valid[b]), int(gt_count[b])
        pb, pc = boxes[b, :n], packed[b, :n, 5].astype(np.int64)
        gb, gc = gt_boxes[b, :g], gt_classes[b, :g]
        if one_class:
            pc, gc = np.zeros_like(pc), np.zeros_like(gc)
        if ((gc < 0) | (gc >= nc)).any() or ((pc < 0) | (pc >= nc)).any():
            totals[nc] += 1
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            ow = np.maximum(np.minimum(pb[:, None, 2], gb[None, :, 2]) - np.maximum(pb[:, None, 0], gb[None, :, 0]), np.float32(0))
            oh = np.maximum(np.minimum(pb[:, None, 3], gb[None, :, 3]) - np.maximum(pb[:, None, 1], gb[None, :, 1]), np.float32(0))
            inter = ow * oh
            a1 = ((pb[:, 2] - pb[:, 0]) * (pb[:, 3] - pb[:, 1]))[:, None]
            a2 = ((gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1]))[None, :]
            iou = inter / (a1 + a2 - inter)                                      # [n,g] fp32
            masks = np.zeros(n, np.uint32)
            for k, t in enumerate(thresholds):
                taken = np.zeros(g, bool)
                for r in range(n):
                    free = np.flatnonzero((gc == pc[r]) & ~taken & (iou[r] >= t))    # NaN >= t is False
                    if len(free):
                        best = free[iou[r, free] == iou[r, free].max()][-1]      # the largest IoU, the higher row on a tie
                        taken[best] = True
                        masks[r] |= np.uint32(1 << k)
                        matches[b, r, k] = best
        records[b, :n, 0] = packed[b, :n, 4].view(np.uint32)
        records[b, :n, 1] = pc.astype(np.uint32) | (masks << np.uint32(16))
        totals[:nc] += np.bincount(gc, minlength=nc)
        totals[nc + 1] += 1
    return (records, totals, matches) if return_matches else (records, totals)


def average_precision(records, gt_totals, nclasses, n_iou):
    """The records of a whole data set ([images, M, 2] uint32, in stream order) and its gt_totals -> COCO-style AP, float64 on
    the host: {"ap": [n_iou, nclasses], "map": [n_iou], "mAP": float, "images": int, "errors": int}.
    Per class c with gt_totals[c] > 0 and per threshold k: the valid records of class c, sorted by score descending (stable
    in record order); cumulative tp (bit k of the mask) and fp; recall = ctp / gt_totals[c], precision = ctp / (ctp + cfp),
    made non-increasing from the right; sampled at the 101 recalls 0, 0.01, ..., 1 (searchsorted, side="left"; 0 beyond the
    last recall); AP = the mean of the 101 samples.  ap is NaN for a class without ground truth, map[k] the mean over the
    classes with ground truth (NaN when there is none), mAP the mean of map."""
    nc, K = int(nclasses), int(n_iou)
    records = np.ascontiguousarray(records).view(np.uint32).reshape(-1, 2)
    totals = np.asarray(gt_totals, np.int64).reshape(-1)
    if totals.size != nc + 2:
        raise ValueError(f"gt_totals of {nc} classes has {nc + 2} entries, got {totals.size}")
    records = records[records[:, 1] != INVALID_RECORD]
    scores = records[:, 0].copy().view(np.float32).astype(np.float64)
    classes, masks = records[:, 1] & np.uint32(0xFFFF), records[:, 1] >> np.uint32(16)
    recalls = np.linspace(0.0, 1.0, 101)
    ap = np.full((K, nc), np.nan)
    for c in np.flatnonzero(totals[:nc] > 0):
        rows = np.flatnonzero(classes == c)
        rows = rows[np.argsort(-scores[rows], kind="stable")]
        for k in range(K):
            tp = ((masks[rows] >> np.uint32(k)) & np.uint32(1)).astype(np.float64)
            ctp, cfp = np.cumsum(tp), np.cumsum(1.0 - tp)
            recall = ctp / float(totals[c])
            precision = np.maximum.accumulate((ctp / (ctp + cfp))[::-1])[::-1]
            at = np.searchsorted(recall, recalls, side="left")
            sampled = np.zeros(101)
            sampled[at < len(rows)] = precision[at[at < len(rows)]]
            ap[k, c] = sampled.mean()
    have = totals[:nc] > 0
    per_threshold = ap[:, have].mean(axis=1) if have.any() else np.full(K, np.nan)
    return {"ap": ap, "map": per_threshold, "mAP": float(per_threshold.mean()), "images": int(totals[nc + 1]), "errors": int(totals[nc])}
