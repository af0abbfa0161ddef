"""Host mirror of reference core/yolo_nms.py -- same name and signature, HIP underneath."""
from ..ops import _nms
from ..runtime import class_scores as _class_scores


def yolo_nms(outputs, yolo_max_boxes, nms_iou_threshold, nms_score_threshold):
    """outputs = (bboxes [B,N,4], confidence [B,N,1], class_probs [B,N,nc]) CUDA tensors.
    Returns (bboxes [B,N,4] f32, class_indices [B,N] i64, scores [B,N] f32 (unfiltered),
    selected_indices_padded [B,max] i32, num_valid_detections [B] i32) -- reference: core/yolo_nms.py:16-34.
    Class-agnostic NMS with TF's `non_max_suppression_padded` semantics (IoU >= threshold suppresses,
    score > threshold passes, ties by lower index)."""
    return _yolo_nms(outputs, yolo_max_boxes, nms_iou_threshold, nms_score_threshold, per_class=False)


def yolo_nms_per_class(outputs, yolo_max_boxes, nms_iou_threshold, nms_score_threshold):
    """yolo_nms with the per-class rule (no reference counterpart): a box is suppressed only by a kept box of its own class
    (ops.nms_padded_per_class), yolo_max_boxes over all classes together.  Same arguments, same 5-tuple; nms_iou_threshold > 0."""
    return _yolo_nms(outputs, yolo_max_boxes, nms_iou_threshold, nms_score_threshold, per_class=True)


def yolo_nms_multi_label(outputs, yolo_max_boxes, nms_iou_threshold, nms_score_threshold, capacity=0, per_class=True):
    """Multi-label detections (multilabel.py; no reference counterpart): every pair (box, class) with confidence * class_prob >
    nms_score_threshold is a candidate of its own (ops.class_candidates; capacity slots per image, 0 = N), and the NMS -- per class by
    default, the rule the published protocol pairs with it; per_class=False: the class-agnostic rule -- decides between them.  Returns
    the reference-shaped 5-tuple OVER CANDIDATES: (cand_bboxes [B,K,4], cand_classes [B,K] i64, cand_scores [B,K],
    selected_indices_padded, num_valid_detections), so that gather_valid_detections_results works unchanged."""
    from ..ops import class_candidates
    from .yolo_decode_layer import _to_device
    bboxes, confidence, class_probs = (_to_device(t) for t in outputs)
    bboxes = bboxes.reshape(bboxes.shape[0], -1, 4).contiguous()
    K = int(capacity) or bboxes.shape[1]
    cand_bboxes, cand_classes, cand_scores, _, _ = class_candidates(bboxes, confidence.contiguous(), class_probs.contiguous(),
                                                                     nms_score_threshold, K)
    selected_indices_padded, num_valid_detections = _nms(cand_bboxes, cand_scores, yolo_max_boxes, nms_iou_threshold, nms_score_threshold,
                                                         classes=cand_classes if per_class else None)
    return (cand_bboxes, cand_classes, cand_scores, selected_indices_padded, num_valid_detections)


def _yolo_nms(outputs, yolo_max_boxes, nms_iou_threshold, nms_score_threshold, per_class):
    from .yolo_decode_layer import _to_device
    bboxes, confidence, class_probs = (_to_device(t) for t in outputs)
    class_indices, scores = _class_scores(confidence.contiguous(), class_probs.contiguous())
    bboxes = bboxes.reshape(bboxes.shape[0], -1, 4).contiguous()
    selected_indices_padded, num_valid_detections = _nms(bboxes, scores, yolo_max_boxes, nms_iou_threshold, nms_score_threshold,
                                                         classes=class_indices if per_class else None)
    return (bboxes, class_indices, scores, selected_indices_padded, num_valid_detections)
