"""`YoloNmsLayer`: the object form of `yolo_nms` -- three NMS limits fixed at construction, applied on call.

Interface of reference core/yolo_nms_layer.py:16-29 (a Keras `Layer` subclass there; it owns no weights, so a plain
callable carries everything the callers at inference.py:114-115 and evaluate_yolov3.py:111-112 use).
per_class=True (a keyword of this project's own, off by default) applies `yolo_nms_per_class` instead; multi_label=True (another,
with multi_label_capacity beside it) applies `yolo_nms_multi_label` under the rule per_class selects.
"""
from .yolo_nms import yolo_nms, yolo_nms_multi_label, yolo_nms_per_class


class YoloNmsLayer:
    _LIMITS = ("yolo_max_boxes", "nms_iou_threshold", "nms_score_threshold")

    def __init__(self, yolo_max_boxes, nms_iou_threshold, nms_score_threshold, **kwargs):
        for key, value in zip(self._LIMITS, (yolo_max_boxes, nms_iou_threshold, nms_score_threshold)):
            setattr(self, key, value)
        self.name = kwargs.pop("name", "yolo_nms_layer")   # the only Layer keyword the callers pass
        self.per_class = bool(kwargs.pop("per_class", False))
        self.multi_label = bool(kwargs.pop("multi_label", False))
        self.multi_label_capacity = int(kwargs.pop("multi_label_capacity", 0))

    def call(self, decoded_outputs, **kwargs):
        """(bboxes, confidences, class_probs) -> the NMS 5-tuple"""
        if self.multi_label:
            return yolo_nms_multi_label(decoded_outputs, *(getattr(self, key) for key in self._LIMITS), self.multi_label_capacity,
                                        self.per_class)
        nms = yolo_nms_per_class if self.per_class else yolo_nms
        return nms(decoded_outputs, *(getattr(self, key) for key in self._LIMITS))

    __call__ = call
