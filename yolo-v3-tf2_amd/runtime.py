"""Thin host wrappers around the C ABI: torch tensors in, torch tensors out.

PyTorch is used for device memory and streams only; every arithmetic step is a call into liby3hip.so on the current torch
stream.  This module is the import point and holds no code of its own: net.py has class Net, stream.py the pipelines behind
Net.detect_stream / Net.evaluate_stream, ops.py the stand-alone op wrappers, input_stage.py the host-to-device input path.
"""
from ._lib import AuxDesc, ConvDesc, TensorDesc, Y3Error, check  # noqa: F401
from .graph import AuxOp, ConvOp, Program  # noqa: F401
from .input_stage import (IMAGE_DESC_DTYPE, InputStage, StagedBatch, canvas_hw, letterbox_geometries, pack_images,  # noqa: F401
                          packed_nbytes, preprocess_batch, preprocess_image, rect_anchors, rect_canvas, unletterbox_detections)
from .net import Net, tuning_table_path  # noqa: F401
from .ops import (ap_iou_thresholds, assign_targets, class_scores, evaluate_detections, match_detections, nms_padded,  # noqa: F401
                  pack_detections, pack_ground_truth, split2_planes, split3_planes, unpack_detections, yolo_decode,
                  yolo_decode_scores, yolo_loss)
from .weights import BN_EPS  # noqa: F401
