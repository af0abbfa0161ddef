"""Counterpart of the reference's evaluation driver (reference: evaluate_yolov3.py:31-237; SURVEY.md 8f "n4").

TFRecord dataset -> batches through the GPU detect path -> per-image gather -> `EvaluateDetections` counters ->
recall / precision per NMS score threshold.  Same function names and argument meaning as the reference; NumPy arrays
where it has tf tensors, Python lists where it has ragged tensors.  The reference script as shipped cannot run (it
imports `decoded_output` but calls `yolo_decode`, evaluate_yolov3.py:23,109); the intended behaviour is built here.

`evaluate(..., on_device=True)` gives the same results from ONE pass over the data set: one model, one y3_net_detect per
batch at the lowest threshold, and the counters of every threshold counted on the GPU (runtime.Net.evaluate_stream).
With `loss=True` the same pass also gives what the reference picks a checkpoint by: val_loss and its per-grid / per-source
breakdown (reference: train.py:39-54,86-91; core/loss_func.py), computed on the GPU from the raw head grids.
"""
from __future__ import annotations

import collections

import numpy as np
import yaml

from .core.load_tfrecords import parse_tfrecords
from .core.parse_model import Input, ParseModel
from .core.utils import get_anchors, resize_image
from .core.loss_func import summarize_loss
from .evaluate_detections import EvaluateDetections, counters_from_row
from .inference import DetectModel


def arrange_predict_output(batch_bboxes_padded, batch_class_indices_padded, batch_scores_padded,
                           batch_selected_indices_padded, batch_num_valid_detections, batch_gt_y):
    """-> (bboxes_batch, classes_batch, gt_bboxes_batch, gt_classes_batch); the first two are per-image lists
    (ragged), the last two stacked arrays (reference: evaluate_yolov3.py:31-82)."""
    bboxes_batch, classes_batch, gt_bboxes_batch, gt_classes_batch = [], [], [], []
    for bb, cc, ss, sel, nv, gt_y in zip(batch_bboxes_padded, batch_class_indices_padded, batch_scores_padded,
                                         batch_selected_indices_padded, batch_num_valid_detections, batch_gt_y):
        b, c, _ = EvaluateDetections.gather_nms_output(bb, cc, ss, sel, nv)
        bboxes_batch.append(b)
        classes_batch.append(c)
        gt_y = np.asarray(gt_y, np.float32)
        gt_bboxes_batch.append(gt_y[..., 0:4])                     # tf.split(gt_y, [4, 1, 1], axis=-1)
        gt_classes_batch.append(gt_y[..., 5].astype(np.int32))
    return bboxes_batch, classes_batch, np.stack(gt_bboxes_batch), np.stack(gt_classes_batch)


def prepare_dataset(tfrecords_dir, batch_size, image_size, yolo_max_boxes, classes_name_file):
    """reference: evaluate_yolov3.py:85-94.  Rows whose objectness column is 1 are kept (drops the zero padding), so
    -- as in the reference -- a batch only stacks when its images hold equally many boxes."""
    dataset = parse_tfrecords(tfrecords_dir, image_size=image_size, max_bboxes=yolo_max_boxes,
                              class_file=classes_name_file)
    dataset = dataset.map(lambda x, y: (x, y[y[..., 4] == 1]))
    dataset = dataset.batch(batch_size)
    dataset = dataset.map(lambda img, y: (resize_image(img, image_size, image_size), y))
    return dataset


def create_model(model_config_file, nclasses, anchors_table, nms_score_threshold, nms_iou_threshold, yolo_max_boxes,
                 input_weights_path, weights=None):
    """reference: evaluate_yolov3.py:97-116 -> callable with .predict(batch) returning the NMS 5-tuple"""
    with open(model_config_file, "r") as _stream:
        model_config = yaml.safe_load(_stream)
    inputs = Input(shape=(None, None, 3))
    model = ParseModel().build_model(inputs, nclasses=nclasses, **model_config)
    if weights is not None:
        model.set_weights_dict(weights)
    else:
        model.load_weights(input_weights_path).expect_partial()
    print("weights loaded")
    return DetectModel(model, anchors_table, nclasses, yolo_max_boxes, nms_iou_threshold, nms_score_threshold)


def calc_recal_precision(counters):
    """reference: evaluate_yolov3.py:119-125 -- per-class vectors, 1e-20 in the denominators"""
    tp, fp, fn = (np.asarray(counters[k], np.float32) for k in ("tp", "fp", "fn"))
    recall = tp / (tp + fn + np.float32(1e-20))
    precision = tp / (tp + fp + np.float32(1e-20))
    print(f"recall: {recall}, precision: {precision}")
    return recall, precision


def report_loss(loss):
    """Print the loss of an evaluation pass in the wording of the reference's eager loop (train.py:86-91) and return
    (val_loss, perGrid [3], perSource [4]).  The reference's totLoss also holds the regulariser; this number does not."""
    val_loss, per_grid, per_source = summarize_loss(loss["sum"], loss["images"])
    print(f'val_loss:{val_loss}, '
          f'perGrid{list(per_grid)}, '
          f'perSource[xy,wh,obj,class]:{per_source}, '
          f'images:{loss["images"]}, errors:{loss["errors"]}')
    return val_loss, per_grid, per_source


def report_ap(ap, iou_thresholds):
    """Prints AP50 and AP75 (when those IoU thresholds are among iou_thresholds) and mAP of Net.evaluate_stream's AP dict."""
    parts = [f'AP{int(round(100 * float(t)))}:{ap["map"][k]:.4f}' for k, t in enumerate(iou_thresholds)
             if any(np.float32(t) == np.float32(v) for v in (0.5, 0.75))]
    lo, hi = float(min(iou_thresholds)), float(max(iou_thresholds))
    print(", ".join(parts + [f'mAP@[{lo:.2f}:{hi:.2f}]:{ap["mAP"]:.4f}', f'images:{ap["images"]}', f'errors:{ap["errors"]}']))


def _evaluate_on_device(detect_config, thresholds, evaluate_iou_threshold, max_batches, weights, one_class, anchors_table, nclasses,
                        loss=False, ap=None, nms_per_class=False, tiles=None, multi_label=False, multi_label_capacity=0):
    """One model and one pass: the un-stacked data set is batched here (images with unlike numbers of boxes may share a batch)
    by a generator that Net.evaluate_stream draws from, so records are decoded while earlier batches run and the data set is
    never held in memory; only the counters come back."""
    if not isinstance(detect_config["image_size"], int):
        raise ValueError("evaluate_yolov3: image_size must be an int; the records are resized to a square on the host "
                         "(an [H, W] canvas is served by Net.evaluate_stream and by inference.py)")
    S, batch_size = int(detect_config["image_size"]), int(detect_config["batch_size"])
    model = create_model(detect_config["model_config_file"], nclasses, anchors_table, min(thresholds),
                         detect_config["nms_iou_threshold"], detect_config["yolo_max_boxes"],
                         detect_config.get("input_weights_path"), weights)
    model.model.set_i8_calibration(detect_config.get("i8_calibration"))   # optional key, needed with dtype i8: the file of tools/calibrate_i8.py
    model.model.set_dtype(detect_config.get("dtype"))     # optional key: f32 | bf16 | f16 | i8; absent: f32
    model.model.set_stem_fusion_f16(detect_config.get("f16_fused_stem"))   # optional key, acts on dtype f16 only; absent: off
    model.model.set_tiny_stem_fusion(detect_config.get("tiny_fused_stem"))   # optional key, the fused stem of YOLOv3-tiny (f32, bf16, f16); absent: off
    model.model.set_pools_i8(detect_config.get("i8_pools"))   # optional key, the pools, up-sample and concat of an i8 plan on int8 tensors (YOLOv3-tiny); absent: off
    model.model.set_nms_per_class(nms_per_class)          # the device net's detect, and the composed route of loss=True, follow it
    model.model.set_multi_label(multi_label, multi_label_capacity)   # multi-label detections: the device net's streams follow it
    model.model.set_tiles(*(tiles or (None,)))            # sliced inference: the device net's streams follow it
    net = model.model._device_net()
    if net.image_size != S or net.max_batch < batch_size:
        net.plan(max(batch_size, net.max_batch), S)
    dataset = parse_tfrecords(detect_config["tfrecords_dir"], image_size=S, max_bboxes=detect_config["yolo_max_boxes"],
                              class_file=detect_config["classes_name_file"])
    max_boxes = int(detect_config["yolo_max_boxes"])
    truths = collections.deque()       # ground truth of the batches the stream has drawn and not yet counted (at most its depth)

    def frames():
        """One list of float32 [S,S,3] frames in [0,1] per batch (mode 0: the stage's resize to S x S is the identity), read
        from the records as the stream asks for them; its ground truth is queued beside it."""
        images, gt = [], []
        for n, (image, y) in enumerate(dataset):
            if max_batches is not None and n >= max_batches * batch_size:
                break
            y = y[y[..., 4] == 1]          # rows whose objectness column is 1: drops the zero padding (prepare_dataset)
            images.append(image)
            gt.append((y[:, 0:4], y[:, 5].astype(np.int32)))
            if len(images) == batch_size:
                truths.append(gt)
                yield images
                images, gt = [], []
        if images:
            truths.append(gt)
            yield images

    def ground_truth():
        while truths:
            yield truths.popleft()

    out = net.evaluate_stream(frames(), ground_truth(), anchors_table, max_boxes, detect_config["nms_iou_threshold"],
                              thresholds, nclasses, evaluate_iou_threshold=evaluate_iou_threshold,
                              one_class="both" if one_class else False, mode=0, max_batch=batch_size,
                              max_blob_bytes=batch_size * (S * S * 12 + 16), max_gt=max_boxes, loss=loss, ap=ap)
    out, ap_result = (out[:-1], out[-1]) if ap is not None else (out, None)
    if ap is not None:
        out = out if loss else out[0]
    out, loss_sums = out if loss else (out, None)
    plain, one = out if one_class else (out, None)
    results = []
    for t, threshold in enumerate(thresholds):
        counters = counters_from_row(plain[t], nclasses)
        counters_oneclass = counters_from_row(one[t], nclasses) if one_class else EvaluateDetections(nclasses, evaluate_iou_threshold).counters
        recall, precision = calc_recal_precision(counters)
        results.append((threshold, recall, precision, counters, counters_oneclass))
    if loss:
        report_loss(loss_sums)
    if ap is not None:
        from .runtime import ap_iou_thresholds
        report_ap(ap_result, ap_iou_thresholds(ap))
    if loss or ap is not None:
        return (results,) + ((loss_sums,) if loss else ()) + ((ap_result,) if ap is not None else ())
    return results


def evaluate(detect_config, evaluate_nms_score_thresholds, evaluate_iou_threshold=0.5, max_batches=20, weights=None,
             one_class=True, on_device=False, loss=False, ap=None, nms_per_class=False, tiles=None, multi_label=False,
             multi_label_capacity=0):
    """The loop of reference evaluate_yolov3.py:153-232: for every score threshold build the detect model, run the
    first `max_batches` dataset batches (`dataset.take(20)` there), count, and report (recall, precision).
    Returns [(threshold, recall, precision, counters, counters_oneclass)].
    on_device=True: the same list from one model and ONE pass over the data set -- the detections at a higher score threshold
    are the rows with score > threshold of the lowest threshold's, so every batch is detected once and the counters of all
    thresholds are counted on the GPU (Net.evaluate_stream).  That route batches the un-stacked data set itself: images with
    unlike numbers of boxes may share a batch, which the host route cannot stack.
    loss=True (with on_device=True): the same pass also computes the validation loss of reference core/loss_func.py on the GPU;
    val_loss, perGrid and perSource[xy,wh,obj,class] are printed as the reference's eager loop prints them (train.py:86-91) and
    the return value becomes (results, {"sum": float64 [3,4], "images": int, "errors": int}) as Net.evaluate_stream gives it.
    The regulariser (model.losses, decay_factor) that the reference's totLoss includes is not part of it.
    ap=True or a sequence of IoU thresholds (with on_device=True): COCO-style average precision from the same pass, matched on the
    GPU (Net.evaluate_stream, ap=; True means the ten thresholds 0.5 ... 0.95).  AP50, AP75 (when those thresholds are present) and
    mAP are printed and the dict of evaluate_detections.average_precision is returned after the existing results: (results, ap)
    or (results, loss, ap).  AP is no reference counterpart; it is taken over the detections at the LOWEST of
    evaluate_nms_score_thresholds, with the class ids as they are (the plain variant, whatever one_class says).
    An optional `dtype: f32 | bf16 | f16` key of detect_config selects the conv arithmetic of the on_device pass (absent: f32);
    an optional `f16_fused_stem: true` runs the first convs of an f16 plan as the fused stem kernel (absent: off);
    an optional `tiny_fused_stem: true` runs the stem of the YOLOv3-tiny model as its fused kernel (absent: off), with which that model
    also takes `dtype: bf16` and `dtype: f16`; an optional `i8_pools: true` on top of it lets that model take `dtype: i8` (absent: off).
    nms_per_class=True, or an optional `nms_per_class: true` key of detect_config (absent: off), on either route: per-class NMS
    (Net.nms_per_class; no reference counterpart) -- a box is suppressed only by a kept box of its own class, the rule published
    YOLOv3 mAP figures are taken under.  The one-pass argument of on_device=True holds as it stands: a box is never affected by a
    box scored below it under either rule.
    tiles=(rows, cols, overlap_px, overview) (with on_device=True), or the optional keys `tiles: [rows, cols]`, `tile_overlap`,
    `tile_overview` of detect_config: sliced inference (Net.evaluate_stream, tiles=) -- every record, resized to image_size on the host as
    before, is cut into windows on the device, each window is detected at image_size and the windows' detections are merged by a second
    NMS; the counters and the AP are taken on the merged rows.  One pass still serves every threshold ("Sliced inference").
    Not together with loss=True.
    multi_label=True (with on_device=True), or the optional key `multi_label: true` of detect_config; multi_label_capacity / the key of
    that name: the candidate slots per image, 0 = every box.  Multi-label detections (Net.multi_label; no reference counterpart): every
    pair (box, class) with conf * prob above the score threshold is a detection of its own, as Darknet's detector and the published
    YOLOv3 protocol have it.  One pass still serves every threshold unless an image has more candidates than the capacity at the lowest
    threshold; Net.evaluate_stream raises then.  The host route refuses the key: its per-threshold loop has no multi-label form."""
    from .inference import Inference
    multi_label = bool(multi_label or detect_config.get("multi_label"))
    multi_label_capacity = int(multi_label_capacity or detect_config.get("multi_label_capacity") or 0)
    if multi_label and not on_device:
        raise ValueError("evaluate: multi_label needs on_device=True (the candidates are formed on the GPU, in the device pass)")
    if multi_label_capacity and not multi_label:
        raise ValueError("evaluate: multi_label_capacity needs multi_label")
    tiles = tiles or Inference.tiles_from_config(detect_config)
    if tiles is not None and not on_device:
        raise ValueError("evaluate: tiles need on_device=True (the windows are cut and merged on the GPU, in the device pass)")
    if tiles is not None and loss:
        raise ValueError("evaluate: loss=True cannot be combined with tiles")
    if loss and not on_device:
        raise ValueError("evaluate: loss=True needs on_device=True (the loss is computed on the GPU, from the device pass)")
    ap = None if ap is False else ap
    if ap is not None and not on_device:
        raise ValueError("evaluate: ap needs on_device=True (the detections are matched on the GPU, in the device pass)")
    anchors_table = np.asarray(get_anchors(detect_config["anchors_file"]), np.float32)
    class_names = [c.strip() for c in open(detect_config["classes_name_file"]).readlines()]
    nclasses = len(class_names)
    nms_per_class = bool(nms_per_class or detect_config.get("nms_per_class"))
    if on_device:
        return _evaluate_on_device(detect_config, list(evaluate_nms_score_thresholds), evaluate_iou_threshold, max_batches, weights,
                                   one_class, anchors_table, nclasses, loss=loss, ap=ap, nms_per_class=nms_per_class, tiles=tiles,
                                   multi_label=multi_label, multi_label_capacity=multi_label_capacity)
    dataset = prepare_dataset(detect_config["tfrecords_dir"], detect_config["batch_size"], detect_config["image_size"],
                              detect_config["yolo_max_boxes"], detect_config["classes_name_file"])
    results = []
    for nms_score_threshold in evaluate_nms_score_thresholds:
        model = create_model(detect_config["model_config_file"], nclasses, anchors_table, nms_score_threshold,
                             detect_config["nms_iou_threshold"], detect_config["yolo_max_boxes"],
                             detect_config.get("input_weights_path"), weights)
        model.model.set_nms_per_class(nms_per_class)
        eval_detections = EvaluateDetections(nclasses, evaluate_iou_threshold)
        eval_detections_oneclass = EvaluateDetections(nclasses, evaluate_iou_threshold)
        for n, (batch_images, batch_gt_y) in enumerate(dataset):
            if max_batches is not None and n >= max_batches:
                break
            out = model.predict(batch_images)
            bboxes_batch, classes_batch, gt_bboxes_batch, gt_classes_batch = arrange_predict_output(*out, batch_gt_y)
            for pred_bboxes, pred_classes, gt_bboxes, gt_classes in zip(bboxes_batch, classes_batch, gt_bboxes_batch,
                                                                        gt_classes_batch):
                eval_detections.evaluate(pred_bboxes, pred_classes, gt_bboxes, gt_classes)
                if one_class:   # boxes only: every class id forced to 0
                    eval_detections_oneclass.evaluate(pred_bboxes, np.zeros_like(pred_classes), gt_bboxes,
                                                      np.zeros_like(gt_classes))
        recall, precision = calc_recal_precision(eval_detections.counters)
        results.append((nms_score_threshold, recall, precision, eval_detections.counters,
                        eval_detections_oneclass.counters))
    return results


def _arg_parser():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="config/detect_config.yaml")
    ap.add_argument("--evaluate-config", default="config/evaluate_config.yaml")
    ap.add_argument("--on-device", action="store_true",
                    help="one pass over the data set for all thresholds, counters computed on the GPU")
    ap.add_argument("--loss", action="store_true",
                    help="with --on-device: also val_loss, perGrid and perSource[xy,wh,obj,class] from the same pass")
    ap.add_argument("--ap", action="store_true",
                    help="with --on-device: also COCO-style AP50, AP75 and mAP from the same pass (IoU thresholds: the optional "
                         "evaluate_ap_iou_thresholds key of the evaluate config, by default 0.5, 0.55, ..., 0.95)")
    ap.add_argument("--tiny-fused-stem", action="store_true",
                    help="with --on-device: the stem of the YOLOv3-tiny model as one fused kernel, with which that model also runs in "
                         "dtype bf16 and f16 (also the optional tiny_fused_stem key of the detect config; absent: off)")
    ap.add_argument("--i8-pools", action="store_true",
                    help="with --on-device: a dtype i8 plan runs the pools, the up-sample and the concat behind its cut on int8 tensors, with "
                         "which (and --tiny-fused-stem) the YOLOv3-tiny model runs in dtype i8 (also the optional i8_pools key of the detect "
                         "config; absent: off)")
    ap.add_argument("--nms-per-class", action="store_true",
                    help="per-class NMS: a box is suppressed only by a kept box of its own class (also the optional nms_per_class "
                         "key of either config; absent: the reference's class-agnostic rule)")
    ap.add_argument("--multi-label", action="store_true",
                    help="with --on-device: every (box, class) pair above the score threshold is a detection of its own (also the optional "
                         "multi_label key of either config; absent: one label per box)")
    ap.add_argument("--multi-label-capacity", type=int, default=0, metavar="K",
                    help="with --multi-label: candidate slots per image (also the optional multi_label_capacity key); 0: every box")
    ap.add_argument("--tiles", type=int, nargs=2, metavar=("R", "C"),
                    help="with --on-device: sliced inference, every frame cut into R x C overlapping windows that are detected at full "
                         "resolution and merged on the GPU (also the optional tiles / tile_overlap / tile_overview keys of the detect config)")
    ap.add_argument("--tile-overlap", type=int, default=0, metavar="P", help="with --tiles: neighbouring windows overlap by at least P pixels")
    ap.add_argument("--tile-overview", action="store_true", help="with --tiles: the whole frame as one more tile")
    return ap


def main(argv=None):
    ap = _arg_parser()
    a = ap.parse_args(argv)
    if a.loss and not a.on_device:
        ap.error("--loss needs --on-device")
    if a.ap and not a.on_device:
        ap.error("--ap needs --on-device")
    if a.tiles and not a.on_device:
        ap.error("--tiles needs --on-device")
    if a.tiny_fused_stem and not a.on_device:
        ap.error("--tiny-fused-stem needs --on-device")
    if a.i8_pools and not a.on_device:
        ap.error("--i8-pools needs --on-device")
    if a.multi_label and not a.on_device:
        ap.error("--multi-label needs --on-device")
    if a.multi_label_capacity and not a.multi_label:
        ap.error("--multi-label-capacity needs --multi-label")
    if (a.tile_overlap or a.tile_overview) and not a.tiles:
        ap.error("--tile-overlap / --tile-overview need --tiles")
    if a.tiles and a.loss:
        ap.error("--tiles cannot be combined with --loss")
    with open(a.evaluate_config) as s:
        evaluate_config = yaml.safe_load(s)
    thresholds = evaluate_config["evaluate_nms_score_thresholds"]
    ap_thresholds = (evaluate_config.get("evaluate_ap_iou_thresholds") or True) if a.ap else None
    with open(a.config) as s:
        detect_config = yaml.safe_load(s)
    if a.tiny_fused_stem:
        detect_config["tiny_fused_stem"] = True
    if a.i8_pools:
        detect_config["i8_pools"] = True
    results = evaluate(detect_config, thresholds, on_device=a.on_device, loss=a.loss, ap=ap_thresholds,
                       nms_per_class=a.nms_per_class or bool(evaluate_config.get("nms_per_class")),
                       tiles=(a.tiles[0], a.tiles[1], a.tile_overlap, a.tile_overview) if a.tiles else None,
                       multi_label=a.multi_label or bool(evaluate_config.get("multi_label")),
                       multi_label_capacity=a.multi_label_capacity or int(evaluate_config.get("multi_label_capacity") or 0))
    if a.loss or a.ap:
        results = results[0]      # the loss and the AP have been printed by evaluate
    print([(t, float(r.mean()), float(p.mean())) for t, r, p, _, _ in results])


if __name__ == "__main__":
    main()
