"""Counterpart of the reference's only working caller (reference: inference.py:19-201).

Same YAML keys (`config/detect_config_coco.yaml` of the reference works unchanged apart from the weight
file format), same 5-tuple per batch, same per-image gather and the same `detect.txt` line payload
(`str([(label_str, xmin, ymin, xmax, ymax), ...])`, reference: core/render_utils.py:91, inference.py:39-41).
The composite model image -> (bboxes, class_indices, scores, selected_indices_padded, num_valid) runs as
conv program -> fused decode/score -> NMS on the GPU.  Rendering stays on the CPU with Pillow.
"""
from __future__ import annotations

import os

import numpy as np
import yaml

from .core.parse_model import Input, ParseModel
from .core.utils import dir_filelist, get_anchors, load_image_u8


class DetectModel:
    """Model(inputs, nms_output, name="yolo_nms") of reference inference.py:109-117: the composition
    `model(inputs)` -> `yolo_decode(grids, anchors_table, nclasses)` -> `YoloNmsLayer(max, iou, score)(decoded)`
    through the plugin surface (core/yolo_decode_layer.py, core/yolo_nms_layer.py), exactly as the reference wires it.
    fused=True runs the same arithmetic as one decode+score kernel that never materialises the [B,N,nclasses]
    probabilities (what bench.py and y3_net_detect use); both give identical tuples."""

    def __init__(self, model, anchors_table, nclasses, yolo_max_boxes, nms_iou_threshold, nms_score_threshold,
                 fused=False):
        from .core.yolo_nms_layer import YoloNmsLayer
        self.model = model
        self.anchors_table = np.asarray(anchors_table, np.float32)
        self.nclasses = nclasses
        self.yolo_max_boxes = int(yolo_max_boxes)
        self.nms_iou_threshold = float(nms_iou_threshold)
        self.nms_score_threshold = float(nms_score_threshold)
        self.fused = bool(fused)
        self.nms_layer = YoloNmsLayer(self.yolo_max_boxes, self.nms_iou_threshold, self.nms_score_threshold)

    def __call__(self, images):
        """images: [B,S,S,3] fp32 (numpy or CUDA tensor) -> the 5-tuple as CUDA tensors."""
        grids = self.model(images)
        per_class = bool(getattr(self.model, "nms_per_class", False))      # the model's switch (set_nms_per_class), read per call
        multi = bool(getattr(self.model, "multi_label", False))            # the model's switch (set_multi_label), read per call
        if multi and self.fused:
            return self._multi_label(grids, per_class)
        if self.fused:
            from . import ops, runtime
            bboxes, cls, scores = runtime.yolo_decode_scores(grids, self.anchors_table, self.nclasses)
            sel, nv = ops._nms(bboxes, scores, self.yolo_max_boxes, self.nms_iou_threshold, self.nms_score_threshold,
                               classes=cls if per_class else None)
            return bboxes, cls, scores, sel, nv
        from .core.yolo_decode_layer import yolo_decode
        decoded_output = yolo_decode(grids, self.anchors_table, self.nclasses)      # reference: inference.py:111
        self.nms_layer.per_class = per_class
        self.nms_layer.multi_label, self.nms_layer.multi_label_capacity = multi, int(getattr(self.model, "multi_label_capacity", 0))
        return self.nms_layer(decoded_output)                                        # reference: inference.py:114-115

    def _multi_label(self, grids, per_class):
        """The 5-tuple OVER CANDIDATES (multilabel.py): every pair (box, class) above the score threshold is a candidate of its own ->
        (cand_bboxes [B,K,4], cand_classes [B,K] i64, cand_scores [B,K], selected_indices_padded, num_valid_detections), so that
        Inference.gather_valid_detections_results works unchanged.  K: the model's multi_label_capacity, 0 = every box."""
        from . import ops
        N = sum(3 * g.shape[1] * g.shape[2] for g in grids)
        K = int(getattr(self.model, "multi_label_capacity", 0)) or N
        boxes, cls, scores, _, _ = ops.decode_candidates(grids, self.anchors_table, self.nclasses, self.nms_score_threshold, K)
        sel, nv = ops._nms(boxes, scores, self.yolo_max_boxes, self.nms_iou_threshold, self.nms_score_threshold,
                           classes=cls if per_class else None)
        return boxes, cls, scores, sel, nv

    def predict(self, images, **_):
        return tuple(t.cpu().numpy() for t in self(images))


class Inference:
    # fp16 plans with the fused stem kernel (runtime.Net.set_stem_fusion_f16; None: off).  The optional YAML key `f16_fused_stem` of the
    # inference config lands here (main()); __call__ keeps the reference's keys plus the two every plan has, low_latency and dtype.
    f16_fused_stem = None
    # The fused stem kernel of YOLOv3-tiny (runtime.Net.set_tiny_stem_fusion; None: off), with which the tiny model also runs in dtype bf16
    # and f16.  The optional YAML key `tiny_fused_stem` lands here the same way.
    tiny_fused_stem = None
    # Stand-alone ops of dtype i8 plans on int8 tensors (runtime.Net.set_pools_i8; None: off), with which -- and with tiny_fused_stem -- the
    # tiny model runs in dtype i8.  The optional YAML key `i8_pools` lands here the same way.
    i8_pools = None
    # Per-class NMS (core.parse_model.YoloModel.set_nms_per_class; None or False: the reference's class-agnostic rule).  The optional YAML
    # key `nms_per_class` lands here the same way.
    nms_per_class = None
    # Multi-label detections (core.parse_model.YoloModel.set_multi_label; None or False: one label per box).  The optional YAML keys
    # `multi_label: true` and `multi_label_capacity: <int>` land here the same way.
    multi_label = None
    multi_label_capacity = 0
    # Sliced inference (core.parse_model.YoloModel.set_tiles; None: off): (rows, cols, overlap_px, overview).  The optional YAML keys
    # `tiles: [rows, cols]`, `tile_overlap: <pixels>` and `tile_overview: true|false` land here the same way (tiles_from_config).
    tiles = None

    @staticmethod
    def tiles_from_config(config, pop=False):
        """The optional keys tiles / tile_overlap / tile_overview of a config dict -> (rows, cols, overlap_px, overview), or None when
        `tiles` is absent.  pop: take the three keys out of the dict."""
        get = config.pop if pop else config.get
        grid, overlap, overview = get("tiles", None), get("tile_overlap", None), get("tile_overview", None)
        if grid is None:
            if overlap is not None or overview is not None:
                raise ValueError("tile_overlap / tile_overview need `tiles: [rows, cols]`")
            return None
        if len(grid) != 2:
            raise ValueError(f"tiles must be [rows, cols] (got {grid!r})")
        return int(grid[0]), int(grid[1]), int(overlap or 0), bool(overview)

    def _detect_tiled(self, model, frames, mode):
        """Sliced inference of one batch of host frames (uint8 [H,W,3|4]) through the device net's detect_stream -> per frame
        (bboxes [n,4], classes [n], scores [n]), the boxes normalised to the frame."""
        net = model.model._device_net()
        (packed, nv), = net.detect_stream([frames], model.anchors_table, model.yolo_max_boxes, model.nms_iou_threshold,
                                          model.nms_score_threshold, mode=mode)      # the net's `tiles` property is the model's
        out = []
        for rows, n in zip(packed, nv):
            rows = rows[:int(n)]
            out.append((rows[:, :4].copy().view(np.float32), rows[:, 5].astype(np.int64), rows[:, 4].copy().view(np.float32)))
        return out

    @staticmethod
    def gather_valid_detections_results(bboxes_padded, class_indices_padded, scores_padded, selected_indices_padded,
                                        num_valid_detections):
        # reference: inference.py:21-28
        sel = selected_indices_padded[:num_valid_detections]
        return bboxes_padded[sel], class_indices_padded[sel], scores_padded[sel]

    @staticmethod
    def _dump_detections_text(image_detections_result, detections_list_outfile):
        detections_list_outfile.write(f"{image_detections_result}\n")
        detections_list_outfile.flush()

    @staticmethod
    def annotate(image, bboxes, classes_names, scores, font_size):
        """Boxes + '<class>: <score>%' labels; returns (PIL image, detections list) with the reference's
        per-detection tuple (label, xmin, ymin, xmax, ymax) in pixels of `image` (core/render_utils.py:71-91)."""
        from PIL import Image, ImageDraw
        pil = Image.fromarray(np.uint8(np.clip(image, 0, 1) * 255)).convert("RGB")
        draw = ImageDraw.Draw(pil)
        w, h = pil.size
        detections = []
        for bbox, name, score in zip(bboxes, classes_names, scores):
            xmin, ymin, xmax, ymax = (float(v) for v in bbox * np.array([w, h, w, h], np.float32))
            label = "{}: {}%".format(name, int(100 * score))
            draw.rectangle([(xmin, ymin), (max(xmax, xmin), max(ymax, ymin))], outline=(255, 255, 255))
            draw.text((max(xmin, 0), max(ymin, 0)), label, fill=(255, 255, 0))
            detections.append((label, xmin, ymin, xmax, ymax))
        return pil, detections

    @staticmethod
    def canvas_and_anchors(image_size, anchors_table):
        """image_size of the config -- an int S, or [H, W] for a rectangular network input (both multiples of 32) -- and the
        anchors of the anchors file -> ((H, W), the anchors for that canvas).  Convention: the anchors file is normalised by
        the square side the model was trained at, and for an [H, W] canvas that side is taken to be max(H, W), the long side
        (what runtime.rect_canvas keeps at image_size): the anchors are rescaled per axis (runtime.rect_anchors), the long
        axis is left as the file has it.  An int, or H == W, leaves the anchors untouched."""
        from . import runtime
        canvas_h, canvas_w = runtime.canvas_hw(image_size)
        anchors_table = np.asarray(anchors_table, np.float32)
        if canvas_h != canvas_w:
            anchors_table = runtime.rect_anchors(anchors_table, max(canvas_h, canvas_w), (canvas_h, canvas_w))
        return (canvas_h, canvas_w), anchors_table

    def build(self, model_config_file, classes_name_file, anchors_file, input_weights_path, yolo_max_boxes,
              nms_iou_threshold, nms_score_threshold, weights=None, low_latency=None, dtype=None, f16_fused_stem=None,
              i8_calibration=None):
        """low_latency (optional YAML key; None or absent: off): plan the network for latency at one to eight images -- the
        fp32 convs that leave most of the chip idle at such a batch are split along K (runtime.Net.set_low_latency).
        dtype (optional YAML key: f32 | bf16 | f16 | i8; None or absent: f32): the conv arithmetic (runtime.Net.set_dtype).
        i8_calibration (optional YAML key, needed with dtype i8): the file of activation scales tools/calibrate_i8.py wrote.
        f16_fused_stem (optional YAML key; None or absent: what self.f16_fused_stem says, off by default): with dtype f16, the first
        convs as the fused stem kernel (runtime.Net.set_stem_fusion_f16); without effect on any other dtype."""
        anchors_table = get_anchors(anchors_file).astype(np.float32)      # reference: inference.py:83
        class_names = [c.strip() for c in open(classes_name_file).readlines()]
        nclasses = len(class_names)
        with open(model_config_file, "r") as f:
            model_config = yaml.safe_load(f)
        from .graph import find_config_root
        model = ParseModel().build_model(Input(shape=(None, None, 3)), model_config["sub_models_configs"],
                                         model_config["output_stage"], nclasses=nclasses,
                                         config_root=find_config_root(model_config_file,
                                                                      model_config["sub_models_configs"]))
        with open("model_inference_summary.txt", "w") as f:
            model.summary(print_fn=lambda x: f.write(x + "\n"))
        if weights is not None:
            model.set_weights_dict(weights)
        else:
            model.load_weights(input_weights_path).expect_partial()
        model.set_low_latency(low_latency)
        model.set_i8_calibration(i8_calibration)
        model.set_dtype(dtype)
        model.set_stem_fusion_f16(self.f16_fused_stem if f16_fused_stem is None else f16_fused_stem)
        model.set_tiny_stem_fusion(self.tiny_fused_stem)
        model.set_pools_i8(self.i8_pools)
        model.set_nms_per_class(self.nms_per_class)
        model.set_multi_label(self.multi_label, int(self.multi_label_capacity or 0))
        model.set_tiles(*(self.tiles or (None,)))
        print("weights loaded")
        return DetectModel(model, anchors_table, nclasses, yolo_max_boxes, nms_iou_threshold,
                           nms_score_threshold), class_names

    def __call__(self, model_config_file, classes_name_file, anchors_file, input_weights_path, image_size,
                 input_data_source, images_dir, tfrecords_dir, batch_size, image_file_path, output_dir, yolo_max_boxes,
                 nms_iou_threshold, nms_score_threshold, bbox_color, font_size, display_result_images=None,
                 save_model_path=None, weights=None, low_latency=None, dtype=None, i8_calibration=None):
        os.makedirs(output_dir, exist_ok=True)
        detections_text_list_outfile = f"{output_dir}/detect.txt"
        try:
            os.remove(detections_text_list_outfile)
        except OSError:
            pass
        out = open(detections_text_list_outfile, "a")
        model, class_names = self.build(model_config_file, classes_name_file, anchors_file, input_weights_path,
                                        yolo_max_boxes, nms_iou_threshold, nms_score_threshold, weights, low_latency, dtype,
                                        i8_calibration=i8_calibration)
        self.detect_model = model    # the DetectModel of the last call (its .model is the YoloModel, ._device_net() the planned Net)
        results = []
        import torch
        from . import runtime
        (canvas_h, canvas_w), model.anchors_table = self.canvas_and_anchors(image_size, model.anchors_table)
        tiled = model.model.tiles is not None
        if tiled:       # sliced inference: the frames go to the device whole, the windows are cut, detected and merged there
            net = model.model._device_net()
            if net.canvas != (canvas_h, canvas_w):
                net.plan(max(net.max_batch, 1), (canvas_h, canvas_w) if canvas_h != canvas_w else canvas_h)
        if input_data_source == "tfrecords":
            # reference: inference.py:119-144.  Records are parsed on the host (core/load_tfrecords.py); the
            # resize(0..255 values) / 255 of parse_tfrecord_fn runs on the GPU straight into the batch tensor.  The
            # reference's following resize_image(img, S, S) sees an S x S image: scale 1, no padding -- the identity.
            from .core.load_tfrecords import decode_jpeg_u8, iter_examples
            image_index = 0   # running index (the reference numbers files within a batch, overwriting earlier ones)
            pend = []

            def run_batch(images_u8):
                nonlocal image_index
                if tiled:       # boxes in frame coordinates: drawn on the frame itself
                    for img, (bboxes, classes, scores) in zip(images_u8, self._detect_tiled(model, images_u8, 2)):
                        classes_names = [class_names[idx] for idx in classes]
                        annotated, detections = self.annotate(img[..., :3].astype(np.float32) / 255.0, bboxes, classes_names, scores, font_size)
                        self._dump_detections_text(detections, out)
                        annotated.save(f"{output_dir}/detect_{image_index}.jpg")
                        results.append((bboxes, classes, scores, classes_names))
                        image_index += 1
                    return
                batch_dev = torch.empty((len(images_u8), canvas_h, canvas_w, 3), dtype=torch.float32,
                                        device="cuda")
                # one copy and one launch for the batch (mode 2: resize the 0..255 values, then / 255)
                blob, descs = runtime.pack_images(images_u8, 2)
                runtime.preprocess_batch(torch.from_numpy(blob).cuda(), descs, batch_dev)
                b_boxes, b_cls, b_scores, b_sel, b_nv = (t.cpu().numpy() for t in model(batch_dev))
                for bb, cc, ss, sel, nv, img in zip(b_boxes, b_cls, b_scores, b_sel, b_nv, batch_dev.cpu().numpy()):
                    bboxes, classes, scores = self.gather_valid_detections_results(bb, cc, ss, sel, int(nv))
                    classes_names = [class_names[idx] for idx in classes]
                    annotated, detections = self.annotate(img, bboxes, classes_names, scores, font_size)
                    self._dump_detections_text(detections, out)
                    annotated.save(f"{output_dir}/detect_{image_index}.jpg")
                    results.append((bboxes, classes, scores, classes_names))
                    image_index += 1

            for example in iter_examples(tfrecords_dir):
                pend.append(decode_jpeg_u8(example["image/encoded"][0]))
                if len(pend) == int(batch_size):
                    run_batch(pend)
                    pend = []
            if pend:
                run_batch(pend)
            filenames = []
        elif input_data_source == "image_file":
            filenames = [image_file_path]
        elif input_data_source == "images_dir":
            filenames = dir_filelist(images_dir, (".jpeg", ".jpg", ".png", ".bmp"))
        else:
            filenames = []
        for image_index, file in enumerate(filenames):
            # decode on the host, then uint8 -> [0,1] -> bilinear resize on the GPU straight into the batch tensor
            # (reference: inference.py:157-158 decode_image + tf.image.resize)
            orig_image = load_image_u8(file)
            if tiled:
                (bboxes, classes, scores), = self._detect_tiled(model, [orig_image], 1)
                classes_names = [class_names[idx] for idx in classes]
                annotated, detections = self.annotate(orig_image.astype(np.float32) / 255.0, bboxes, classes_names, scores, font_size)
                self._dump_detections_text(detections, out)
                annotated.save(f"{output_dir}/detect_{image_index}.jpg")
                results.append((bboxes, classes, scores, classes_names))
                continue
            batch_dev = torch.empty((1, canvas_h, canvas_w, 3), dtype=torch.float32, device="cuda")
            runtime.preprocess_image(torch.from_numpy(orig_image).cuda(), batch_dev, 0)
            b_boxes, b_cls, b_scores, b_sel, b_nv = (t.cpu().numpy() for t in model(batch_dev))
            batch = batch_dev.cpu().numpy()
            for bb, cc, ss, sel, nv, img in zip(b_boxes, b_cls, b_scores, b_sel, b_nv, batch):
                bboxes, classes, scores = self.gather_valid_detections_results(bb, cc, ss, sel, int(nv))
                classes_names = [class_names[idx] for idx in classes]
                annotated, detections = self.annotate(img, bboxes, classes_names, scores, font_size)
                annotated = annotated.resize((orig_image.shape[1], orig_image.shape[0]))
                self._dump_detections_text(detections, out)
                annotated.save(f"{output_dir}/detect_{image_index}.jpg")
                results.append((bboxes, classes, scores, classes_names))
        if results:
            bboxes, classes, scores, classes_names = results[-1]
            for class_name, bbox, score in zip(classes_names, bboxes, scores):
                print(f"{class_name} bbox: {bbox} score: {score}")
        out.close()
        return results


def main(argv=None):
    import argparse
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, default="config/detect_config.yaml", help="yaml config file")
    args = parser.parse_args(argv)
    with open(args.config, "r") as stream:
        detect_config = yaml.safe_load(stream)
    inference = Inference()
    inference.f16_fused_stem = detect_config.pop("f16_fused_stem", None)    # optional key, absent: off
    inference.tiny_fused_stem = detect_config.pop("tiny_fused_stem", None)  # optional key, absent: off
    inference.i8_pools = detect_config.pop("i8_pools", None)                # optional key, absent: off
    inference.nms_per_class = detect_config.pop("nms_per_class", None)      # optional key, absent: off
    inference.multi_label = detect_config.pop("multi_label", None)          # optional keys, absent: off, every box of the plan
    inference.multi_label_capacity = detect_config.pop("multi_label_capacity", 0)
    inference.tiles = Inference.tiles_from_config(detect_config, pop=True)  # optional keys tiles / tile_overlap / tile_overview, absent: off
    inference(**detect_config)


if __name__ == "__main__":
    main()
