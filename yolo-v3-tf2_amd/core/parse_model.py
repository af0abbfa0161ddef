"""Host mirror of the reference's graph builder (reference: core/parse_model.py).

`ParseModel().build_model(model_inputs, sub_models_configs, output_stage, decay_factor, nclasses)`
keeps the reference's name, argument meaning and error behaviour (ValueError for an unknown layer
type or a route with more than two sources, AssertionError for a bad activation, Exception for a
missing source sub-model) but returns a `YoloModel` whose forward pass is the fused HIP conv program
instead of a Keras functional graph.  There is no CPU fallback: calling the model without a GPU or
without liby3hip.so raises.
"""
from __future__ import annotations

import os

import numpy as np
import yaml

from ..graph import build_program
from .. import weights as _weights


class Input:
    """Placeholder standing in for tensorflow.keras.Input (reference: inference.py:87)."""

    def __init__(self, shape=(None, None, 3), name="input", **_):
        self.shape = tuple(shape)
        self.name = name


class _LoadStatus:
    def expect_partial(self):  # reference: inference.py:102
        return self


_DEFERRED_DEFAULTS = {"set_low_latency": False, "set_low_latency_f16": False, "set_low_latency_i8": False, "set_stem_fusion_f16": 0,
                      "set_tiny_stem_fusion": 0, "set_pools_i8": 0,
                      "load_calibration": None, "set_dtype": None}


class YoloModel:
    """Callable network: image batch [B,S,S,3] (fp32, NHWC, values in [0,1]) -> [grid13, grid26, grid52],
    each [B,g,g,3,5+nclasses] (reference: the Keras Model returned by build_model, core/parse_model.py:313)."""

    def __init__(self, program, name="yolo"):
        self.program = program
        self.name = name
        self._net = None
        self._weights = None
        # the settings a device net is given when it is made, Net method -> argument, in the order they are applied: the low-latency
        # switches, stem fusion, the calibration file an "i8" plan needs, the dtype (None: fp32).  An entry at its value here is skipped.
        self._deferred = dict(_DEFERRED_DEFAULTS)
        self.nms_per_class = False      # set_nms_per_class: a property of the device net, not one of its methods, so kept beside them
        self.multi_label, self.multi_label_capacity = False, 0      # set_multi_label: the device net's properties of those names
        self.tiles = None               # set_tiles: (rows, cols, overlap_px, overview), the device net's property of that name

    def __getattr__(self, name):     # the settings read as attributes: low_latency, ..., stem_fusion_f16, tiny_stem_fusion, pools_i8, i8_calibration, dtype
        method = {"i8_calibration": "load_calibration"}.get(name, "set_" + name)
        if method in _DEFERRED_DEFAULTS and "_deferred" in self.__dict__:
            return self._deferred[method]
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    # lazily create the device object so that building/inspecting a model works without a GPU
    def _device_net(self):
        if self._net is None:
            from ..runtime import Net
            self._net = Net(self.program)
            for method, arg in self._deferred.items():
                if arg != _DEFERRED_DEFAULTS[method]:
                    getattr(self._net, method)(arg)
            self._net.nms_per_class = self.nms_per_class
            self._net.multi_label_capacity, self._net.multi_label = self.multi_label_capacity, self.multi_label
            self._net.tiles = self.tiles
            if self._weights is not None:
                self._net.load_weights(self._weights)
        return self._net

    def _defer(self, method, arg):
        """Record a validated setting and, when the device net exists, apply it (an unset one is not: there is nothing to undo)."""
        self._deferred[method] = arg
        if self._net is not None and (method.startswith("set_") or arg != _DEFERRED_DEFAULTS[method]):
            getattr(self._net, method)(arg)

    def set_low_latency(self, on=True):
        """Low-latency fp32 plans (runtime.Net.set_low_latency): split-K convs for batches of one to eight images.  Takes
        effect at the next plan, i.e. before the first call or when the batch shape changes."""
        from ..runtime import Net
        self._defer("set_low_latency", Net._low_latency_arg(on))

    def set_low_latency_f16(self, on=True):
        """Low-latency fp16 plans (runtime.Net.set_low_latency_f16): the same for plans made with dtype "f16"."""
        from ..runtime import Net
        self._defer("set_low_latency_f16", Net._low_latency_arg(on))

    def set_low_latency_i8(self, on=True):
        """Low-latency int8 plans (runtime.Net.set_low_latency_i8): the same for plans made with dtype "i8"."""
        from ..runtime import Net
        self._defer("set_low_latency_i8", Net._low_latency_arg(on))

    def set_stem_fusion_f16(self, on=True):
        """The fused stem kernel for fp16 plans (runtime.Net.set_stem_fusion_f16): off by default; acts on dtype "f16" only."""
        from ..runtime import Net
        self._defer("set_stem_fusion_f16", Net._stem_fusion_arg(on))

    def set_tiny_stem_fusion(self, on=True):
        """The fused stem kernel of YOLOv3-tiny (runtime.Net.set_tiny_stem_fusion): off by default; with it the tiny model also plans in
        dtype "bf16" and "f16".  Ignored by a program that does not start with tiny's stem.  Takes effect at the next plan."""
        from ..runtime import Net
        self._defer("set_tiny_stem_fusion", Net._tiny_stem_arg(on))

    def set_pools_i8(self, on=True):
        """Stand-alone ops of dtype "i8" plans on int8 tensors (runtime.Net.set_pools_i8): off by default; with it, and with
        set_tiny_stem_fusion, the tiny model plans in dtype "i8".  Does nothing in any other dtype.  Takes effect at the next plan."""
        from ..runtime import Net
        self._defer("set_pools_i8", Net._pools_i8_arg(on))

    def set_nms_per_class(self, on=True):
        """Per-class NMS (runtime.Net.nms_per_class; no reference counterpart): a box is suppressed only by a kept box of its own
        class.  None or False: the reference's class-agnostic rule, the default.  The device net's detect / detect_stream /
        evaluate_stream and both routes of inference.DetectModel follow it."""
        if on is not None and not isinstance(on, (bool, np.bool_)):
            raise TypeError(f"set_nms_per_class: a bool or None (got {on!r})")
        self.nms_per_class = bool(on)
        if self._net is not None:
            self._net.nms_per_class = self.nms_per_class

    def set_multi_label(self, on=True, capacity=0):
        """Multi-label detections (runtime.Net.multi_label / multi_label_capacity; no reference counterpart): every pair (box, class)
        with conf * prob above the score threshold is a detection of its own, and the NMS of the model's rule decides between them.
        None or False: one label per box, the default.  capacity: candidate slots per image, 0 = every box of the plan.  The device
        net's detect / detect_stream / evaluate_stream and both routes of inference.DetectModel follow it."""
        if on is not None and not isinstance(on, (bool, np.bool_)):
            raise TypeError(f"set_multi_label: a bool or None (got {on!r})")
        if isinstance(capacity, (bool, np.bool_)) or not isinstance(capacity, (int, np.integer)) or capacity < 0:
            raise TypeError(f"set_multi_label: capacity must be an int >= 0 (got {capacity!r})")
        self.multi_label, self.multi_label_capacity = bool(on), int(capacity)
        if self._net is not None:
            self._net.multi_label_capacity, self._net.multi_label = self.multi_label_capacity, self.multi_label

    def set_tiles(self, rows=None, cols=None, overlap_px=0, overview=False):
        """Sliced inference (runtime.Net.detect_stream / evaluate_stream, tiles=; no reference counterpart): every frame is cut into
        rows x cols windows overlapping by at least overlap_px pixels, plus the whole frame with overview, each window runs through the
        network at full resolution and the windows' detections are merged on the device.  set_tiles(None), the default: off.  The device
        net's detect_stream / evaluate_stream follow it (runtime.Net.tiles), and through them inference.Inference and evaluate_yolov3."""
        if rows is None:
            tiles = None
        else:
            from ..tiles import tile_grid
            tiles = (int(rows), int(cols), int(overlap_px), bool(overview))
            tile_grid(max(tiles[2], 1), max(tiles[2], 1), *tiles)      # the grid's own checks on the smallest frame that takes the overlap (ValueError)
        self.tiles = tiles
        if self._net is not None:
            self._net.tiles = tiles

    def set_dtype(self, dtype):
        """Conv arithmetic of the plans (runtime.Net.set_dtype): None or "f32" (default), "bf16", "f16" -- 16-bit activations and
        weights on the matrix cores, fp32 accumulation, fp32 images in and fp32 grids out -- a plane-split mode, or "i8": calibrated
        int8 from the first conv that qualifies on (set_i8_calibration first: the plan needs the activation scales)."""
        from ..runtime import Net
        self._defer("set_dtype", Net._dtype_arg(dtype))

    def set_i8_calibration(self, path):
        """The calibration file (tools/calibrate_i8.py; runtime.Net.save_calibration) whose activation scales dtype "i8" plans with;
        None: none.  A file made for another graph is refused when the device net reads it."""
        self._defer("load_calibration", path or None)

    def set_weights_dict(self, weights):
        self._weights = weights
        if self._net is not None:
            self._net.load_weights(weights)

    def load_weights(self, path):
        """`.safetensors` (this package's container) or Darknet `.weights` (reference: convert.py:93-137).
        TensorFlow checkpoints cannot be read without TensorFlow."""
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        if path.endswith(".weights"):
            w = _weights.read_darknet_weights(path, self.program)
        elif path.endswith(".safetensors"):
            w = _weights.load_weights(path)
        else:
            raise ValueError(f"unsupported weight file {path!r}: use .safetensors or Darknet .weights")
        self.set_weights_dict(w)
        return _LoadStatus()

    def __call__(self, images, training=False):
        import torch
        if training:
            raise NotImplementedError("the HIP path is inference only")
        if self._weights is None:
            raise RuntimeError("model has no weights: call load_weights() or set_weights_dict() first")
        net = self._device_net()
        if isinstance(images, np.ndarray):
            images = torch.from_numpy(np.ascontiguousarray(images, np.float32)).cuda()
        return net.forward(images.contiguous())

    def predict(self, images, batch_size=None, **_):
        return [g.cpu().numpy() for g in self(images)]

    def summary(self, print_fn=print):
        p = self.program
        print_fn(f'Model: "{self.name}"')
        for n in p.conv_nodes:
            cin = p.tensors[n.inputs[0]].channels
            print_fn(f"conv{n.conv_index:<3d} {n.sub_model:<9s} {n.size}x{n.size}/{n.stride} {cin:>4d} -> {n.filters:<4d}"
                     f" {'bn' if n.bn else 'bias':<4s} {'leaky' if n.leaky else 'linear'}")
        print_fn(f"Total params: {p.n_params():,}")
        print_fn(f"GFLOP / image @416: {p.flops_per_image(416) / 1e9:.3f}")


class ParseModel:
    def build_model(self, model_inputs, sub_models_configs, output_stage="head", decay_factor=0, nclasses=0, **kwargs):
        """reference: core/parse_model.py:279-314.  `model_inputs` is accepted for signature compatibility
        (the input is always [B,S,S,3]); `decay_factor` only affects training in the reference."""
        in_ch = 3
        shape = getattr(model_inputs, "shape", None)
        if shape is not None and len(shape) >= 1 and shape[-1] not in (None, 3):
            raise ValueError("the HIP path expects 3-channel images")
        program = build_program(sub_models_configs, output_stage, nclasses, config_root=kwargs.get("config_root"),
                                in_channels=in_ch)
        return YoloModel(program)

    def create_model(self, nclasses, model_config_file):
        """reference: core/parse_model.py:316-322"""
        with open(model_config_file, "r") as f:
            cfg = yaml.safe_load(f)
        return self.build_model(Input(shape=(None, None, 3)), cfg["sub_models_configs"],
                                cfg.get("output_stage", "head"), nclasses=nclasses)
