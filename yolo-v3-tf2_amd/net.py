"""The device-side network: class Net over the y3_net_* entry points -- plan, switches, forward, detect, calibration and clock
measurement -- and the tile table a plan takes (tuning_table_path).  The streaming pipelines behind Net.detect_stream and
Net.evaluate_stream are in stream.py."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib, stream
from ._args import _anchors, _dev, _fptr, _images_arg, _need_cuda
from ._lib import AuxDesc, ConvDesc, TensorDesc, Y3Error, check
from .graph import AuxOp, ConvOp, Program
from .input_stage import canvas_hw
from .weights import BN_EPS, pad_weights

_AUX_KIND = {"add": _lib.Y3_AUX_ADD, "upsample": _lib.Y3_AUX_UPSAMPLE2X, "concat": _lib.Y3_AUX_CONCAT,
             "maxpool_s2": _lib.Y3_AUX_MAXPOOL2X2_S2, "maxpool_s1": _lib.Y3_AUX_MAXPOOL2X2_S1}
# plan dtype -> the suffix of its tile setter (y3_net_set_tile*): fp16 and int8 plans run the 16-bit conv family's tiles
_TILE_KIND = {_lib.Y3_DTYPE_F32: "", _lib.Y3_DTYPE_BF16: "_bf16", _lib.Y3_DTYPE_F32X3: "_x3", _lib.Y3_DTYPE_F32X2: "_x2",
              _lib.Y3_DTYPE_F16: "_bf16", _lib.Y3_DTYPE_I8: "_bf16"}


def tuning_table_path(tag: str, batch: int, image_size) -> str:
    """The tile table of a plan: tuning/<mode>_b<batch>_s<size>.json of the package (may not exist: heuristic tiles).
    Y3_TUNING_FILE (tools: A/B of tables) replaces it only for the plan it was made for: the file names its mode
    ("dtype": "f32" | "bf16" | "f32x3" | "f32x2") and its batch / image_size; a plan of another mode or geometry in the
    same process (bench.py's alt measurements re-plan the net) keeps its own packaged table.
    A non-square (H, W) plan takes the table of (mode, batch, max(H, W)), every row of it (Net.conv_signature is formed at
    max(H, W) as well): tile validity depends on channel counts only; whether those tiles are the fastest for the smaller M is
    unmeasured."""
    import json
    import os
    from . import PACKAGE_DIR
    image_size = max(canvas_hw(image_size))
    path = os.path.join(PACKAGE_DIR, "tuning", f"{tag}_b{batch}_s{image_size}.json")
    override = os.environ.get("Y3_TUNING_FILE")
    if override and os.path.exists(override):
        with open(override) as f:
            odoc = json.load(f)
        if odoc.get("dtype") == tag and int(odoc.get("batch", -1)) == batch and int(odoc.get("image_size", -1)) == image_size:
            path = override
    return path


class _TinyStemSwitch:
    """The fused stem of YOLOv3-tiny (include/y3.h, y3_net_set_tiny_stem_fusion; csrc/conv_tiny_stem.hip): the part of Net's interface that
    came with it, kept in a base of its own."""

    @staticmethod
    def _tiny_stem_arg(on) -> int:
        if on is None:
            return 0
        if isinstance(on, (bool, np.bool_, int, np.integer)) and int(on) in (0, 1):
            return int(on)
        raise Y3Error(f"tiny stem fusion must be None, a bool, 0 or 1 (got {on!r})")

    def set_tiny_stem_fusion(self, on=True):
        """conv0 + pool 0 + conv1 + pool 1 of YOLOv3-tiny as one kernel: off by default; None means off.  Before plan(): on a planned net it
        waits for the next plan.  Acts on fp32, bf16
        and fp16 plans of a program that starts with that stem and is ignored on any other; with it tiny plans in bf16 and fp16, which
        refuse it otherwise.  keep_activations() does not switch it off: the three tensors inside the launch are not stored, and
        read_tensor on one of them raises.  set_stem_fusion / set_stem_fusion_f16 do not act on it, nor it on them."""
        on = self._tiny_stem_arg(on)            # the argument check comes first: it needs no device net
        check(self.lib.y3_net_set_tiny_stem_fusion(self._h, on), "y3_net_set_tiny_stem_fusion")

    @property
    def tiny_stem_fused(self) -> int:
        """1 when the planned net runs the fused tiny stem launch (y3_net_get_tiny_stem_fused), 0 otherwise, also before plan()."""
        return int(self.lib.y3_net_get_tiny_stem_fused(self._h))


class _PoolsI8Switch:
    """Stand-alone ops of an int8 plan (include/y3.h, y3_net_set_pools_i8: the max-pools, the up-sample and the concat of YOLOv3-tiny on
    int8 tensors behind the cut): the part of Net's interface that came with it, kept in a base of its own."""

    @staticmethod
    def _pools_i8_arg(on) -> int:
        if on is None:
            return 0
        if isinstance(on, (bool, np.bool_, int, np.integer)) and int(on) in (0, 1):
            return int(on)
        raise Y3Error(f"pools_i8 must be None, a bool, 0 or 1 (got {on!r})")

    def set_pools_i8(self, on=True):
        """An "i8" plan runs the max-pools, up-samples and concats behind its cut on int8 tensors instead of refusing a net that holds a
        pool: off by default; None means off.  Before plan(): on a planned net it waits for the next plan.  Does nothing in any other
        dtype.  YOLOv3-tiny needs set_tiny_stem_fusion as well (the part before the cut is an fp16 plan), and scales for the tensors the
        aux ops write (calibrate_i8 with this switch on measures them)."""
        on = self._pools_i8_arg(on)             # the argument check comes first: it needs no device net
        check(self.lib.y3_net_set_pools_i8(self._h, on), "y3_net_set_pools_i8")
        self.__dict__["_pools_i8_on"] = on

    @property
    def pools_i8(self) -> int:
        """1 when the plan in force runs at least one aux op in int8 (y3_net_pools_i8), 0 otherwise, also before plan()."""
        return int(self.lib.y3_net_pools_i8(self._h))


class Net(_TinyStemSwitch, _PoolsI8Switch):
    """Device-side network = the fused conv program (reference counterpart: the Keras Model returned by
    ParseModel.build_model, core/parse_model.py:279-314)."""

    def __init__(self, program: Program):
        _lib.require_gpu()
        self.program = program
        self.lib = _lib.load()
        p = program
        # the device holds the stored widths (graph.Program.stored: padded where a narrow conv output feeds a conv); read_tensor,
        # flops_per_image and the weight dictionary stay at the real ones
        self._stored = list(p.stored) if p.stored else [t.channels for t in p.tensors]
        tens = (TensorDesc * len(p.tensors))(*[TensorDesc(c, t.div) for c, t in zip(self._stored, p.tensors)])
        kinds, convs, auxs = [], [], []
        self.conv_ops: List[ConvOp] = []
        for o in p.ops:
            if isinstance(o, ConvOp):
                kinds.append(0)
                convs.append(ConvDesc(o.size, o.stride, o.cin, o.cout, int(o.bn), int(o.leaky), o.src0,
                                      int(o.src0_upsample), o.c0, o.src1, o.residual, o.dst, o.in_div, o.out_div))
                self.conv_ops.append(o)
            elif isinstance(o, AuxOp):
                kinds.append(1)
                auxs.append(AuxDesc(_AUX_KIND[o.kind], o.inputs[0], o.inputs[1] if len(o.inputs) > 1 else -1, o.dst))
        if len(p.outputs) not in (2, 3):
            raise Y3Error(f"the HIP path runs nets of two or three detection heads (this program has {len(p.outputs)})")
        self.heads = len(p.outputs)
        self._h = C.c_void_p()
        k_arr = (C.c_int32 * len(kinds))(*kinds)
        c_arr = (ConvDesc * max(1, len(convs)))(*convs)
        a_arr = (AuxDesc * max(1, len(auxs)))(*auxs)
        outs = (C.c_int32 * self.heads)(*p.outputs)
        if self.heads == 3 and getattr(self.lib.y3_net_create_heads, "missing", False):      # an older build under Y3_LIB_PATH: three heads only
            st = self.lib.y3_net_create(tens, len(p.tensors), k_arr, len(kinds), c_arr, len(convs), a_arr, len(auxs), p.input_tensor, outs,
                                        p.nclasses, C.byref(self._h))
        else:
            st = self.lib.y3_net_create_heads(tens, len(p.tensors), k_arr, len(kinds), c_arr, len(convs), a_arr, len(auxs), p.input_tensor,
                                              outs, self.heads, p.nclasses, C.byref(self._h))
        check(st, "y3_net_create")
        self.image_size = 0
        self._tiles, self._merge_iou_threshold = None, None      # the properties tiles / merge_iou_threshold
        self.canvas = (0, 0)     # the planned (H, W); image_size is the int S for a plan made with an int
        self.max_batch = 0
        self.dtype = _lib.Y3_DTYPE_F32
        self.weights_loaded = False

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self.lib.y3_net_destroy(h)
            self._h = None      # (module globals may already be gone at interpreter shutdown)

    # -- weights ----------------------------------------------------------------------------------
    def load_weights(self, weights: Dict[str, np.ndarray], eps: float = BN_EPS):
        """weights: the dictionary at the real widths of the program's nodes; where the lowering pads channels the upload is padded
        (weights.pad_weights: zero rows and filters, BN statistics that make the pad channels exact zeros)."""
        p = self.program
        real = {n.conv_index: (n.size, n.size, p.tensors[n.inputs[0]].channels, n.filters) for n in p.conv_nodes}
        for o in self.conv_ops:
            shape = np.shape(weights[f"conv{o.conv_index}.w"])
            if tuple(shape) != real[o.conv_index]:
                raise Y3Error(f"conv{o.conv_index}.w has shape {tuple(shape)}, expected {real[o.conv_index]}")
        if self._stored != [t.channels for t in p.tensors]:
            weights = pad_weights(p, weights)
        for slot, o in enumerate(self.conv_ops):
            i = o.conv_index
            w = np.ascontiguousarray(weights[f"conv{i}.w"], np.float32)
            if w.shape != (o.size, o.size, o.cin, o.cout):
                raise Y3Error(f"conv{i}.w has shape {w.shape}, expected {(o.size, o.size, o.cin, o.cout)}")
            get = lambda k: np.ascontiguousarray(weights[f"conv{i}.{k}"], np.float32)
            if o.bn:
                g, b, m, v = get("gamma"), get("beta"), get("mean"), get("var")
                st = self.lib.y3_net_set_conv_weights(self._h, slot, _fptr(w), _fptr(g), _fptr(b), _fptr(m), _fptr(v),
                                                      None, eps)
            else:
                bias = get("bias")
                st = self.lib.y3_net_set_conv_weights(self._h, slot, _fptr(w), None, None, None, None, _fptr(bias), eps)
            check(st, f"y3_net_set_conv_weights(conv{i})")
        self.weights_loaded = True

    # -- planning / execution ---------------------------------------------------------------------
    def keep_activations(self, keep=True):
        """No buffer reuse in the plans made from now on, so that read_tensor reads any stored tensor after a forward.  On a planned net
        it waits for the next plan() (include/y3.h, "Setters on a planned net")."""
        check(self.lib.y3_net_keep_activations(self._h, int(keep)), "y3_net_keep_activations")

    def set_lanes(self, lanes: int):
        """Concurrent sub-batches of a forward, 1..4; acts at once on a planned net.  plan() sets it from the plan's tuning table (1
        without one): call it after plan()."""
        check(self.lib.y3_net_set_lanes(self._h, int(lanes)), "y3_net_set_lanes")
        self.lanes = int(lanes)

    def set_xcd_mode(self, mode: int):
        """fp32 conv tile placement on the 8 XCDs: 1 = XCD-blocked order chosen per conv (default), 0 = contiguous runs.  Read by every
        forward: acts at once on a planned net and survives plan()."""
        check(self.lib.y3_net_set_xcd_mode(self._h, int(mode)), "y3_net_set_xcd_mode")

    def set_k_chunk(self, channels: int):
        """K order of the fp32 3x3 convs: channels per chunk (multiple of 32) walked chunk-major, 0 tap-major, -1 default.  Read by every forward:
        acts at once on a planned net and survives plan()."""
        check(self.lib.y3_net_set_k_chunk(self._h, int(channels)), "y3_net_set_k_chunk")

    def set_border_skip(self, mode: int):
        """fp32 3x3 convs on batch-minor rows that skip their padding taps (bit-identical): -1 the library's rule, 0 off, 1 on wherever legal.
        Read by every forward: acts at once on a planned net and survives plan()."""
        check(self.lib.y3_net_set_border_skip(self._h, int(mode)), "y3_net_set_border_skip")

    def border_skip(self, slot: int, batch: int) -> int:
        """In how many of its sub-batches a forward of `batch` images launches conv `slot` of the planned net with the border skip."""
        return int(self.lib.y3_net_get_border_skip(self._h, int(slot), int(batch)))

    @property
    def nms_per_class(self) -> bool:
        """Which NMS rule detect, detect_stream and evaluate_stream run (y3_net_set_nms_mode): False (the default), the reference's
        class-agnostic rule; True, a box is suppressed only by a kept box of its own class (ops.nms_padded_per_class; needs
        iou_threshold > 0).  Read whenever a detect is enqueued: a captured graph keeps the rule it was captured with."""
        return self.lib.y3_net_get_nms_mode(self._h) == _lib.Y3_NMS_PER_CLASS

    @nms_per_class.setter
    def nms_per_class(self, on):
        if not isinstance(on, (bool, np.bool_)):
            raise TypeError(f"nms_per_class: a bool (got {on!r})")
        check(self.lib.y3_net_set_nms_mode(self._h, _lib.Y3_NMS_PER_CLASS if on else _lib.Y3_NMS_AGNOSTIC), "y3_net_set_nms_mode")

    @property
    def multi_label(self) -> bool:
        """Multi-label detections in detect, detect_stream and evaluate_stream (y3_net_set_multi_label; no reference counterpart): False
        (the default), every box carries its arg-max class; True, every pair (box, class) with conf * prob above the score threshold is
        a detection of its own and the NMS of the net's mode decides between them (multilabel.py restates the rule; `multi_label_capacity`
        and `multi_label_totals` beside it).  A row then reads {box of n, conf[n] * prob[n,c], c, n} and two rows of an image may share n.
        Read whenever a detect is enqueued: a captured graph keeps what it was captured with."""
        get = self.lib.y3_net_get_multi_label
        return False if getattr(get, "missing", False) else bool(get(self._h))      # an older build under Y3_LIB_PATH has no such route: off

    @multi_label.setter
    def multi_label(self, on):
        if not isinstance(on, (bool, np.bool_)):
            raise TypeError(f"multi_label: a bool (got {on!r})")
        check(self.lib.y3_net_set_multi_label(self._h, int(on), self.multi_label_capacity), "y3_net_set_multi_label")

    @property
    def multi_label_capacity(self) -> int:
        """Candidate slots per image of the multi-label route: 0 (the default), N of the plan; otherwise 1 <= capacity <= N, checked
        when a detect is enqueued.  An image with more candidates keeps the first `capacity` in (box, class) order; multi_label_totals
        tells."""
        return int(self.lib.y3_net_get_multi_label_capacity(self._h))

    @multi_label_capacity.setter
    def multi_label_capacity(self, capacity):
        if isinstance(capacity, (bool, np.bool_)) or not isinstance(capacity, (int, np.integer)):
            raise TypeError(f"multi_label_capacity: an int (got {capacity!r})")
        check(self.lib.y3_net_set_multi_label(self._h, int(self.multi_label), int(capacity)), "y3_net_set_multi_label")

    @property
    def multi_label_totals(self) -> torch.Tensor:
        """[max_batch] int32 on the GPU: the candidates of every image of the last multi-label detect enqueued on this plan, uncapped
        (0 for images it did not have); total > capacity says the image was truncated.  Enqueues a copy on the current stream."""
        totals = torch.empty((max(self.max_batch, 1),), dtype=torch.int32, device="cuda")
        check(self.lib.y3_net_read_multi_label_totals(self._h, totals.shape[0], _dev(totals), _lib.stream_ptr()),
              "y3_net_read_multi_label_totals")
        return totals

    @property
    def tiles(self):
        """Sliced inference in detect_stream / evaluate_stream: None (off, the default) or (rows, cols, overlap_px, overview) -- every frame
        is cut into rows x cols windows overlapping by at least overlap_px pixels (y3_tile_grid), plus the whole frame with overview; each
        window runs through the network as an image of its own and y3_merge_tile_detections merges the windows' detections per frame.
        Read when a stream starts.  No reference counterpart."""
        return self._tiles

    @tiles.setter
    def tiles(self, tiles):
        from .input_stage import tiles_arg
        self._tiles = None if tiles is None else tiles_arg("Net.tiles", tiles)[0]

    @property
    def merge_iou_threshold(self):
        """The IoU threshold of the merge NMS of sliced inference; None (the default): the stream's iou_threshold."""
        return self._merge_iou_threshold

    @merge_iou_threshold.setter
    def merge_iou_threshold(self, t):
        if t is not None and not isinstance(t, (int, float, np.floating)):
            raise TypeError(f"merge_iou_threshold: a number or None (got {t!r})")
        self._merge_iou_threshold = None if t is None else float(t)

    @staticmethod
    def _dtype_arg(dtype) -> int:
        """None (absent: fp32), a _lib.Y3_DTYPE_* value or its tag ("f32", "bf16", "f16", "f32x3", "f32x2") -> the Y3_DTYPE_* value."""
        if dtype is None:
            return _lib.Y3_DTYPE_F32
        if isinstance(dtype, str) and dtype in _lib.DTYPE_TAGS.values():
            return next(k for k, v in _lib.DTYPE_TAGS.items() if v == dtype)
        if not isinstance(dtype, (bool, np.bool_)) and isinstance(dtype, (int, np.integer)) and int(dtype) in _lib.DTYPE_TAGS:
            return int(dtype)
        raise Y3Error(f"dtype must be None or one of {sorted(_lib.DTYPE_TAGS.values())} (got {dtype!r})")

    def set_dtype(self, dtype):
        """The conv arithmetic of the plans this net makes for itself from now on (forward / detect re-plan when the batch
        shape changes; plan() without a dtype): None or "f32", "bf16", "f16", "f32x3", "f32x2", "i8" (needs the activation scales:
        calibrate_i8 / load_calibration / set_act_scales), or a _lib.Y3_DTYPE_* value.
        A net already planned in another dtype is planned again, same batch and canvas.  When that plan is refused the call raises and
        the dtype stays what it was: the old plan is intact, or gone (max_batch 0) and the next forward plans in the old dtype (plan())."""
        dtype = self._dtype_arg(dtype)
        if self.max_batch and dtype != self.dtype:
            self.plan(self.max_batch, self.image_size, dtype)
        self.dtype = dtype

    @staticmethod
    def _low_latency_arg(on) -> bool:
        if on is None:
            return False
        if isinstance(on, (bool, np.bool_)) or (isinstance(on, (int, np.integer)) and int(on) in (0, 1)):
            return bool(on)
        raise Y3Error(f"low_latency must be None, a bool, 0 or 1 (got {on!r})")

    @staticmethod
    def _split_k_arg(S) -> int:
        if isinstance(S, (bool, np.bool_)) or not isinstance(S, (int, np.integer)) or not (int(S) in (-1, 1) or 2 <= int(S) <= 16):
            raise Y3Error(f"split_k must be -1 (heuristic), 1 (off) or an int in 2..16 (got {S!r})")
        return int(S)

    def _slot_arg(self, who: str, slot) -> int:
        if isinstance(slot, (bool, np.bool_)) or not isinstance(slot, (int, np.integer)) or not 0 <= int(slot) < len(self.conv_ops):
            raise Y3Error(f"{who}: conv slot must be an int in [0, {len(self.conv_ops)}) (got {slot!r})")
        return int(slot)

    def _set_low_latency(self, sfx: str, on):   # sfx, here and below: "" the fp32 plans' entry points, "_bf16" the bf16 plans', "_f16" the fp16 plans', "_i8" the int8 plans'
        on = int(self._low_latency_arg(on))     # the argument checks come first: they need no device net
        check(getattr(self.lib, "y3_net_set_low_latency" + sfx)(self._h, on), "y3_net_set_low_latency" + sfx)

    def _set_split_k(self, sfx: str, slot, S):
        S, slot = self._split_k_arg(S), self._slot_arg("set_split_k" + sfx, slot)
        check(getattr(self.lib, "y3_net_set_split_k" + sfx)(self._h, slot, S), "y3_net_set_split_k" + sfx)

    def _split_k(self, sfx: str, slot) -> int:
        slot = self._slot_arg("split_k" + sfx, slot)
        return int(getattr(self.lib, "y3_net_get_split_k" + sfx)(self._h, slot))

    def set_low_latency(self, on=True):
        """Low-latency fp32 plan for one to eight images (y3_net_set_low_latency), before plan(): each eligible conv is cut
        along K into the number of slices y3_choose_split_k gives for the planned batch, summed in a fixed order by a second
        launch.  Off by default; results differ from the default plan's in the last bits.  None means off.  This switch and the _bf16 / _f16 /
        _i8 ones, like the set_split_k* requests, act at once on a planned net of their mode and survive plan(), also a plan in another
        mode, where they rest."""
        self._set_low_latency("", on)

    def set_split_k(self, slot: int, S: int):
        """K slices of conv `slot`: -1 the heuristic (in force only with set_low_latency), 1 off, 2..16 forced.  An
        ineligible conv (first layer, fused stem, tile 33, a detection head, a plan that is not fp32) or S above the conv's K
        tiles raises here."""
        self._set_split_k("", slot, S)

    def split_k(self, slot: int) -> int:
        """K slices in force for conv `slot` after plan() (1: the ordinary launch)."""
        return self._split_k("", slot)

    def set_low_latency_bf16(self, on=True):
        """Low-latency bf16 plan for one to eight images (y3_net_set_low_latency_bf16): as set_low_latency, for a plan made with
        Y3_DTYPE_BF16.  The two switches are independent; each acts on plans of its own dtype only.  None means off."""
        self._set_low_latency("_bf16", on)

    def set_split_k_bf16(self, slot: int, S: int):
        """K slices of conv `slot` in a bf16 plan: -1 the heuristic (in force only with set_low_latency_bf16), 1 off, 2..16 forced.
        An ineligible conv (first layer, fused stem, tile 32, a BK = 32 tile, a tile other than 11 / 12, a detection head, a plan that
        is not bf16) or S above the conv's K tiles (K / 64) raises here."""
        self._set_split_k("_bf16", slot, S)

    def split_k_bf16(self, slot: int) -> int:
        """K slices in force for conv `slot` in a bf16 plan after plan() (1: the ordinary launch; 1 on every other plan)."""
        return self._split_k("_bf16", slot)

    def set_low_latency_f16(self, on=True):
        """Low-latency fp16 plan for one to eight images (y3_net_set_low_latency_f16): as set_low_latency_bf16, for a plan made with
        Y3_DTYPE_F16.  The three switches are independent; each acts on plans of its own dtype only.  None means off."""
        self._set_low_latency("_f16", on)

    def set_split_k_f16(self, slot: int, S: int):
        """K slices of conv `slot` in an fp16 plan: -1 the heuristic (in force only with set_low_latency_f16), 1 off, 2..16 forced.
        Refused as set_split_k_bf16 refuses, with "a plan that is not fp16" for "a plan that is not bf16"."""
        self._set_split_k("_f16", slot, S)

    def split_k_f16(self, slot: int) -> int:
        """K slices in force for conv `slot` in an fp16 plan after plan() (1: the ordinary launch; 1 on every other plan)."""
        return self._split_k("_f16", slot)

    def set_low_latency_i8(self, on=True):
        """Low-latency int8 plan for one to eight images (y3_net_set_low_latency_i8): as set_low_latency_f16, for a plan made with
        Y3_DTYPE_I8.  It acts on the int8 convs (from i8_first_conv() on); the fp16 convs before the cut stay unsplit.  The slices hold
        i32 sums, so the results are the default int8 plan's bit for bit.  The four switches are independent.  None means off."""
        self._set_low_latency("_i8", on)

    def set_split_k_i8(self, slot: int, S: int):
        """K slices of conv `slot` in an int8 plan: -1 the heuristic (in force only with set_low_latency_i8), 1 off, 2..16 forced.
        An ineligible conv (first layer, a detection head, a tile other than 11 / 12, a conv before the cut of a planned int8 net, a
        plan that is not int8) or S above the conv's K tiles (K / 128) raises here."""
        self._set_split_k("_i8", slot, S)

    def split_k_i8(self, slot: int) -> int:
        """K slices in force for conv `slot` in an int8 plan after plan() (1: the ordinary launch; 1 on every other plan)."""
        return self._split_k("_i8", slot)

    @staticmethod
    def _stem_fusion_arg(on) -> int:
        if on is None:
            return 0
        if isinstance(on, (bool, np.bool_, int, np.integer)) and int(on) in (0, 1, 2):
            return int(on)
        raise Y3Error(f"stem fusion must be None, a bool, 0, 1 or 2 (got {on!r})")

    def set_stem_fusion(self, on):
        """conv0 + conv1 (+ the 1x1 conv that follows them) as one kernel (default on; applies when the program starts with
        the Darknet-53 stem and the plan is fp32 or bf16 without keep_activations).  2: conv0 + conv1 only.  Acts at once on a planned
        fp32 or bf16 net; survives plan()."""
        check(self.lib.y3_net_set_stem_fusion(self._h, int(on)), "y3_net_set_stem_fusion")

    def set_stem_fusion_f16(self, on=True):
        """The same switch for fp16 plans, and for them only (y3_net_set_stem_fusion_f16): off by default; True / 1, 2 as
        set_stem_fusion; None means off.  Pixel values must be finite and at most 65504 in magnitude.  Acts at once on a planned fp16 or
        int8 net; survives plan()."""
        on = self._stem_fusion_arg(on)          # the argument check comes first: it needs no device net
        check(self.lib.y3_net_set_stem_fusion_f16(self._h, on), "y3_net_set_stem_fusion_f16")

    def set_early_chunk(self, n_convs: int, chunk_images: int):
        """Before plan(): the first n_convs convs run chunk_images images at a time (their activations then stay in the
        Infinity Cache between producer and consumer); 0, 0 switches it off.  On a planned net it waits for the next plan(): the plan in
        force keeps the segment and the chunk size it was made with."""
        check(self.lib.y3_net_set_early_chunk(self._h, int(n_convs), int(chunk_images)), "y3_net_set_early_chunk")

    # A tile forced through these setters acts at once on a planned net and survives plan(): the tuning table only fills the convs left
    # on automatic (tile -1 hands the conv back to the library's heuristic at once, and to the table at the next plan()).
    def _set_tile(self, kind: str, slot: int, tile: int):     # kind: a suffix of _TILE_KIND
        check(getattr(self.lib, "y3_net_set_tile" + kind)(self._h, slot, tile), f"y3_net_set_tile{kind}")

    def _force(self, kind: str, slot: int, tile: int):
        self._set_tile(kind, slot, tile)
        forced = self.__dict__.setdefault("_forced_tiles", {})
        if tile >= 0:
            forced[(kind, slot)] = tile
        else:
            forced.pop((kind, slot), None)

    def set_tile(self, slot: int, tile: int):
        self._force("", slot, tile)

    def set_tile_x3(self, slot: int, tile: int):
        self._force("_x3", slot, tile)

    def set_tile_x2(self, slot: int, tile: int):
        self._force("_x2", slot, tile)

    def set_tile_bf16(self, slot: int, tile: int):
        """Force a tile of the 16-bit conv family on conv `slot`: acts on bf16 and fp16 plans alike (one tile table, one field)."""
        self._force("_bf16", slot, tile)

    def plan(self, max_batch: int, image_size, dtype: Optional[int] = None):
        """image_size: an int S (the S x S canvas) or an (H, W) pair, both sides multiples of 32 (y3_net_plan_hw).
        dtype: _lib.Y3_DTYPE_F32 (default, fp32 MFMA), _lib.Y3_DTYPE_F32X3 (fp32-accurate on the bf16 matrix cores:
        three bf16 planes per value), _lib.Y3_DTYPE_F32X2 (two fp16 planes per value, 2^-22 representation, |x| < 65504)
        _lib.Y3_DTYPE_BF16 (bf16 activations/weights, fp32 accumulate) or _lib.Y3_DTYPE_F16 (the same with IEEE fp16: 8 x closer to
        fp32, values beyond 65504 become inf; the fused stem and split-K only through set_stem_fusion_f16 / set_low_latency_f16).
        A refused plan raises and leaves either the old plan intact, with these fields unchanged, or no plan at all: max_batch 0 and
        canvas (0, 0), and the next forward / detect plans by itself (include/y3.h names which refusal leaves which).  Every set_*
        survives a plan; lanes alone are set again by each plan, from its tuning table."""
        if dtype is None:
            dtype = self.dtype
        H, W = canvas_hw(image_size)
        try:
            check(self.lib.y3_net_plan_hw(self._h, max_batch, H, W, dtype), "y3_net_plan")
        except Y3Error:
            self._forget_plan_if_gone()
            raise
        self.max_batch, self.dtype, self.canvas = max_batch, dtype, (H, W)
        # the form grid_sizes() answers in -- g for an int plan, (gh, gw) for a pair plan -- is that of the last plan() a caller made
        self.image_size = int(image_size) if isinstance(image_size, (int, np.integer)) else (H, W)
        self._apply_tuning()

    def _forget_plan_if_gone(self):
        """After a refused plan(): the library either kept the old plan, and so do max_batch / canvas / image_size / dtype, or freed it
        (include/y3.h, the table at y3_net_plan_hw; y3_net_get_plan tells) -- then max_batch = 0 and canvas = (0, 0) as before the first
        plan, image_size keeps only its form (0 or (0, 0): _plan_for's rule), dtype stays what it was before the call, and the next
        forward / detect plans by itself in that dtype."""
        get = self.lib.y3_net_get_plan
        if getattr(get, "missing", False) or get(self._h, None, None, None, None):
            return
        self.max_batch, self.canvas = 0, (0, 0)
        self.image_size = (0, 0) if isinstance(self.image_size, tuple) else 0

    @staticmethod
    def conv_signature(o: ConvOp, image_size) -> str:
        ho = max(canvas_hw(image_size)) // o.out_div
        return f"k{o.size}s{o.stride}_c{o.cin}_n{o.cout}_h{ho}_r{int(o.residual >= 0)}_u{int(o.src1 >= 0)}"

    def _apply_tuning(self):
        """Per-conv tile ids measured by tools/tune_tiles.py for this (dtype, batch, image size), if a table exists;
        otherwise the library's heuristic stays in force.  An fp16 plan takes the bf16 table of its batch and size, lanes included,
        through set_tile_bf16 (same kernels, same tile ids; no fp16 table is tuned or shipped)."""
        import json
        import os
        sixteen = self.dtype in (_lib.Y3_DTYPE_F16, _lib.Y3_DTYPE_I8)
        tag = _lib.DTYPE_TAGS[_lib.Y3_DTYPE_BF16 if sixteen else self.dtype]
        path = tuning_table_path(tag, self.max_batch, self.image_size)
        kind = _TILE_KIND[self.dtype]
        # an int8 plan: the convs before its cut run as an fp16 plan's and take the bf16 table like one (lanes included); the int8 convs
        # are left to the library's heuristic (no int8 table is tuned or shipped)
        i8_from = self.i8_first_conv() if self.dtype == _lib.Y3_DTYPE_I8 else len(self.conv_ops)
        forced = self.__dict__.get("_forced_tiles", {})
        table, lanes = {}, 1
        if os.path.exists(path) and not os.environ.get("Y3_NO_TUNING"):
            with open(path) as f:
                doc = json.load(f)
            table, lanes = doc.get("tiles", {}), int(doc.get("lanes", 1))
        # concurrent sub-batches (tools/lanes_sweep.py): the tail of one sub-batch's kernel overlaps another's bulk
        self.set_lanes(lanes)
        for slot, o in enumerate(self.conv_ops):
            if o.cin == 3 or (kind, slot) in forced:
                continue
            tile = int(table.get(self.conv_signature(o, self.image_size), -1)) if slot < i8_from else -1
            self._set_tile(kind, slot, tile)

    def grid_sizes(self, image_size=None):
        """Per head: g for an int image size, (gh, gw) for an (H, W) pair (default: what the net was planned with)."""
        return self.program.grid_sizes(image_size or (self.image_size if self.max_batch else 0))

    def _grid_hw(self):
        return [(self.canvas[0] // self.program.tensors[o].div, self.canvas[1] // self.program.tensors[o].div)
                for o in self.program.outputs]

    def _plan_for(self, images: torch.Tensor):
        """Re-plan when the batch's [B,H,W,..] does not match the plan.  The plan keeps the form the caller last gave it: a net
        planned with a pair stays a pair plan (grid_sizes() keeps returning pairs) also for an H == W batch; a net planned with
        an int, or never planned, takes a square batch as an int plan."""
        B, H, W = images.shape[0], images.shape[1], images.shape[2]
        if (H, W) != self.canvas or B > self.max_batch:
            pair = H != W or isinstance(self.image_size, tuple)
            self.plan(max(B, self.max_batch), (H, W) if pair else H)
        return B

    def forward(self, images: torch.Tensor, out: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
        """images [B,H,W,3] fp32 on the GPU -> the head grids, coarsest first (three, or two for a two-head net), each [B,gh,gw,3,5+nc]."""
        _need_cuda(images)
        cin = self.program.tensors[self.program.input_tensor].channels
        # bf16 / fp16 plan + an input that feeds an MFMA conv directly (layer tests): the input is bf16 / fp16 as well
        if self.dtype == _lib.Y3_DTYPE_F32X3 and cin != 3:
            # layer tests: an input feeding an MFMA conv directly is handed over as three bf16 planes [B,S,S,3,C]
            if images.dtype != torch.bfloat16 or images.dim() != 5 or images.shape[3] != 3 or images.shape[4] != cin:
                raise Y3Error(f"images must be bfloat16 [B,S,S,3,{cin}] (split3_planes) in the three-plane mode")
        elif self.dtype == _lib.Y3_DTYPE_F32X2 and cin != 3:
            if images.dtype != torch.float16 or images.dim() != 5 or images.shape[3] != 2 or images.shape[4] != cin:
                raise Y3Error(f"images must be float16 [B,S,S,2,{cin}] (split2_planes) in the two-plane mode")
        else:
            want = torch.float32 if cin == 3 else {_lib.Y3_DTYPE_BF16: torch.bfloat16, _lib.Y3_DTYPE_F16: torch.float16,
                                                   _lib.Y3_DTYPE_I8: torch.float16}.get(self.dtype, torch.float32)
            if images.dtype != want or images.dim() != 4 or images.shape[3] != cin:
                raise Y3Error(f"images must be {want} [B,S,S,{cin}]")
        B = self._plan_for(images)
        nc = self.program.nclasses
        gs = self._grid_hw()
        if out is None:
            if nc > 0:
                out = [torch.empty((B, gh, gw, 3, 5 + nc), dtype=torch.float32, device=images.device) for gh, gw in gs]
            else:  # raw feature outputs (layer tests)
                out = [torch.empty((B, gh, gw, self.program.tensors[o].channels), dtype=torch.float32,
                                   device=images.device) for (gh, gw), o in zip(gs, self.program.outputs)]
        _need_cuda(*out)
        ptrs = self._grid_ptrs(out)
        check(self.lib.y3_net_forward(self._h, _dev(images), B, ptrs, _lib.stream_ptr()), "y3_net_forward")
        return list(out)

    __call__ = forward

    def _grid_ptrs(self, out):
        if len(out) != self.heads:
            raise Y3Error(f"expected {self.heads} head grids (got {len(out)})")
        return (C.c_void_p * self.heads)(*[t.data_ptr() for t in out])

    def measure_sclk(self, images: torch.Tensor, out: Sequence[torch.Tensor], forwards: int = 30, conv: int = -1) -> float:
        """Shader clock (MHz) the chip holds under this network's load: `forwards` forwards back to back, in the last one
        a conv launch stamps s_memtime / s_memrealtime (y3_net_measure_sclk: the conv with the most FLOPs; conv >= 0:
        that conv slot, y3_net_measure_sclk_conv).  Raises when no launch of the plan / not that launch carries stamps."""
        _need_cuda(images, *out)
        ptrs = self._grid_ptrs(out)
        mhz = C.c_float()
        if conv >= 0:
            check(self.lib.y3_net_measure_sclk_conv(self._h, _dev(images), images.shape[0], ptrs, int(forwards), int(conv),
                                                    C.byref(mhz), _lib.stream_ptr()), "y3_net_measure_sclk_conv")
        else:
            check(self.lib.y3_net_measure_sclk(self._h, _dev(images), images.shape[0], ptrs, int(forwards), C.byref(mhz),
                                               _lib.stream_ptr()), "y3_net_measure_sclk")
        return float(mhz.value)

    def measure_sclk_all(self, images: torch.Tensor, out: Sequence[torch.Tensor], forwards: int = 30):
        """Per conv slot: (MHz, start_us, end_us) of the stamped workgroup of its launch in the last of `forwards`
        back-to-back forwards (y3_net_measure_sclk_all); MHz 0 where a conv leaves no stamps.  numpy arrays."""
        _need_cuda(images, *out)
        ptrs = self._grid_ptrs(out)
        n = len(self.conv_ops)
        mhz = (C.c_float * n)()
        t0 = (C.c_double * n)()
        t1 = (C.c_double * n)()
        check(self.lib.y3_net_measure_sclk_all(self._h, _dev(images), images.shape[0], ptrs, int(forwards), mhz, t0, t1,
                                               _lib.stream_ptr()), "y3_net_measure_sclk_all")
        return np.array(mhz[:], dtype=np.float64), np.array(t0[:]), np.array(t1[:])

    def _read_tensor(self, sfx: str, dtype, tensor_id: int, batch: int, stored=False) -> torch.Tensor:
        fn, what = getattr(self.lib, "y3_net_read_tensor" + sfx), "y3_net_read_tensor" + sfx
        n = C.c_size_t()
        check(fn(self._h, tensor_id, batch, None, C.byref(n), None), what)
        t = self.program.tensors[tensor_id]
        out = torch.empty((batch, self.canvas[0] // t.div, self.canvas[1] // t.div, self._stored[tensor_id]), dtype=dtype, device="cuda")
        assert out.numel() == n.value
        check(fn(self._h, tensor_id, batch, _dev(out), C.byref(n), _lib.stream_ptr()), what)
        return out if stored or self._stored[tensor_id] == t.channels else out[..., :t.channels].contiguous()      # the real channels

    def read_tensor(self, tensor_id: int, batch: int) -> torch.Tensor:
        return self._read_tensor("", torch.float32, tensor_id, batch)

    # -- int8 plans (include/y3.h, "int8 plans"; the scheme restated in quant.py) ----------------------------------------------------
    def read_tensor_i8(self, tensor_id: int, batch: int) -> torch.Tensor:
        """The raw bytes of an int8 tensor of the last forward of an int8 plan: a tensor behind the cut, or the int8 copy of one that
        crosses it.  -> int8 [batch, h, w, C]."""
        return self._read_tensor("_i8", torch.int8, tensor_id, batch)

    def set_act_scales(self, scales):
        """One fp32 scale per tensor of the program (entries <= 0 or None: unset), read by the next plan() in "i8": a planned int8 net
        keeps the scales its plan took."""
        a = np.ascontiguousarray([0.0 if s is None else float(s) for s in scales], np.float32)
        check(self.lib.y3_net_set_act_scales(self._h, _fptr(a), int(a.size)), "y3_net_set_act_scales")

    def act_scales(self) -> List[float]:
        """The scales in force, one per tensor; 0.0 where unset."""
        return [float(self.lib.y3_net_get_act_scale(self._h, t)) for t in range(len(self.program.tensors))]

    def i8_first_conv(self) -> int:
        """c*: the first conv slot an int8 plan runs in int8 (-1 when the net is not planned in "i8")."""
        return int(self.lib.y3_net_i8_first_conv(self._h))

    def calibrate_i8(self, images: torch.Tensor, percentile: float = 100.0) -> List[float]:
        """Activation scales for int8 plans from one batch of images [B,H,W,3] fp32 on the GPU: runs the fp32 plan with every
        activation kept, takes per tensor the absmax of |x| (percentile=100) or the given percentile of |x|, divides by 127, gives the
        two sources of every concat conv the larger of their scales (with set_pools_i8: also measures the tensors the aux ops write, and
        gives every class of quant.scale_classes its largest scale), sets the scales (set_act_scales) and returns them.  Offline: the
        reductions are torch's.  The net is left planned in fp32 with activations kept; plan it again for inference."""
        from . import quant
        if not 0.0 < float(percentile) <= 100.0:
            raise Y3Error(f"calibrate_i8: percentile must be in (0, 100] (got {percentile!r})")
        _need_cuda(images)
        B = int(images.shape[0])
        self.keep_activations(True)
        self.plan(B, (int(images.shape[1]), int(images.shape[2])), _lib.Y3_DTYPE_F32)
        grids = self.forward(images)
        p = self.program
        scales = [0.0] * len(p.tensors)
        written = {o.dst for o in p.conv_ops()}
        if self.__dict__.get("_pools_i8_on"):   # set_pools_i8: the tensors the aux ops write carry scales of their own
            written |= {o.dst for o in p.ops if isinstance(o, AuxOp)}
            if self.tiny_stem_fused:            # ... but those the fused tiny stem keeps on chip: they lie before any cut
                written -= {p.ops[0].dst, p.ops[1].dst, p.ops[2].dst}
        if p.tensors[p.input_tensor].channels != 3:   # layer tests: the input feeds an MFMA conv directly and is quantised itself
            written.add(p.input_tensor)
        for t in sorted(written):
            x = images if t == p.input_tensor else grids[p.outputs.index(t)] if t in p.outputs else self.read_tensor(t, B)
            a = x.abs().flatten().float()
            if float(percentile) >= 100.0:
                m = float(a.max())
            else:   # the k-th smallest of |x| at the percentile (kthvalue: exact, no interpolation)
                k = min(a.numel(), max(1, int(np.ceil(a.numel() * float(percentile) / 100.0))))
                m = float(a.kthvalue(k).values)
            scales[t] = quant.scale_from_absmax(m)
        torch.cuda.synchronize()
        scales = quant.equalize_concat(p, scales, classes=bool(self.__dict__.get("_pools_i8_on")))
        self.set_act_scales(scales)
        self.keep_activations(False)
        return scales

    def save_calibration(self, path: str):
        """The scales in force as JSON (tensor id -> scale) with the program's conv signature."""
        from . import quant
        quant.save_calibration(path, self.program, self.act_scales())

    def load_calibration(self, path: str):
        """Set the scales of a file save_calibration wrote; a table made for another graph is refused (Y3Error)."""
        from . import quant
        try:
            scales = quant.load_calibration(path, self.program)
        except ValueError as e:
            raise Y3Error(str(e)) from None
        self.set_act_scales(scales)
        return scales

    def forward_decode(self, images: torch.Tensor, anchors):
        """images -> (bboxes [B,N,4], class_indices [B,N] int64, scores [B,N]): the conv program with the head convs decoding
        their own tiles (y3_net_forward_decode; reference: model(inputs) -> yolo_decode -> argmax / score).  Same bits as
        forward() + yolo_decode_scores()."""
        _images_arg(images)
        B = self._plan_for(images)
        a = _anchors(anchors, reshape=True, scales=self.heads)
        n = sum(3 * gh * gw for gh, gw in self._grid_hw())
        bboxes = torch.empty((B, n, 4), dtype=torch.float32, device=images.device)
        cls = torch.empty((B, n), dtype=torch.int64, device=images.device)
        scores = torch.empty((B, n), dtype=torch.float32, device=images.device)
        check(self.lib.y3_net_forward_decode(self._h, _dev(images), B, _fptr(a), _dev(bboxes), _dev(cls), _dev(scores),
                                             _lib.stream_ptr()), "y3_net_forward_decode")
        return bboxes, cls, scores

    def detect(self, images: torch.Tensor, anchors, max_boxes: int, iou_threshold: float, score_threshold: float):
        """The whole path in one C call (y3_net_detect): -> (packed [B,max_boxes,7] int32 words, num_valid [B] int32);
        `unpack_detections` splits the rows."""
        _images_arg(images)
        B = self._plan_for(images)
        a = _anchors(anchors, reshape=True, scales=self.heads)
        packed = torch.empty((B, int(max_boxes), 7), dtype=torch.int32, device=images.device)
        nv = torch.empty((B,), dtype=torch.int32, device=images.device)
        check(self.lib.y3_net_detect(self._h, _dev(images), B, _fptr(a), int(max_boxes), float(iou_threshold),
                                     float(score_threshold), _dev(packed), _dev(nv), _lib.stream_ptr()), "y3_net_detect")
        return packed, nv

    def detect_stream(self, batches, anchors, max_boxes: int, iou_threshold: float, score_threshold: float, mode=1,
                      depth: int = 2, max_batch: Optional[int] = None, max_blob_bytes: Optional[int] = None, letterbox=False):
        """Frames in host memory -> detections, overlapped: a generator over an iterable of image lists (each image a
        NumPy [H,W,3|4] uint8 or float32 array; `mode` as for pack_images) that yields (packed [B,max_boxes,7] int32 words,
        num_valid [B] int32) as NumPy arrays, one pair per list, in submission order; a ragged last list is allowed.
        Batch i+1 is packed, copied and resized on the InputStage's copy stream before y3_net_detect of batch i is
        enqueued on the current stream, and only the packed rows come back to the host (pinned buffers, one event per
        batch): the host waits for the result of batch i while batch i+1 is already queued behind it.
        letterbox=True: the frames keep their aspect ratio (zero padding around them, core/utils.resize_image) and the
        boxes of the yielded rows are normalised to the frame that was handed in, not to the padded network input:
        y3_unletterbox_detections runs behind y3_net_detect on the same stream, before the read-back.
        The net keeps its planned image size -- an (H, W) plan letterboxes (or stretches) onto that canvas, and the yielded
        boxes are in source-frame coordinates all the same; the anchors are then the caller's rect_anchors -- and is re-planned at most once, for max_batch images; the stage's blobs hold
        max_blob_bytes.  Both default to the largest list of `batches`, which must then be a list or tuple.
        With the property `tiles` set to (rows, cols, overlap_px, overview): sliced inference for frames much larger than the canvas
        (a property like nms_per_class, so that the signature stays what it is; `merge_iou_threshold` beside it).  Every frame, uploaded
        once, is cut on the device into rows x cols overlapping windows (y3_tile_grid) plus, with overview, the whole frame; each
        window is stretched -- or with letterbox=True letterboxed -- onto the canvas as an image of its own
        (y3_preprocess_tiles_hw); y3_net_detect runs on the max_batch * T tile images the net is planned for; and
        y3_merge_tile_detections, in the place of y3_unletterbox_detections, maps the tiles' rows to the frame and runs the padded
        NMS over their union at merge_iou_threshold (default: iou_threshold), in the net's NMS mode.  The yielded rows are per
        FRAME, normalised to the frame, with the shapes described above; the index word of a row is t * max_boxes + r, its tile
        and its row there.  tiles = None, the default, enqueues exactly what it did before the property existed."""
        return stream.detect_stream(self, batches, anchors, max_boxes, iou_threshold, score_threshold, mode, depth, max_batch,
                                    max_blob_bytes, letterbox, self.tiles, self.merge_iou_threshold)

    def evaluate_stream(self, batches, gts, anchors, max_boxes: int, iou_threshold: float, score_thresholds, nclasses: int,
                        evaluate_iou_threshold: float = 0.5, one_class=False, mode=1, depth: int = 2,
                        max_batch: Optional[int] = None, max_blob_bytes: Optional[int] = None, letterbox=False,
                        max_gt: Optional[int] = None, loss=False, ap=None):
        """Frames in host memory -> the evaluation counters of EVERY NMS score threshold, from one detect pass: NumPy int64
        [T, 5*nclasses + 2] (rows as y3_evaluate_detections / evaluate_detections.counters_from_row name them), T =
        len(score_thresholds).  one_class=True: every class id taken as 0; one_class="both": the pair (plain counters,
        one-class counters) from the same pass.
        batches as for detect_stream (the same InputStage pipeline and the same loop); gts: per batch, a list of per-image
        (boxes [g,4], classes [g]) in normalised (xmin, ymin, xmax, ymax) -- with letterbox=True in the coordinates of the
        frame that was handed in, like the rows detect_stream yields.
        Per batch ONE y3_net_detect is enqueued, at min(score_thresholds): the detections of a higher threshold are its rows
        with score > threshold.  The ground truth goes up through a small pinned buffer per ring slot, y3_evaluate_detections
        accumulates into one device buffer, nothing is read back and the host waits for no result until the stream ends:
        then T x (5*nclasses + 2) integers (twice that for "both") come back in one copy.
        max_gt: the rows of ground truth the buffers hold per image.  By default the largest count of `gts`, which must then be
        a list or tuple; with max_gt given, `gts` may be any iterable and is consumed one entry per batch, in step with
        `batches` (a data set can then be streamed through without ever being held in memory).  The number of entries of `gts`
        must equal the number of batches either way.
        loss=True: the validation loss of reference core/loss_func.py from the same pass; the return value becomes (counters,
        {"sum": float64 [3,4], "images": int, "errors": int}).  "sum" holds, per scale, the sums xy, wh, obj, class over the
        "images" images that were counted; "errors" images were not (a class outside [0,nclasses), a box centred outside the
        image, a non-finite coordinate: they add nothing to "sum").  core.loss_func.summarize_loss turns it into val_loss,
        perGrid and perSource as reference train.py:45-52 forms them.  It is the validation loss only: no gradient is taken and
        the regulariser the reference's training loop adds (model.losses) is not part of it.  Each batch then takes y3_net_detect_grids, the composed
        route y3_net_forward -> y3_yolo_decode_scores -> y3_nms_padded -> y3_pack_detections as one call (bit-identical detections; the raw
        grids are written and read back, which y3_net_detect avoids), y3_yolo_assign_targets and y3_yolo_loss run on the same
        grids with the ground truth already on the device, and the sums come back with the counters in the one final copy.
        nclasses must be the program's.  Not together with letterbox=True: the reference trains on letterboxed images with
        unmapped boxes, and mapping the ground truth onto the canvas is a decision this method does not take.  Not on a
        non-square (H, W) plan either: y3_yolo_assign_targets / y3_yolo_loss take one g per scale.
        ap=True (or a sequence of 1 to 16 IoU thresholds; True means 0.5, 0.55, ..., 0.95): COCO-style average precision from
        the same pass; the return value gains a LAST element, the dict of evaluate_detections.average_precision ("ap" float64
        [K, nclasses], "map" [K], "mAP", "images", "errors").  Per batch ONE y3_match_detections is enqueued on the same
        stream behind y3_evaluate_detections, on the same packed rows (already in frame coordinates with letterbox=True) and
        the same ground-truth words; its records (8 bytes per packed row) stay on the device until the stream ends and come
        back with the counters, and the integral is taken on the host.  The rows of y3_net_detect at min(score_thresholds)
        are what is matched: pass a low score threshold for a meaningful AP.  one_class=True matches with every class taken
        as 0; with one_class="both" AP follows the plain variant.  AP has no reference counterpart: the matching rule (greedy
        in score order, a ground-truth box matched at most once per IoU threshold; no crowd flags, no area ranges, max_boxes
        as the per-image cap) is this project's statement of the COCO matching and is not checked against pycocotools.
        ap=None enqueues nothing new and returns exactly what is described above.
        With the properties `tiles` / `merge_iou_threshold` set: sliced inference as in detect_stream, in the same loop: the counters and the AP are taken on
        the merged per-frame rows, against ground truth in frame coordinates.  The one detect pass still serves every score
        threshold: both stages are greedy rules in which no box is affected by a lower-scored one, and the per-tile cap keeps a
        prefix, so the merged rows at a higher threshold are the rows with score > threshold of the merged rows at the lowest
        ("Sliced inference").  Not together with loss=True."""
        return stream.evaluate_stream(self, batches, gts, anchors, max_boxes, iou_threshold, score_thresholds, nclasses,
                                      evaluate_iou_threshold, one_class, mode, depth, max_batch, max_blob_bytes, letterbox,
                                      max_gt, loss, ap, self.tiles, self.merge_iou_threshold)

    def flops_per_image(self) -> float:
        """2 * MAC of the convs at the planned canvas, at the real channel counts (the device's own count, y3_net_flops_per_image,
        where nothing is padded)."""
        if self._stored != [t.channels for t in self.program.tensors]:
            return float(self.program.flops_per_image(self.canvas)) if self.canvas[0] else 0.0
        return float(self.lib.y3_net_flops_per_image(self._h))

    def profile_convs(self, images: torch.Tensor) -> np.ndarray:
        _need_cuda(images)
        ms = np.zeros(len(self.conv_ops), np.float32)
        check(self.lib.y3_net_profile_convs(self._h, _dev(images), images.shape[0], _fptr(ms), len(ms),
                                            _lib.stream_ptr()), "y3_net_profile_convs")
        return ms
