"""Thin host wrappers around the C ABI: torch tensors in, torch tensors out.

PyTorch is used for device memory and streams only; every arithmetic step below is a call into
liby3hip.so on the current torch stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import AuxDesc, ConvDesc, TensorDesc, Y3Error, check
from .graph import AuxOp, ConvOp, Program
from .weights import BN_EPS

_AUX_KIND = {"add": _lib.Y3_AUX_ADD, "upsample": _lib.Y3_AUX_UPSAMPLE2X, "concat": _lib.Y3_AUX_CONCAT}


def _fptr(a: Optional[np.ndarray]):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _dev(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _need_cuda(*ts):
    for t in ts:
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise Y3Error("expected contiguous CUDA(HIP) tensors; the y3 kernels have no CPU fallback")


def canvas_hw(image_size):
    """An image size as the (H, W) of the network canvas: an int S is the square (S, S), a pair is taken as (H, W)."""
    if isinstance(image_size, (int, np.integer)):
        return int(image_size), int(image_size)
    hw = tuple(int(v) for v in image_size)
    if len(hw) != 2:
        raise Y3Error(f"image_size must be an int or an (H, W) pair (got {image_size!r})")
    return hw


def _f32_geometry(h: int, w: int, Hc: int, Wc: int):
    """(sh, sw) of the letterbox geometry in the library's own fp32 arithmetic (include/y3.h, Y3_IMAGE_LETTERBOX;
    core/utils.letterbox_geometry is the same restatement with the offsets)."""
    scale = min(np.float32(Hc) / np.float32(h), np.float32(Wc) / np.float32(w))
    return max(1, int(np.rint(scale * np.float32(h)))), max(1, int(np.rint(scale * np.float32(w))))


def rect_canvas(height: int, width: int, image_size: int, stride: int = 32):
    """The smallest (H, W) canvas, both sides multiples of `stride`, that holds the aspect-preserving resize of a
    height x width frame whose long side becomes image_size -- the plan to letterbox such frames onto instead of the
    image_size^2 square, whose zero bars the conv stack would convolve.  (480, 640, 416) -> (320, 416).
    The resized extent is computed with the library's fp32 geometry; the canvas found is then checked with the same
    geometry (the frame letterboxed onto it must fit) and a side grows by one stride where rounding says otherwise."""
    h, w, S, st = int(height), int(width), int(image_size), int(stride)
    if h < 1 or w < 1 or S < 1 or st < 1:
        raise Y3Error("rect_canvas: height, width, image_size and stride must be at least 1")
    sh, sw = _f32_geometry(h, w, S, S)
    up = lambda v: -(-v // st) * st
    H, W = up(sh), up(sw)
    while True:
        gh, gw = _f32_geometry(h, w, H, W)
        if gh <= H and gw <= W:
            return H, W
        H, W = (H + st, W) if gh > H else (H, W + st)


def rect_anchors(anchors_table, image_size: int, canvas):
    """Anchors normalised by the square image_size (datasets/*/anchors.txt through core.utils.get_anchors) -> normalised
    by an (H, W) canvas: aw * S / W, ah * S / H, in fp32.  The anchor keeps its size in pixels.  An axis whose side equals
    image_size -- the long side of every rect_canvas -- is copied, not computed: x * S / S is not x in fp32."""
    H, W = canvas_hw(canvas)
    a = np.asarray(anchors_table, np.float32)
    out = a.copy()
    if W != int(image_size):
        out[..., 0] = a[..., 0] * np.float32(image_size) / np.float32(W)
    if H != int(image_size):
        out[..., 1] = a[..., 1] * np.float32(image_size) / np.float32(H)
    return out


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


class Net:
    """Device-side network = the fused conv program (reference counterpart: the Keras Model returned by
    ParseModel.build_model, core/parse_model.py:279-314)."""

    def __init__(self, program: Program):
        _lib.require_gpu()
        self.program = program
        self.lib = _lib.load()
        p = program
        tens = (TensorDesc * len(p.tensors))(*[TensorDesc(t.channels, t.div) for t in p.tensors])
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
        if len(p.outputs) != 3:
            raise Y3Error("the HIP path expects exactly three detection heads")
        self._h = C.c_void_p()
        k_arr = (C.c_int32 * len(kinds))(*kinds)
        c_arr = (ConvDesc * max(1, len(convs)))(*convs)
        a_arr = (AuxDesc * max(1, len(auxs)))(*auxs)
        outs = (C.c_int32 * 3)(*p.outputs)
        check(self.lib.y3_net_create(tens, len(p.tensors), k_arr, len(kinds), c_arr, len(convs), a_arr, len(auxs),
                                     p.input_tensor, outs, p.nclasses, C.byref(self._h)), "y3_net_create")
        self.image_size = 0
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
        check(self.lib.y3_net_keep_activations(self._h, int(keep)), "y3_net_keep_activations")

    def set_lanes(self, lanes: int):
        check(self.lib.y3_net_set_lanes(self._h, int(lanes)), "y3_net_set_lanes")
        self.lanes = int(lanes)

    def set_xcd_mode(self, mode: int):
        """fp32 conv tile placement on the 8 XCDs: 1 = XCD-blocked order chosen per conv (default), 0 = contiguous runs."""
        check(self.lib.y3_net_set_xcd_mode(self._h, int(mode)), "y3_net_set_xcd_mode")

    def set_k_chunk(self, channels: int):
        """K order of the fp32 3x3 convs: channels per chunk (multiple of 32) walked chunk-major, 0 tap-major, -1 default."""
        check(self.lib.y3_net_set_k_chunk(self._h, int(channels)), "y3_net_set_k_chunk")

    def set_border_skip(self, mode: int):
        """fp32 3x3 convs on batch-minor rows that skip their padding taps (bit-identical): -1 the library's rule, 0 off, 1 on wherever legal."""
        check(self.lib.y3_net_set_border_skip(self._h, int(mode)), "y3_net_set_border_skip")

    def border_skip(self, slot: int, batch: int) -> int:
        """In how many of its sub-batches a forward of `batch` images launches conv `slot` of the planned net with the border skip."""
        return int(self.lib.y3_net_get_border_skip(self._h, int(slot), int(batch)))

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
        A net already planned in another dtype is planned again, same batch and canvas."""
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
        launch.  Off by default; results differ from the default plan's in the last bits.  None means off."""
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
        the Darknet-53 stem and the plan is fp32 or bf16 without keep_activations).  2: conv0 + conv1 only."""
        check(self.lib.y3_net_set_stem_fusion(self._h, int(on)), "y3_net_set_stem_fusion")

    def set_stem_fusion_f16(self, on=True):
        """The same switch for fp16 plans, and for them only (y3_net_set_stem_fusion_f16): off by default; True / 1, 2 as
        set_stem_fusion; None means off.  Pixel values must be finite and at most 65504 in magnitude."""
        on = self._stem_fusion_arg(on)          # the argument check comes first: it needs no device net
        check(self.lib.y3_net_set_stem_fusion_f16(self._h, on), "y3_net_set_stem_fusion_f16")

    def set_early_chunk(self, n_convs: int, chunk_images: int):
        """Before plan(): the first n_convs convs run chunk_images images at a time (their activations then stay in the
        Infinity Cache between producer and consumer); 0, 0 switches it off."""
        check(self.lib.y3_net_set_early_chunk(self._h, int(n_convs), int(chunk_images)), "y3_net_set_early_chunk")

    # A tile forced through these setters survives plan(): the tuning table only fills the convs left on automatic
    # (tile -1 hands the conv back to the table / the library's heuristic).
    def _force(self, kind: str, fn, slot: int, tile: int):
        check(fn(self._h, slot, tile), f"y3_net_set_tile{kind}")
        forced = self.__dict__.setdefault("_forced_tiles", {})
        if tile >= 0:
            forced[(kind, slot)] = tile
        else:
            forced.pop((kind, slot), None)

    def set_tile(self, slot: int, tile: int):
        self._force("", self.lib.y3_net_set_tile, slot, tile)

    def set_tile_x3(self, slot: int, tile: int):
        self._force("_x3", self.lib.y3_net_set_tile_x3, slot, tile)

    def set_tile_x2(self, slot: int, tile: int):
        self._force("_x2", self.lib.y3_net_set_tile_x2, slot, tile)

    def set_tile_bf16(self, slot: int, tile: int):
        """Force a tile of the 16-bit conv family on conv `slot`: acts on bf16 and fp16 plans alike (one tile table, one field)."""
        self._force("_bf16", self.lib.y3_net_set_tile_bf16, slot, tile)

    def plan(self, max_batch: int, image_size, dtype: Optional[int] = None):
        """image_size: an int S (the S x S canvas) or an (H, W) pair, both sides multiples of 32 (y3_net_plan_hw).
        dtype: _lib.Y3_DTYPE_F32 (default, fp32 MFMA), _lib.Y3_DTYPE_F32X3 (fp32-accurate on the bf16 matrix cores:
        three bf16 planes per value), _lib.Y3_DTYPE_F32X2 (two fp16 planes per value, 2^-22 representation, |x| < 65504)
        _lib.Y3_DTYPE_BF16 (bf16 activations/weights, fp32 accumulate) or _lib.Y3_DTYPE_F16 (the same with IEEE fp16: 8 x closer to
        fp32, values beyond 65504 become inf; the fused stem and split-K only through set_stem_fusion_f16 / set_low_latency_f16)."""
        if dtype is None:
            dtype = self.dtype
        H, W = canvas_hw(image_size)
        check(self.lib.y3_net_plan_hw(self._h, max_batch, H, W, dtype), "y3_net_plan")
        self.max_batch, self.dtype, self.canvas = max_batch, dtype, (H, W)
        # the form grid_sizes() answers in -- g for an int plan, (gh, gw) for a pair plan -- is that of the last plan() a caller made
        self.image_size = int(image_size) if isinstance(image_size, (int, np.integer)) else (H, W)
        self._apply_tuning()

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
        kind, fn = {_lib.Y3_DTYPE_F32: ("", self.lib.y3_net_set_tile), _lib.Y3_DTYPE_BF16: ("_bf16", self.lib.y3_net_set_tile_bf16),
                    _lib.Y3_DTYPE_F32X3: ("_x3", self.lib.y3_net_set_tile_x3),
                    _lib.Y3_DTYPE_F32X2: ("_x2", self.lib.y3_net_set_tile_x2),
                    _lib.Y3_DTYPE_F16: ("_bf16", self.lib.y3_net_set_tile_bf16),
                    _lib.Y3_DTYPE_I8: ("_bf16", self.lib.y3_net_set_tile_bf16)}[self.dtype]
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
            check(fn(self._h, slot, tile), f"y3_net_set_tile{kind}")

    def grid_sizes(self, image_size=None):
        """Per head: g for an int image size, (gh, gw) for an (H, W) pair (default: what the net was planned with)."""
        return self.program.grid_sizes(image_size or self.image_size)

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
        """images [B,H,W,3] fp32 on the GPU -> [grid13, grid26, grid52], each [B,gh,gw,3,5+nc]."""
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
        ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in out])
        check(self.lib.y3_net_forward(self._h, _dev(images), B, ptrs, _lib.stream_ptr()), "y3_net_forward")
        return list(out)

    __call__ = forward

    def measure_sclk(self, images: torch.Tensor, out: Sequence[torch.Tensor], forwards: int = 30, conv: int = -1) -> float:
        """Shader clock (MHz) the chip holds under this network's load: `forwards` forwards back to back, in the last one
        a conv launch stamps s_memtime / s_memrealtime (y3_net_measure_sclk: the conv with the most FLOPs; conv >= 0:
        that conv slot, y3_net_measure_sclk_conv).  Raises when no launch of the plan / not that launch carries stamps."""
        _need_cuda(images, *out)
        ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in out])
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
        import numpy as np
        _need_cuda(images, *out)
        ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in out])
        n = len(self.conv_ops)
        mhz = (C.c_float * n)()
        t0 = (C.c_double * n)()
        t1 = (C.c_double * n)()
        check(self.lib.y3_net_measure_sclk_all(self._h, _dev(images), images.shape[0], ptrs, int(forwards), mhz, t0, t1,
                                               _lib.stream_ptr()), "y3_net_measure_sclk_all")
        return np.array(mhz[:], dtype=np.float64), np.array(t0[:]), np.array(t1[:])

    def read_tensor(self, tensor_id: int, batch: int) -> torch.Tensor:
        n = C.c_size_t()
        check(self.lib.y3_net_read_tensor(self._h, tensor_id, batch, None, C.byref(n), None), "y3_net_read_tensor")
        t = self.program.tensors[tensor_id]
        out = torch.empty((batch, self.canvas[0] // t.div, self.canvas[1] // t.div, t.channels), dtype=torch.float32, device="cuda")
        assert out.numel() == n.value
        check(self.lib.y3_net_read_tensor(self._h, tensor_id, batch, _dev(out), C.byref(n), _lib.stream_ptr()),
              "y3_net_read_tensor")
        return out

    # -- int8 plans (include/y3.h, "int8 plans"; the scheme restated in quant.py) ----------------------------------------------------
    def read_tensor_i8(self, tensor_id: int, batch: int) -> torch.Tensor:
        """The raw bytes of an int8 tensor of the last forward of an int8 plan: a tensor behind the cut, or the int8 copy of one that
        crosses it.  -> int8 [batch, h, w, C]."""
        n = C.c_size_t()
        check(self.lib.y3_net_read_tensor_i8(self._h, tensor_id, batch, None, C.byref(n), None), "y3_net_read_tensor_i8")
        t = self.program.tensors[tensor_id]
        out = torch.empty((batch, self.canvas[0] // t.div, self.canvas[1] // t.div, t.channels), dtype=torch.int8, device="cuda")
        assert out.numel() == n.value
        check(self.lib.y3_net_read_tensor_i8(self._h, tensor_id, batch, _dev(out), C.byref(n), _lib.stream_ptr()), "y3_net_read_tensor_i8")
        return out

    def set_act_scales(self, scales):
        """One fp32 scale per tensor of the program (entries <= 0 or None: unset), read by the next plan() in "i8"."""
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
        two sources of every concat conv the larger of their scales, sets the scales (set_act_scales) and returns them.  Offline: the
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
        scales = quant.equalize_concat(p, scales)
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
        _need_cuda(images)
        if images.dtype != torch.float32 or images.dim() != 4 or images.shape[3] != 3:
            raise Y3Error("images must be float32 [B,H,W,3]")
        B = self._plan_for(images)
        a = np.ascontiguousarray(np.asarray(anchors, np.float32).reshape(3, 3, 2))
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
        _need_cuda(images)
        if images.dtype != torch.float32 or images.dim() != 4 or images.shape[3] != 3:
            raise Y3Error("images must be float32 [B,H,W,3]")
        B = self._plan_for(images)
        a = np.ascontiguousarray(np.asarray(anchors, np.float32).reshape(3, 3, 2))
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
        max_blob_bytes.  Both default to the largest list of `batches`, which must then be a list or tuple."""
        M = int(max_boxes)
        outs = {}       # ring slot -> pinned rows, pinned counts, event: made on the slot's first use
        pending = []

        def result(entry):
            k, n = entry
            packed_host, nv_host, done = outs[k]
            done.synchronize()      # an event wait: the next batch's detect is already queued behind this one
            return packed_host[:n].numpy().copy(), nv_host[:n].numpy().copy()

        for i, handle, packed_dev, nv_dev, cur, stage, _ in self._detect_batches(
                "detect_stream", batches, anchors, M, iou_threshold, score_threshold, mode, depth, max_batch, max_blob_bytes, letterbox):
            k, n = i % stage.depth, handle.batch.shape[0]
            if k not in outs:
                outs[k] = (torch.empty((stage.max_batch, M, 7), dtype=torch.int32, pin_memory=True),
                           torch.empty((stage.max_batch,), dtype=torch.int32, pin_memory=True), torch.cuda.Event())
            packed_host, nv_host, done = outs[k]
            packed_host[:n].copy_(packed_dev[:n], non_blocking=True)
            nv_host[:n].copy_(nv_dev[:n], non_blocking=True)
            done.record(cur)
            pending.append((k, n))
            if len(pending) == stage.depth:     # its output buffers are the next to be reused
                yield result(pending.pop(0))
        while pending:
            yield result(pending.pop(0))

    def _detect_batches(self, who, batches, anchors, M, iou_threshold, score_threshold, mode, depth, max_batch, max_blob_bytes,
                        letterbox, keep_grids=False):
        """The loop detect_stream and evaluate_stream share: a generator that stages batch i+1 on the InputStage's copy stream,
        enqueues y3_net_detect (and, with letterbox, y3_unletterbox_detections) of batch i on the current stream, and yields
        (i, handle, packed_dev, nv_dev, stream, stage, grids) for the consumer to enqueue its own work on `stream` behind them.
        The device buffers are slot i % depth of a ring: the consumer's reads are ordered before their reuse by the stream.
        keep_grids: the consumer wants the raw head grids as well (`grids`: three [n,g,g,3,5+nc] views, otherwise None), so
        each batch takes the composed route include/y3.h documents as bit-identical to y3_net_detect: y3_net_forward into
        grid buffers made once here, y3_yolo_decode_scores, y3_nms_padded, y3_pack_detections.  One set of buffers serves
        every batch: all of it runs on the one stream."""
        if max_batch is None or max_blob_bytes is None:
            if not isinstance(batches, (list, tuple)):
                raise Y3Error(f"{who}: pass max_batch and max_blob_bytes when `batches` is not a list or tuple")
            if max_batch is None:
                max_batch = max((len(b) for b in batches), default=0)
            if max_blob_bytes is None:
                max_blob_bytes = max((packed_nbytes(b) for b in batches), default=0)
        S = self.image_size
        Hc, Wc = self.canvas
        if Hc <= 0:
            raise Y3Error(f"{who}: plan() the net first (the image size is the plan's)")
        if depth < 2:
            raise Y3Error(f"{who}: depth must be at least 2 (batch i+1 is staged while batch i is detected)")
        if max_batch < 1:
            return
        stage = InputStage(S, max_batch, max(int(max_blob_bytes), 16), depth)
        if max_batch > self.max_batch:
            self.plan(max_batch, S)
        a = np.ascontiguousarray(np.asarray(anchors, np.float32).reshape(3, 3, 2))
        dev = stage.device
        ring = [(torch.empty((max_batch, M, 7), dtype=torch.int32, device=dev),
                 torch.empty((max_batch,), dtype=torch.int32, device=dev)) for _ in range(stage.depth)]
        grid_bufs = None
        if keep_grids:
            nc, gs = self.program.nclasses, self._grid_hw()
            if nc <= 0:
                raise Y3Error(f"{who}: the program has no detection heads")
            N = sum(3 * gh * gw for gh, gw in gs)
            grid_bufs = [torch.empty((max_batch, gh, gw, 3, 5 + nc), dtype=torch.float32, device=dev) for gh, gw in gs]
            grid_ptrs, grid_hw = (C.c_void_p * 3)(*[t.data_ptr() for t in grid_bufs]), (C.c_int32 * 6)(*[v for g in gs for v in g])
            bboxes = torch.empty((max_batch, N, 4), dtype=torch.float32, device=dev)
            cls = torch.empty((max_batch, N), dtype=torch.int64, device=dev)
            scores = torch.empty((max_batch, N), dtype=torch.float32, device=dev)
            sel = torch.empty((max_batch, M), dtype=torch.int32, device=dev)
            ws_bytes = self.lib.y3_nms_workspace_bytes(max_batch, N)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        it = iter(batches)
        first = next(it, None)
        handle = stage.submit(first, mode, letterbox) if first is not None else None
        i = 0
        while handle is not None:
            nxt = next(it, None)
            following = stage.submit(nxt, mode, letterbox) if nxt is not None else None   # batch i+1 goes in before detect of batch i
            cur = torch.cuda.current_stream()
            cur.wait_event(handle.ready)
            n = handle.batch.shape[0]
            packed_dev, nv_dev = ring[i % stage.depth]
            sp = C.c_void_p(cur.cuda_stream)
            if keep_grids:      # the first n images of every buffer are a contiguous prefix
                check(self.lib.y3_net_forward(self._h, _dev(handle.batch), n, grid_ptrs, sp), "y3_net_forward")
                check(self.lib.y3_yolo_decode_scores_hw(grid_ptrs, grid_hw, n, nc, _fptr(a), _dev(bboxes), _dev(cls), _dev(scores), sp),
                      "y3_yolo_decode_scores")
                check(self.lib.y3_nms_padded(_dev(bboxes), _dev(scores), n, N, M, float(iou_threshold), float(score_threshold),
                                             _dev(sel), _dev(nv_dev), _dev(ws), ws_bytes, sp), "y3_nms_padded")
                check(self.lib.y3_pack_detections(_dev(bboxes), _dev(cls), _dev(scores), _dev(sel), _dev(nv_dev), n, N, M,
                                                  _dev(packed_dev), sp), "y3_pack_detections")
            else:
                check(self.lib.y3_net_detect(self._h, _dev(handle.batch), n, _fptr(a), M, float(iou_threshold),
                                             float(score_threshold), _dev(packed_dev), _dev(nv_dev), sp), "y3_net_detect")
            stage.release(handle)
            if letterbox:
                g = handle.geometry
                check(self.lib.y3_unletterbox_detections_hw(_dev(packed_dev), _dev(nv_dev), g.ctypes.data_as(C.POINTER(C.c_int32)), n, M, Hc, Wc,
                                                            C.c_void_p(cur.cuda_stream)), "y3_unletterbox_detections")
            yield i, handle, packed_dev, nv_dev, cur, stage, ([t[:n] for t in grid_bufs] if keep_grids else None)
            handle, i = following, i + 1

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
        the regulariser the reference's training loop adds (model.losses) is not part of it.  Each batch then takes the composed
        route y3_net_forward -> y3_yolo_decode_scores -> y3_nms_padded -> y3_pack_detections (bit-identical detections; the raw
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
        ap=None enqueues nothing new and returns exactly what is described above."""
        thresholds = [float(t) for t in score_thresholds]
        ap_thr = None if ap is None or ap is False else ap_iou_thresholds(ap)
        if loss and letterbox:
            raise Y3Error("evaluate_stream: loss=True cannot be combined with letterbox=True (the ground truth is not mapped onto the canvas)")
        if loss and self.canvas[0] != self.canvas[1]:
            raise ValueError(f"evaluate_stream: loss=True needs a square plan (the net is planned for {self.canvas[0]} x {self.canvas[1]}; "
                          "the loss kernels take one grid size per scale)")
        if loss and int(nclasses) != self.program.nclasses:
            raise Y3Error(f"evaluate_stream: loss=True needs nclasses = {self.program.nclasses}, the program's (got {int(nclasses)})")
        both = isinstance(one_class, str)
        if both and one_class != "both":
            raise Y3Error('evaluate_stream: one_class must be False, True or "both"')
        if not 1 <= len(thresholds) <= 16:
            raise Y3Error("evaluate_stream: 1 to 16 score thresholds")
        if max_gt is None:
            if not isinstance(gts, (list, tuple)):
                raise Y3Error("evaluate_stream: pass max_gt when `gts` is not a list or tuple")
            G = max((len(np.asarray(c).reshape(-1)) for g in gts for _, c in g), default=0) or 1
        else:
            G = int(max_gt)
        gt_iter, missing = iter(gts), object()
        nc, M, T = int(nclasses), int(max_boxes), len(thresholds)
        variants = (0, 1) if both else (int(bool(one_class)),)
        thr = np.asarray(thresholds, np.float32)
        counters = None
        n_counters = len(variants) * T * (5 * nc + 2)
        n_loss, n_ap = (14 if loss else 0), (nc + 2 if ap_thr is not None else 0)
        ap_records = []     # per batch, the [n, M, 2] records: on the device until the stream ends
        a = np.ascontiguousarray(np.asarray(anchors, np.float32).reshape(3, 3, 2))
        slots = {}      # ring slot -> pinned ground-truth words, their device copy, "copied" event
        for i, handle, packed_dev, nv_dev, cur, stage, grids in self._detect_batches(
                "evaluate_stream", batches, anchors, M, iou_threshold, min(thresholds), mode, depth, max_batch, max_blob_bytes, letterbox,
                keep_grids=bool(loss)):
            n, k = handle.batch.shape[0], i % stage.depth
            gt = next(gt_iter, missing)
            if gt is missing:
                raise Y3Error(f"evaluate_stream: `gts` ends before batch {i}")
            gt = list(gt)
            if len(gt) != n:
                raise Y3Error(f"evaluate_stream: batch {i} has {n} frames, its ground truth {len(gt)} entries")
            if counters is None:
                # one buffer of 64-bit words, read back once: the counters, then (loss) the [3,4] float64 sums, the images counted and the errors
                # ... then (ap) the nclasses + 2 ground-truth totals of y3_match_detections
                result = torch.zeros(n_counters + n_loss + n_ap, dtype=torch.int64, device=stage.device)
                counters = result[:n_counters].view(len(variants), T, 5 * nc + 2)
                if loss:
                    loss_sum, loss_images = result[n_counters:n_counters + 12].view(torch.float64).view(3, 4), result[n_counters + 12:n_counters + 14]
                    cells_d = torch.empty((stage.max_batch, G), dtype=torch.int32, device=stage.device)
                    loss_d = torch.empty((stage.max_batch, 3, 4), dtype=torch.float64, device=stage.device)
                    gs = [g for g, _ in self._grid_hw()]
            if k not in slots:
                words = stage.max_batch * (G * 5 + 1)
                slots[k] = (torch.empty(words, dtype=torch.int32, pin_memory=True),
                            torch.empty(words, dtype=torch.int32, device=stage.device), torch.cuda.Event(), [False])
            pinned, gt_dev, copied, used = slots[k]
            if used[0]:
                copied.synchronize()      # the slot's earlier copy (depth batches ago) has left the pinned words
            boxes_w, classes_w, count_w = _gt_views(pinned.numpy(), n, G)
            pack_ground_truth(gt, G, out=(boxes_w.view(np.float32), classes_w, count_w))
            words = n * (G * 5 + 1)
            gt_dev[:words].copy_(pinned[:words], non_blocking=True)
            copied.record(cur)
            used[0] = True
            boxes_d, classes_d, count_d = _gt_views(gt_dev, n, G)
            for v, oc in enumerate(variants):
                check(self.lib.y3_evaluate_detections(_dev(packed_dev), _dev(nv_dev), n, M, _dev(boxes_d), _dev(classes_d),
                                                      _dev(count_d), G, nc, float(evaluate_iou_threshold), _fptr(thr), T, oc,
                                                      _dev(counters[v]), C.c_void_p(cur.cuda_stream)), "y3_evaluate_detections")
            if ap_thr is not None:
                ap_records.append(torch.empty((n, M, 2), dtype=torch.int32, device=stage.device))
                check(self.lib.y3_match_detections(_dev(packed_dev), _dev(nv_dev), n, M, _dev(boxes_d), _dev(classes_d), _dev(count_d),
                                                   G, nc, _fptr(ap_thr), len(ap_thr), variants[0], _dev(ap_records[-1]),
                                                   _dev(result[n_counters + n_loss:]), C.c_void_p(cur.cuda_stream)), "y3_match_detections")
            if loss:
                assign_targets(boxes_d.view(torch.float32), classes_d, count_d, a, gs, nc, cells=cells_d[:n])
                yolo_loss(grids, a, nc, boxes_d.view(torch.float32), classes_d, cells_d[:n], loss=loss_d[:n])
                loss_sum += loss_d[:n].sum(dim=0)
                bad = (cells_d[:n, 0] == -3).sum()
                loss_images += torch.stack([n - bad, bad])
        if next(gt_iter, missing) is not missing:
            raise Y3Error("evaluate_stream: `gts` has more entries than there are batches")
        if counters is None:
            out = np.zeros(n_counters + n_loss + n_ap, np.int64)
        else:
            out = result.cpu().numpy()      # the one read-back: waits for the stream
        words, out = out, out[:n_counters].reshape(len(variants), T, 5 * nc + 2)
        counted = (out[0], out[1]) if both else out[0]
        if not loss and ap_thr is None:
            return counted
        ret = [counted]
        if loss:
            ret.append({"sum": words[n_counters:n_counters + 12].view(np.float64).reshape(3, 4).copy(),
                        "images": int(words[n_counters + 12]), "errors": int(words[n_counters + 13])})
        if ap_thr is not None:
            from .evaluate_detections import average_precision
            rec = torch.cat(ap_records).cpu().numpy() if ap_records else np.zeros((0, M, 2), np.int32)   # behind the read-back above
            ret.append(average_precision(rec.view(np.uint32), words[n_counters + n_loss:], nc, len(ap_thr)))
        return tuple(ret)

    def flops_per_image(self) -> float:
        return float(self.lib.y3_net_flops_per_image(self._h))

    def profile_convs(self, images: torch.Tensor) -> np.ndarray:
        _need_cuda(images)
        ms = np.zeros(len(self.conv_ops), np.float32)
        check(self.lib.y3_net_profile_convs(self._h, _dev(images), images.shape[0], _fptr(ms), len(ms),
                                            _lib.stream_ptr()), "y3_net_profile_convs")
        return ms


# ------------------------------------------------------------------------------------------------
def _grids_args(grids, square=True):
    _need_cuda(*grids)
    if len(grids) != 3:
        raise Y3Error("expected three grids")
    for g in grids:
        if g.dtype != torch.float32 or g.dim() != 5 or g.shape[3] != 3 or (square and g.shape[1] != g.shape[2]):
            raise Y3Error("each grid must be float32 [B,g,g,3,5+nc]" if square else "each grid must be float32 [B,gh,gw,3,5+nc]")
    ptrs = (C.c_void_p * 3)(*[g.data_ptr() for g in grids])
    if square:
        gs = (C.c_int32 * 3)(*[g.shape[1] for g in grids])
    else:       # grid_hw[3][2] = {gh, gw}
        gs = (C.c_int32 * 6)(*[v for g in grids for v in (g.shape[1], g.shape[2])])
    B = grids[0].shape[0]
    N = sum(3 * g.shape[1] * g.shape[2] for g in grids)
    return ptrs, gs, B, N


def _anchors(anchors_table):
    a = np.ascontiguousarray(anchors_table.detach().cpu().numpy() if isinstance(anchors_table, torch.Tensor)
                             else anchors_table, np.float32)
    if a.shape != (3, 3, 2):
        raise Y3Error("anchors_table must be [3,3,2]")
    return a


def yolo_decode(grids, anchors_table, nclasses):
    """-> (bboxes [B,N,4], confidence [B,N,1], class_probs [B,N,nc]).  Grids [B,gh,gw,3,5+nc]: each centre is normalised by
    its own axis (include/y3.h, y3_yolo_decode_hw), which for gh == gw is the reference's arithmetic bit for bit."""
    ptrs, gs, B, N = _grids_args(grids, square=False)
    a = _anchors(anchors_table)
    dev = grids[0].device
    bboxes = torch.empty((B, N, 4), dtype=torch.float32, device=dev)
    conf = torch.empty((B, N, 1), dtype=torch.float32, device=dev)
    probs = torch.empty((B, N, nclasses), dtype=torch.float32, device=dev)
    check(_lib.load().y3_yolo_decode_hw(ptrs, gs, B, nclasses, _fptr(a), _dev(bboxes), _dev(conf), _dev(probs),
                                     _lib.stream_ptr()), "y3_yolo_decode")
    return bboxes, conf, probs


def yolo_decode_scores(grids, anchors_table, nclasses):
    """fused decode + class arg-max/score -> (bboxes [B,N,4], class_indices [B,N] i64, scores [B,N])"""
    ptrs, gs, B, N = _grids_args(grids, square=False)
    a = _anchors(anchors_table)
    dev = grids[0].device
    bboxes = torch.empty((B, N, 4), dtype=torch.float32, device=dev)
    cls = torch.empty((B, N), dtype=torch.int64, device=dev)
    scores = torch.empty((B, N), dtype=torch.float32, device=dev)
    check(_lib.load().y3_yolo_decode_scores_hw(ptrs, gs, B, nclasses, _fptr(a), _dev(bboxes), _dev(cls), _dev(scores),
                                            _lib.stream_ptr()), "y3_yolo_decode_scores")
    return bboxes, cls, scores


def class_scores(conf, probs):
    _need_cuda(conf, probs)
    B, N, nc = probs.shape
    cls = torch.empty((B, N), dtype=torch.int64, device=probs.device)
    scores = torch.empty((B, N), dtype=torch.float32, device=probs.device)
    check(_lib.load().y3_class_scores(_dev(conf), _dev(probs), B, N, nc, _dev(cls), _dev(scores), _lib.stream_ptr()),
          "y3_class_scores")
    return cls, scores


def split3_planes(x: torch.Tensor) -> torch.Tensor:
    """fp32 [...,C] -> bf16 [...,3,C] with hi + mid + lo == x exactly (the activation format of Y3_DTYPE_F32X3)."""
    hi = x.to(torch.bfloat16)
    r1 = x - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    return torch.stack([hi, mid, lo], dim=-2).contiguous()


def split2_planes(x: torch.Tensor) -> torch.Tensor:
    """fp32 [...,C] -> fp16 [...,2,C]: h = fp16(x), l' = fp16((x - h) * 2^11), x == h + l' * 2^-11 up to 2^-22 |x|
    (the activation format of Y3_DTYPE_F32X2)."""
    h = x.to(torch.float16)
    lo = ((x - h.float()) * 2048.0).to(torch.float16)
    return torch.stack([h, lo], dim=-2).contiguous()


def preprocess_image(image: torch.Tensor, batch: torch.Tensor, slot: int, divide_after: bool = False, letterbox: bool = False):
    """image [H,W,3|4] uint8 or float32 on the GPU -> batch[slot] ([Hc,Wc,3] fp32, the canvas the batch's shape names; values in [0,1] for uint8 input):
    decode_image's uint8->float conversion fused with tf.image.resize's bilinear resampling.  divide_after=True is
    the tfrecords source's order (reference: core/load_tfrecords.py:46-48): resize the 0..255 values, then / 255.
    letterbox=True keeps the aspect ratio and pads with zeros (reference: core/utils.py:17-28, resize_image); the whole
    slot is written."""
    _need_cuda(image, batch)
    if image.dim() != 3 or image.dtype not in (torch.uint8, torch.float32) or batch.dtype != torch.float32:
        raise Y3Error("image must be [H,W,C] uint8/float32 and batch float32 [B,Hc,Wc,3]")
    if batch.dim() != 4 or batch.shape[3] != 3 or not (0 <= slot < batch.shape[0]):
        raise Y3Error("batch must be [B,Hc,Wc,3] and slot inside it")
    H, W, C_ = image.shape
    mode = (2 if divide_after else 1) if image.dtype == torch.uint8 else 0
    if divide_after and mode == 0:
        raise Y3Error("divide_after applies to uint8 images")
    if letterbox:
        mode |= _lib.Y3_IMAGE_LETTERBOX
    check(_lib.load().y3_preprocess_image_hw(_dev(image), mode, H, W, C_, _dev(batch), slot,
                                             batch.shape[1], batch.shape[2], _lib.stream_ptr()), "y3_preprocess_image")
    return batch


# y3_image_desc (include/y3.h), as a NumPy structured dtype: what pack_images returns and preprocess_batch takes
IMAGE_DESC_DTYPE = np.dtype([("offset", "<u8"), ("height", "<i4"), ("width", "<i4"), ("channels", "<i4"), ("mode", "<i4")])
_BLOB_ALIGN = 16     # image starts inside a pixel blob


def _image_modes(images, mode):
    if np.ndim(mode) == 0:
        modes = [int(mode)] * len(images)
    else:
        modes = [int(m) for m in mode]
        if len(modes) != len(images):
            raise Y3Error(f"pack_images: {len(modes)} modes for {len(images)} images")
    for i, (im, m) in enumerate(zip(images, modes)):
        if not isinstance(im, np.ndarray) or im.ndim != 3 or im.shape[2] not in (3, 4) or 0 in im.shape:
            raise Y3Error(f"pack_images: image {i} must be a non-empty NumPy array [H,W,3|4]")
        want = {0: np.float32, 1: np.uint8, 2: np.uint8}.get(m)
        if want is None:
            raise Y3Error(f"pack_images: image {i}: mode must be 0, 1 or 2 (got {m})")
        if im.dtype != want:
            raise Y3Error(f"pack_images: image {i} is {im.dtype}, mode {m} takes {np.dtype(want)}")
    return modes


def _blob_offsets(images):
    offsets, end = [], 0
    for im in images:
        start = -(-end // _BLOB_ALIGN) * _BLOB_ALIGN
        offsets.append(start)
        end = start + im.nbytes
    return offsets, end


def packed_nbytes(images) -> int:
    """Bytes pack_images needs for this list (image starts 16-byte aligned)."""
    return _blob_offsets(images)[1]


def _image_flags(images, letterbox):
    if np.ndim(letterbox) == 0:
        return [_lib.Y3_IMAGE_LETTERBOX if letterbox else 0] * len(images)
    flags = [_lib.Y3_IMAGE_LETTERBOX if f else 0 for f in letterbox]
    if len(flags) != len(images):
        raise Y3Error(f"pack_images: {len(flags)} letterbox flags for {len(images)} images")
    return flags


def pack_images(images, mode, out: Optional[np.ndarray] = None, letterbox=False):
    """A list of [H,W,3|4] uint8 / float32 arrays -> (blob_u8, descs): one contiguous byte buffer with every image start
    16-byte aligned, and the y3_image_desc array (IMAGE_DESC_DTYPE) that names them.  Pure NumPy.
    mode: one value for the whole list or one per image -- 0 float32, 1 uint8 scaled by 1/255 before the resize (the
    image_file / images_dir sources), 2 uint8 divided by 255 after it (the tfrecords source).
    letterbox: one bool for the whole list or one per image -- True sets Y3_IMAGE_LETTERBOX in the descriptor's mode: the
    image keeps its aspect ratio and is padded with zeros (core/utils.resize_image) instead of being stretched.
    out: a 1-D uint8 array to pack into (e.g. a view of pinned memory); blob_u8 is then its used prefix."""
    images = list(images)
    modes = _image_modes(images, mode)
    flags = _image_flags(images, letterbox)
    offsets, total = _blob_offsets(images)
    if out is None:
        out = np.empty(total, np.uint8)
    elif not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.ndim != 1 or not out.flags.c_contiguous:
        raise Y3Error("pack_images: out must be a contiguous 1-D uint8 array")
    elif out.size < total:
        raise Y3Error(f"pack_images: out holds {out.size} bytes, the images need {total}")
    descs = np.zeros(len(images), IMAGE_DESC_DTYPE)
    for i, (im, m, f, off) in enumerate(zip(images, modes, flags, offsets)):
        np.copyto(out[off:off + im.nbytes].view(im.dtype).reshape(im.shape), im)
        descs[i] = (off, im.shape[0], im.shape[1], im.shape[2], m | f)
    return out[:total], descs


def letterbox_geometries(descs: np.ndarray, image_size) -> np.ndarray:
    """The descriptor array of pack_images -> int32 [n,4] (sh, sw, top, left): where each image lies on the
    canvas (image_size: an int S or an (H, W) pair), the whole canvas (H, W, 0, 0) for an image without the letterbox flag.  One host call for the whole batch
    (y3_letterbox_geometry; no GPU needed); the rows unletterbox_detections takes."""
    if not isinstance(descs, np.ndarray) or descs.dtype != IMAGE_DESC_DTYPE or descs.ndim != 1:
        raise Y3Error("descs must be the descriptor array of pack_images")
    d = np.ascontiguousarray(descs)
    geoms = np.empty((len(d), 4), np.int32)
    Hc, Wc = canvas_hw(image_size)
    check(_lib.load().y3_letterbox_geometry_hw(d.ctypes.data_as(C.POINTER(_lib.ImageDesc)), len(d), Hc, Wc,
                                               geoms.ctypes.data_as(C.POINTER(C.c_int32))), "y3_letterbox_geometry")
    return geoms


def unletterbox_detections(packed: torch.Tensor, num_valid: torch.Tensor, geoms, image_size):
    """packed [B,M,7] int32 words and num_valid [B] int32 on the GPU (Net.detect / pack_detections), geoms int32 [B,4]
    on the host (letterbox_geometries): the boxes of the valid rows are rewritten in place from the padded canvas to
    the coordinates of the source frames (y3_unletterbox_detections; host restatement: core/utils.unletterbox_boxes).
    Nothing else is touched.  image_size: the canvas, an int S or an (H, W) pair.  Enqueues on the current stream only."""
    _need_cuda(packed, num_valid)
    if packed.dtype != torch.int32 or packed.dim() != 3 or packed.shape[2] != 7 or not packed.is_contiguous():
        raise Y3Error("packed must be contiguous int32 [B,M,7]")
    if num_valid.dtype != torch.int32 or num_valid.shape != (packed.shape[0],) or not num_valid.is_contiguous():
        raise Y3Error("num_valid must be contiguous int32 [B]")
    g = np.ascontiguousarray(geoms, dtype=np.int32)
    if g.shape != (packed.shape[0], 4):
        raise Y3Error(f"geoms must be int32 [{packed.shape[0]},4]")
    Hc, Wc = canvas_hw(image_size)
    check(_lib.load().y3_unletterbox_detections_hw(_dev(packed), _dev(num_valid), g.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   packed.shape[0], packed.shape[1], Hc, Wc, _lib.stream_ptr()),
          "y3_unletterbox_detections")
    return packed


def pack_ground_truth(gts, max_gt: Optional[int] = None, out=None):
    """A list of per-image (boxes [g,4], classes [g]) -> padded (boxes [B,G,4] float32, classes [B,G] int32, count [B] int32),
    the ground-truth form of evaluate_detections.  Pure NumPy.  G = max_gt, by default the largest g of the list (at least 1);
    an image with more rows than max_gt raises.  out: the three arrays to fill (e.g. views of pinned memory); rows behind
    an image's count are zeroed."""
    gts = [(np.asarray(b, np.float32).reshape(-1, 4), np.asarray(c).reshape(-1)) for b, c in gts]
    for i, (b, c) in enumerate(gts):
        if len(b) != len(c):
            raise Y3Error(f"pack_ground_truth: image {i} has {len(b)} boxes and {len(c)} classes")
    most = max((len(c) for _, c in gts), default=0)
    G = max(most, 1) if max_gt is None else int(max_gt)
    if G < 1 or most > G:
        raise Y3Error(f"pack_ground_truth: max_gt = {G}, the images hold up to {most} boxes")
    B = len(gts)
    if out is None:
        out = (np.empty((B, G, 4), np.float32), np.empty((B, G), np.int32), np.empty((B,), np.int32))
    boxes, classes, count = out
    if (boxes.shape, classes.shape, count.shape) != ((B, G, 4), (B, G), (B,)) or \
            (boxes.dtype, classes.dtype, count.dtype) != (np.float32, np.int32, np.int32):
        raise Y3Error(f"pack_ground_truth: out must be float32 [{B},{G},4], int32 [{B},{G}], int32 [{B}]")
    boxes[...] = 0
    classes[...] = 0
    for i, (b, c) in enumerate(gts):
        boxes[i, :len(b)] = b
        classes[i, :len(c)] = c
        count[i] = len(c)
    return boxes, classes, count


def _gt_views(words, n: int, G: int):
    """A 1-D int32 buffer (NumPy or torch) -> its (boxes [n,G,4], classes [n,G], count [n]) parts, boxes still as words."""
    nb, ncl = n * G * 4, n * G
    return words[:nb].reshape(n, G, 4), words[nb:nb + ncl].reshape(n, G), words[nb + ncl:nb + ncl + n]


def evaluate_detections(packed: torch.Tensor, num_valid: torch.Tensor, gt_boxes: torch.Tensor, gt_classes: torch.Tensor,
                        gt_count: torch.Tensor, nclasses: int, iou_threshold: float, score_thresholds, one_class=False,
                        counters: Optional[torch.Tensor] = None):
    """packed [B,M,7] int32 words and num_valid [B] int32 on the GPU (Net.detect at the LOWEST threshold of the sweep,
    pack_detections, unletterbox_detections), ground truth on the GPU as pack_ground_truth lays it out (gt_boxes [B,G,4]
    float32, gt_classes [B,G] int32, gt_count [B] int32) -> the counters of every score threshold, int64
    [T, 5*nclasses + 2] on the GPU: preds, gts, tp, fp, fn (each [nclasses]), errors, examples per threshold
    (y3_evaluate_detections; host restatement: evaluate_detections.sweep_counters).  counters=None: a zeroed tensor is
    made; otherwise the call ADDS to the one given.  Enqueues on the current stream only."""
    _need_cuda(packed, num_valid, gt_boxes, gt_classes, gt_count, counters)
    if packed.dtype != torch.int32 or packed.dim() != 3 or packed.shape[2] != 7:
        raise Y3Error("packed must be contiguous int32 [B,M,7]")
    B, M = packed.shape[0], packed.shape[1]
    if num_valid.dtype != torch.int32 or num_valid.shape != (B,):
        raise Y3Error(f"num_valid must be int32 [{B}]")
    if gt_boxes.dtype != torch.float32 or gt_boxes.dim() != 3 or gt_boxes.shape[0] != B or gt_boxes.shape[2] != 4:
        raise Y3Error(f"gt_boxes must be float32 [{B},G,4]")
    G = gt_boxes.shape[1]
    if gt_classes.dtype != torch.int32 or gt_classes.shape != (B, G):
        raise Y3Error(f"gt_classes must be int32 [{B},{G}]")
    if gt_count.dtype != torch.int32 or gt_count.shape != (B,):
        raise Y3Error(f"gt_count must be int32 [{B}]")
    thr = np.ascontiguousarray(np.asarray(score_thresholds, np.float32).reshape(-1))
    nc = int(nclasses)
    if counters is None:
        counters = torch.zeros((len(thr), 5 * nc + 2), dtype=torch.int64, device=packed.device)
    elif counters.dtype != torch.int64 or counters.shape != (len(thr), 5 * nc + 2):
        raise Y3Error(f"counters must be int64 [{len(thr)},{5 * nc + 2}]")
    check(_lib.load().y3_evaluate_detections(_dev(packed), _dev(num_valid), B, M, _dev(gt_boxes), _dev(gt_classes), _dev(gt_count),
                                             G, nc, float(iou_threshold), _fptr(thr), len(thr), int(bool(one_class)),
                                             _dev(counters), _lib.stream_ptr()), "y3_evaluate_detections")
    return counters


def ap_iou_thresholds(ap):
    """The `ap` argument of evaluate_stream / evaluate -> its IoU thresholds, float32 [K]: True means the ten thresholds 0.5, 0.55,
    ..., 0.95 of mAP@[.5:.95] (evaluate_detections.AP_IOU_THRESHOLDS), a sequence means those thresholds."""
    from .evaluate_detections import AP_IOU_THRESHOLDS
    thr = AP_IOU_THRESHOLDS if ap is True else np.ascontiguousarray(np.asarray(ap, np.float32).reshape(-1))
    if not 1 <= len(thr) <= 16 or not np.isfinite(thr).all():
        raise Y3Error("ap: 1 to 16 finite IoU thresholds (or True for 0.5, 0.55, ..., 0.95)")
    return thr


def match_detections(packed: torch.Tensor, num_valid: torch.Tensor, gt_boxes: torch.Tensor, gt_classes: torch.Tensor,
                     gt_count: torch.Tensor, nclasses: int, iou_thresholds, one_class=False,
                     records: Optional[torch.Tensor] = None, gt_totals: Optional[torch.Tensor] = None):
    """The inputs of evaluate_detections -> (records int32 [B,M,2], gt_totals int64 [nclasses + 2]) on the GPU: per image the
    greedy matching behind COCO-style average precision, at every IoU threshold of iou_thresholds [K <= 16] (y3_match_detections;
    host restatement: evaluate_detections.match_detections, which also names the words; evaluate_detections.average_precision
    integrates the records of a data set).  The rows are matched in ROW order -- Net.detect writes them in descending score --
    and nothing is sorted.  records: the tensor to write (every row of it is written; torch has no arithmetic on uint32, so the
    words travel as int32 like the packed rows: .view(np.uint32) on the host); gt_totals=None: a zeroed tensor is made, otherwise
    the call ADDS to the one given.  Enqueues on the current stream only."""
    _need_cuda(packed, num_valid, gt_boxes, gt_classes, gt_count, records, gt_totals)
    if packed.dtype != torch.int32 or packed.dim() != 3 or packed.shape[2] != 7:
        raise Y3Error("packed must be contiguous int32 [B,M,7]")
    B, M = packed.shape[0], packed.shape[1]
    if num_valid.dtype != torch.int32 or num_valid.shape != (B,):
        raise Y3Error(f"num_valid must be int32 [{B}]")
    if gt_boxes.dtype != torch.float32 or gt_boxes.dim() != 3 or gt_boxes.shape[0] != B or gt_boxes.shape[2] != 4:
        raise Y3Error(f"gt_boxes must be float32 [{B},G,4]")
    G = gt_boxes.shape[1]
    if gt_classes.dtype != torch.int32 or gt_classes.shape != (B, G):
        raise Y3Error(f"gt_classes must be int32 [{B},{G}]")
    if gt_count.dtype != torch.int32 or gt_count.shape != (B,):
        raise Y3Error(f"gt_count must be int32 [{B}]")
    thr = np.ascontiguousarray(np.asarray(iou_thresholds, np.float32).reshape(-1))
    nc = int(nclasses)
    if records is None:
        records = torch.empty((B, M, 2), dtype=torch.int32, device=packed.device)
    elif records.dtype != torch.int32 or records.shape != (B, M, 2):
        raise Y3Error(f"records must be int32 [{B},{M},2]")
    if gt_totals is None:
        gt_totals = torch.zeros((max(nc, 0) + 2,), dtype=torch.int64, device=packed.device)
    elif gt_totals.dtype != torch.int64 or gt_totals.shape != (nc + 2,):
        raise Y3Error(f"gt_totals must be int64 [{nc + 2}]")
    check(_lib.load().y3_match_detections(_dev(packed), _dev(num_valid), B, M, _dev(gt_boxes), _dev(gt_classes), _dev(gt_count),
                                          G, nc, _fptr(thr), len(thr), int(bool(one_class)), _dev(records), _dev(gt_totals),
                                          _lib.stream_ptr()), "y3_match_detections")
    return records, gt_totals


def _gt_args(who, gt_boxes, gt_classes):
    if gt_boxes.dtype != torch.float32 or gt_boxes.dim() != 3 or gt_boxes.shape[2] != 4:
        raise Y3Error(f"{who}: gt_boxes must be float32 [B,G,4]")
    B, G = gt_boxes.shape[0], gt_boxes.shape[1]
    if gt_classes.dtype != torch.int32 or gt_classes.shape != (B, G):
        raise Y3Error(f"{who}: gt_classes must be int32 [{B},{G}]")
    return B, G


def assign_targets(gt_boxes: torch.Tensor, gt_classes: torch.Tensor, gt_count: torch.Tensor, anchors_table, grid_sizes,
                   nclasses: int, cells: Optional[torch.Tensor] = None):
    """Ground truth on the GPU as pack_ground_truth lays it out (gt_boxes [B,G,4] float32, gt_classes [B,G] int32, gt_count [B]
    int32) -> cells [B,G] int32 on the GPU: per ground-truth row the index of its label's row in decode's row order (best
    anchor by width/height IoU, the cell of its centre, the later row winning a shared cell), -1 behind the count, -2 for a row
    that lost its cell, -3 for the rows of an error image (y3_yolo_assign_targets; reference
    core/preprocess_dataset.py::_arrange_in_grid in sparse form; host restatement: core.preprocess_dataset.assign_targets).
    cells: the tensor to write.  Enqueues on the current stream only."""
    _need_cuda(gt_boxes, gt_classes, gt_count, cells)
    B, G = _gt_args("assign_targets", gt_boxes, gt_classes)
    if gt_count.dtype != torch.int32 or gt_count.shape != (B,):
        raise Y3Error(f"assign_targets: gt_count must be int32 [{B}]")
    gs = [int(g) for g in grid_sizes]
    if len(gs) != 3:
        raise Y3Error("assign_targets: three grid sizes")
    a = _anchors(anchors_table)
    if cells is None:
        cells = torch.empty((B, G), dtype=torch.int32, device=gt_boxes.device)
    elif cells.dtype != torch.int32 or cells.shape != (B, G):
        raise Y3Error(f"assign_targets: cells must be int32 [{B},{G}]")
    check(_lib.load().y3_yolo_assign_targets(_dev(gt_boxes), _dev(gt_classes), _dev(gt_count), B, G, int(nclasses),
                                             (C.c_int32 * 3)(*gs), _fptr(a), _dev(cells), _lib.stream_ptr()),
          "y3_yolo_assign_targets")
    return cells


def yolo_loss(grids, anchors_table, nclasses: int, gt_boxes: torch.Tensor, gt_classes: torch.Tensor, cells: torch.Tensor,
              loss: Optional[torch.Tensor] = None):
    """The raw head grids of Net.forward ([B,g,g,3,5+nc] each) + ground truth + the cells of assign_targets -> float64 [B,3,4] on
    the GPU: per image and scale the sums xy, wh, obj, class of reference core/loss_func.py (y3_yolo_loss; host restatement:
    core.loss_func.loss_from_cells).  An error image (cells -3) gets twelve zeros.  Each image's numbers are bit-identical
    whatever batch it is in.  This is the validation loss: no gradient, and the regulariser the reference's training loop adds
    (model.losses) is not part of it.  loss: the tensor to write (overwritten, not added to).  Enqueues on the current stream only."""
    ptrs, gs, B, _ = _grids_args(grids)
    _need_cuda(gt_boxes, gt_classes, cells, loss)
    nc = int(nclasses)
    if any(g.shape[4] != 5 + nc for g in grids):
        raise Y3Error(f"yolo_loss: each grid must be float32 [B,g,g,3,{5 + nc}]")
    if any(g.shape[0] != B for g in grids):
        raise Y3Error("yolo_loss: the grids hold unlike batches")
    Bg, G = _gt_args("yolo_loss", gt_boxes, gt_classes)
    if Bg != B:
        raise Y3Error(f"yolo_loss: {B} images in the grids, {Bg} in the ground truth")
    if cells.dtype != torch.int32 or cells.shape != (B, G):
        raise Y3Error(f"yolo_loss: cells must be int32 [{B},{G}]")
    a = _anchors(anchors_table)
    if loss is None:
        loss = torch.empty((B, 3, 4), dtype=torch.float64, device=gt_boxes.device)
    elif loss.dtype != torch.float64 or loss.shape != (B, 3, 4):
        raise Y3Error(f"yolo_loss: loss must be float64 [{B},3,4]")
    check(_lib.load().y3_yolo_loss(ptrs, gs, B, nc, _fptr(a), _dev(gt_boxes), _dev(gt_classes), _dev(cells), G, _dev(loss),
                                   _lib.stream_ptr()), "y3_yolo_loss")
    return loss


def preprocess_batch(blob_dev: torch.Tensor, descs: np.ndarray, batch: torch.Tensor, first_slot: int = 0):
    """The pixel blob of pack_images on the GPU (1-D uint8) -> batch[first_slot + i] for image i, one launch per 64
    images (y3_preprocess_batch); every slot has the bits preprocess_image gives for the same image."""
    _need_cuda(blob_dev, batch)
    if blob_dev.dtype != torch.uint8 or blob_dev.dim() != 1:
        raise Y3Error("blob_dev must be a 1-D uint8 tensor")
    if not isinstance(descs, np.ndarray) or descs.dtype != IMAGE_DESC_DTYPE or descs.ndim != 1:
        raise Y3Error("descs must be the descriptor array of pack_images")
    if batch.dtype != torch.float32 or batch.dim() != 4 or batch.shape[3] != 3:
        raise Y3Error("batch must be float32 [B,Hc,Wc,3]")
    if not (0 <= first_slot and first_slot + len(descs) <= batch.shape[0]):
        raise Y3Error(f"slots {first_slot}..{first_slot + len(descs) - 1} are outside the batch of {batch.shape[0]}")
    d = np.ascontiguousarray(descs)
    check(_lib.load().y3_preprocess_batch_hw(_dev(blob_dev), blob_dev.numel(), d.ctypes.data_as(C.POINTER(_lib.ImageDesc)),
                                             len(d), _dev(batch), int(first_slot), batch.shape[1], batch.shape[2], _lib.stream_ptr()),
          "y3_preprocess_batch")
    return batch


class StagedBatch:
    """What InputStage.submit returns: `batch` ([n,S,S,3] fp32 on the GPU) holds the images once a stream has waited on
    the event `ready`; hand it back with InputStage.release when the consumer's work on it is enqueued.  `geometry`
    (int32 [n,4] on the host: sh, sw, top, left) says where each frame lies in its slot."""

    def __init__(self, slot, batch, ready, geometry):
        self.slot, self.batch, self.ready, self.geometry = slot, batch, ready, geometry


class _StageSlot:
    def __init__(self, image_size, max_batch, max_blob_bytes, device):
        self.pinned = torch.empty(max_blob_bytes, dtype=torch.uint8, pin_memory=True)
        self.pinned_np = self.pinned.numpy()
        self.blob_dev = torch.empty(max_blob_bytes, dtype=torch.uint8, device=device)
        self.batch = torch.empty((max_batch, *canvas_hw(image_size), 3), dtype=torch.float32, device=device)
        self.ready = torch.cuda.Event()      # copy stream: pixels copied and resized into `batch`
        self.released = torch.cuda.Event()   # consumer stream: `batch` has been read
        self.state = "free"                  # free -> held (submit) -> released (release) -> held ...


class InputStage:
    """Host frames -> device batches, overlapped with the consumer: a ring of `depth` slots, each a pinned host blob, a
    device blob and a device batch [max_batch,S,S,3], fed by one copy stream.
    submit(images, mode, letterbox) packs the list into the next slot's pinned blob and enqueues, on the copy stream, one
    host-to-device copy and y3_preprocess_batch; release(handle) tells the stage that the consumer's reads are enqueued.
    Every wait is on an event: the host waits for `ready` of the slot's previous use before it overwrites the pinned
    blob, the copy stream waits for `released` before it overwrites the device buffers.  Nothing synchronises the device."""

    def __init__(self, image_size, max_batch: int, max_blob_bytes: int, depth: int = 2):
        _lib.require_gpu()      # image_size: an int S or an (H, W) canvas
        if min(canvas_hw(image_size)) < 1 or max_batch < 1 or max_blob_bytes < 1 or depth < 1:
            raise Y3Error("InputStage: image_size, max_batch, max_blob_bytes and depth must be at least 1")
        self.image_size = int(image_size) if isinstance(image_size, (int, np.integer)) else canvas_hw(image_size)
        self.max_batch, self.depth = int(max_batch), int(depth)
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.stream = torch.cuda.Stream(self.device)
        self.slots = [_StageSlot(self.image_size, self.max_batch, int(max_blob_bytes), self.device) for _ in range(self.depth)]
        for s in self.slots:     # used on the copy stream for as long as the stage lives
            s.blob_dev.record_stream(self.stream)
            s.batch.record_stream(self.stream)
        self._next = 0

    def submit(self, images, mode, letterbox=False) -> StagedBatch:
        images = list(images)
        if not 1 <= len(images) <= self.max_batch:
            raise Y3Error(f"InputStage.submit: {len(images)} images, the stage holds 1..{self.max_batch}")
        slot = self.slots[self._next]
        if slot.state == "held":
            raise Y3Error(f"InputStage.submit: all {self.depth} slots are in use; release() the oldest batch first")
        if slot.state == "released":
            slot.ready.synchronize()     # the slot's earlier copy has left the pinned blob
        blob, descs = pack_images(images, mode, out=slot.pinned_np, letterbox=letterbox)
        geometry = letterbox_geometries(descs, self.image_size)     # one host call per batch
        n = blob.size
        with torch.cuda.stream(self.stream):
            if slot.state == "released":
                self.stream.wait_event(slot.released)
            slot.blob_dev[:n].copy_(slot.pinned[:n], non_blocking=True)
            preprocess_batch(slot.blob_dev, descs, slot.batch, 0)
            slot.ready.record(self.stream)
        slot.state = "held"
        self._next = (self._next + 1) % self.depth
        return StagedBatch(slot, slot.batch[:len(images)], slot.ready, geometry)

    def release(self, handle: StagedBatch):
        """Call on the consumer's stream after its last use of handle.batch has been enqueued."""
        if handle.slot.state != "held" or handle.ready is not handle.slot.ready:
            raise Y3Error("InputStage.release: not a batch in flight")
        handle.slot.released.record(torch.cuda.current_stream())
        handle.slot.state = "released"


_ws_cache: Dict[tuple, torch.Tensor] = {}


def nms_padded(bboxes, scores, max_output_size, iou_threshold, score_threshold):
    """-> (selected_indices_padded [B,M] i32, num_valid [B] i32)"""
    _need_cuda(bboxes, scores)
    if bboxes.dtype != torch.float32 or scores.dtype != torch.float32:
        raise Y3Error("boxes and scores must be float32")
    B, N = scores.shape
    lib = _lib.load()
    need = lib.y3_nms_workspace_bytes(B, N)
    key = (bboxes.device.index, need)
    ws = _ws_cache.get(key)
    if ws is None:
        _ws_cache.clear()
        ws = _ws_cache[key] = torch.empty(need, dtype=torch.uint8, device=bboxes.device)
    sel = torch.empty((B, int(max_output_size)), dtype=torch.int32, device=bboxes.device)
    nv = torch.empty((B,), dtype=torch.int32, device=bboxes.device)
    check(lib.y3_nms_padded(_dev(bboxes), _dev(scores), B, N, int(max_output_size), float(iou_threshold),
                            float(score_threshold), _dev(sel), _dev(nv), _dev(ws), need, _lib.stream_ptr()),
          "y3_nms_padded")
    return sel, nv


def pack_detections(bboxes, cls, scores, sel, nv):
    """-> [B,M,7] int32 words: box (4 x f32 bits), score (f32 bits), class, index; rows >= num_valid zero"""
    _need_cuda(bboxes, cls, scores, sel, nv)
    B, N = scores.shape
    M = sel.shape[1]
    out = torch.empty((B, M, 7), dtype=torch.int32, device=bboxes.device)
    check(_lib.load().y3_pack_detections(_dev(bboxes), _dev(cls), _dev(scores), _dev(sel), _dev(nv), B, N, M, _dev(out),
                                         _lib.stream_ptr()), "y3_pack_detections")
    return out


def unpack_detections(packed: torch.Tensor):
    """[.., M, 7] int32 words -> (boxes f32 [..,M,4], scores f32 [..,M], classes i32, indices i32)"""
    f = packed[..., :5].contiguous().view(torch.float32)
    return f[..., :4], f[..., 4], packed[..., 5], packed[..., 6]
