"""The surface of yolo_v3_tf2_amd.runtime (no GPU): its public names, the public methods of Net, InputStage and StagedBatch, the
signature text of every public function and method, and that what carried a docstring still carries one.  The literals below were
taken from the single-file runtime.py before it was split by concern; the module stays the import point of every drop-in module,
tool and test, so they change only with a deliberate change of the interface."""
import inspect

import pytest

# names that leaked from runtime.py's own imports: allowed, not required
LEAKED = {"C", "np", "torch", "annotations", "Dict", "List", "Optional", "Sequence"}

NAMES = ['AuxDesc', 'AuxOp', 'BN_EPS', 'ConvDesc', 'ConvOp', 'IMAGE_DESC_DTYPE', 'InputStage', 'Net', 'Program', 'StagedBatch',
         'TensorDesc', 'Y3Error', 'ap_iou_thresholds', 'assign_targets', 'canvas_hw', 'check', 'class_scores', 'evaluate_detections',
         'letterbox_geometries', 'match_detections', 'nms_padded', 'pack_detections', 'pack_ground_truth', 'pack_images', 'packed_nbytes',
         'preprocess_batch', 'preprocess_image', 'rect_anchors', 'rect_canvas', 'split2_planes', 'split3_planes', 'tuning_table_path',
         'unletterbox_detections', 'unpack_detections', 'yolo_decode', 'yolo_decode_scores', 'yolo_loss']

_T = "'torch.Tensor'"
_OT = "'Optional[torch.Tensor]'"
_OI = "'Optional[int]'"
_GT = f"gt_boxes: {_T}, gt_classes: {_T}, gt_count: {_T}"

FUNCTIONS = {
    'ap_iou_thresholds': '(ap)',
    'assign_targets': f"({_GT}, anchors_table, grid_sizes, nclasses: 'int', cells: {_OT} = None)",
    'canvas_hw': '(image_size)',
    'check': "(status: 'int', what: 'str' = '')",
    'class_scores': '(conf, probs)',
    'evaluate_detections': f"(packed: {_T}, num_valid: {_T}, {_GT}, nclasses: 'int', iou_threshold: 'float', score_thresholds, one_class=False, "
                           f"counters: {_OT} = None)",
    'letterbox_geometries': "(descs: 'np.ndarray', image_size) -> 'np.ndarray'",
    'match_detections': f"(packed: {_T}, num_valid: {_T}, {_GT}, nclasses: 'int', iou_thresholds, one_class=False, records: {_OT} = None, "
                        f"gt_totals: {_OT} = None)",
    'nms_padded': '(bboxes, scores, max_output_size, iou_threshold, score_threshold)',
    'pack_detections': '(bboxes, cls, scores, sel, nv)',
    'pack_ground_truth': f"(gts, max_gt: {_OI} = None, out=None)",
    'pack_images': "(images, mode, out: 'Optional[np.ndarray]' = None, letterbox=False)",
    'packed_nbytes': "(images) -> 'int'",
    'preprocess_batch': f"(blob_dev: {_T}, descs: 'np.ndarray', batch: {_T}, first_slot: 'int' = 0)",
    'preprocess_image': f"(image: {_T}, batch: {_T}, slot: 'int', divide_after: 'bool' = False, letterbox: 'bool' = False)",
    'rect_anchors': "(anchors_table, image_size: 'int', canvas)",
    'rect_canvas': "(height: 'int', width: 'int', image_size: 'int', stride: 'int' = 32)",
    'split2_planes': f"(x: {_T}) -> {_T}",
    'split3_planes': f"(x: {_T}) -> {_T}",
    'tuning_table_path': "(tag: 'str', batch: 'int', image_size) -> 'str'",
    'unletterbox_detections': f"(packed: {_T}, num_valid: {_T}, geoms, image_size)",
    'unpack_detections': f"(packed: {_T})",
    'yolo_decode': '(grids, anchors_table, nclasses)',
    'yolo_decode_scores': '(grids, anchors_table, nclasses)',
    'yolo_loss': f"(grids, anchors_table, nclasses: 'int', gt_boxes: {_T}, gt_classes: {_T}, cells: {_T}, loss: {_OT} = None)",
}

_FWD = f"(self, images: {_T}, out: 'Optional[Sequence[torch.Tensor]]' = None) -> 'List[torch.Tensor]'"
_SLOT_S = "(self, slot: 'int', S: 'int')"
_SLOT_TILE = "(self, slot: 'int', tile: 'int')"
_SLOT_INT = "(self, slot: 'int') -> 'int'"
_READ = f"(self, tensor_id: 'int', batch: 'int') -> {_T}"

NET_METHODS = {
    '__call__': _FWD,
    '__init__': "(self, program: 'Program')",
    'act_scales': "(self) -> 'List[float]'",
    'border_skip': "(self, slot: 'int', batch: 'int') -> 'int'",
    'calibrate_i8': f"(self, images: {_T}, percentile: 'float' = 100.0) -> 'List[float]'",
    'conv_signature': "(o: 'ConvOp', image_size) -> 'str'",
    'detect': f"(self, images: {_T}, anchors, max_boxes: 'int', iou_threshold: 'float', score_threshold: 'float')",
    'detect_stream': f"(self, batches, anchors, max_boxes: 'int', iou_threshold: 'float', score_threshold: 'float', mode=1, depth: 'int' = 2, "
                     f"max_batch: {_OI} = None, max_blob_bytes: {_OI} = None, letterbox=False)",
    'evaluate_stream': f"(self, batches, gts, anchors, max_boxes: 'int', iou_threshold: 'float', score_thresholds, nclasses: 'int', "
                       f"evaluate_iou_threshold: 'float' = 0.5, one_class=False, mode=1, depth: 'int' = 2, max_batch: {_OI} = None, "
                       f"max_blob_bytes: {_OI} = None, letterbox=False, max_gt: {_OI} = None, loss=False, ap=None)",
    'flops_per_image': "(self) -> 'float'",
    'forward': _FWD,
    'forward_decode': f"(self, images: {_T}, anchors)",
    'grid_sizes': '(self, image_size=None)',
    'i8_first_conv': "(self) -> 'int'",
    'keep_activations': '(self, keep=True)',
    'load_calibration': "(self, path: 'str')",
    'load_weights': "(self, weights: 'Dict[str, np.ndarray]', eps: 'float' = 0.001)",
    'measure_sclk': f"(self, images: {_T}, out: 'Sequence[torch.Tensor]', forwards: 'int' = 30, conv: 'int' = -1) -> 'float'",
    'measure_sclk_all': f"(self, images: {_T}, out: 'Sequence[torch.Tensor]', forwards: 'int' = 30)",
    'plan': f"(self, max_batch: 'int', image_size, dtype: {_OI} = None)",
    'profile_convs': f"(self, images: {_T}) -> 'np.ndarray'",
    'read_tensor': _READ,
    'read_tensor_i8': _READ,
    'save_calibration': "(self, path: 'str')",
    'set_act_scales': '(self, scales)',
    'set_border_skip': "(self, mode: 'int')",
    'set_dtype': '(self, dtype)',
    'set_early_chunk': "(self, n_convs: 'int', chunk_images: 'int')",
    'set_k_chunk': "(self, channels: 'int')",
    'set_lanes': "(self, lanes: 'int')",
    'set_low_latency': '(self, on=True)',
    'set_low_latency_bf16': '(self, on=True)',
    'set_low_latency_f16': '(self, on=True)',
    'set_low_latency_i8': '(self, on=True)',
    'set_split_k': _SLOT_S,
    'set_split_k_bf16': _SLOT_S,
    'set_split_k_f16': _SLOT_S,
    'set_split_k_i8': _SLOT_S,
    'set_stem_fusion': '(self, on)',
    'set_stem_fusion_f16': '(self, on=True)',
    'set_tile': _SLOT_TILE,
    'set_tile_bf16': _SLOT_TILE,
    'set_tile_x2': _SLOT_TILE,
    'set_tile_x3': _SLOT_TILE,
    'set_xcd_mode': "(self, mode: 'int')",
    'split_k': _SLOT_INT,
    'split_k_bf16': _SLOT_INT,
    'split_k_f16': _SLOT_INT,
    'split_k_i8': _SLOT_INT,
}
# the argument checks core/parse_model.py and tools/hash_outputs.py borrow from Net
NET_ARG_CHECKS = {'_low_latency_arg': "(on) -> 'bool'", '_stem_fusion_arg': "(on) -> 'int'", '_dtype_arg': "(dtype) -> 'int'"}

INPUTSTAGE_METHODS = {
    '__init__': "(self, image_size, max_batch: 'int', max_blob_bytes: 'int', depth: 'int' = 2)",
    'release': "(self, handle: 'StagedBatch')",
    'submit': "(self, images, mode, letterbox=False) -> 'StagedBatch'",
}
STAGEDBATCH_METHODS = {'__init__': '(self, slot, batch, ready, geometry)'}

# what had no docstring when the literals were taken; everything else has one and keeps one
UNDOCUMENTED = {'check', 'class_scores', 'Net.__init__', 'Net.conv_signature', 'Net.flops_per_image', 'Net.keep_activations',
                'Net.load_weights', 'Net.profile_convs', 'Net.read_tensor', 'Net.set_lanes', 'Net.set_tile', 'Net.set_tile_x2',
                'Net.set_tile_x3', 'InputStage.__init__', 'InputStage.submit', 'StagedBatch.__init__'}

CLASSES = {"Net": NET_METHODS, "InputStage": INPUTSTAGE_METHODS, "StagedBatch": STAGEDBATCH_METHODS}


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    return runtime


def _methods(cls):
    out = {}
    for name, v in vars(cls).items():
        f = v.__func__ if isinstance(v, (staticmethod, classmethod)) else v
        if inspect.isfunction(f) and (not name.startswith("_") or name in ("__init__", "__call__")):
            out[name] = f
    return out


def test_public_names(rt):
    public = {n for n in dir(rt) if not n.startswith("_")}
    assert set(NAMES) <= public, sorted(set(NAMES) - public)
    assert public - set(NAMES) <= LEAKED, sorted(public - set(NAMES) - LEAKED)
    assert sorted(n for n in NAMES if inspect.isfunction(getattr(rt, n))) == sorted(FUNCTIONS)
    for n in ("Net", "InputStage", "StagedBatch", "Y3Error"):
        assert inspect.isclass(getattr(rt, n)), n
    assert issubclass(rt.Y3Error, RuntimeError)


@pytest.mark.parametrize("name", sorted(FUNCTIONS))
def test_function_signature_and_docstring(rt, name):
    f = getattr(rt, name)
    assert str(inspect.signature(f)) == FUNCTIONS[name]
    assert name in UNDOCUMENTED or (f.__doc__ or "").strip(), f"{name} lost its docstring"


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_class_methods_signatures_and_docstrings(rt, cls):
    c, want = getattr(rt, cls), CLASSES[cls]
    have = _methods(c)
    assert sorted(have) == sorted(want)
    assert (c.__doc__ or "").strip(), f"{cls} lost its docstring"
    for name, f in have.items():
        assert str(inspect.signature(f)) == want[name], f"{cls}.{name}"
        assert f"{cls}.{name}" in UNDOCUMENTED or (f.__doc__ or "").strip(), f"{cls}.{name} lost its docstring"


def test_net_argument_checks_stay_reachable(rt):
    for name, sig in NET_ARG_CHECKS.items():
        assert isinstance(inspect.getattr_static(rt.Net, name), staticmethod), name
        assert str(inspect.signature(getattr(rt.Net, name))) == sig, name
    assert rt.Net._low_latency_arg(None) is False and rt.Net._stem_fusion_arg(None) == 0 and rt.Net._dtype_arg(None) == 0
