"""Per-class NMS on the host (no GPU): the NumPy restatement nms_per_class.nms_padded_per_class_ref -- what the device is held to
in tests/test_nms_per_class_gpu.py -- against a brute-force loop written here, against the C oracle through the two consequences
of the rule (all ids equal: the agnostic result; any ids: the merge of per-class agnostic runs), the score-threshold prefix
property the one-pass evaluation rests on, what the rule does to AP, and the Python surface.  Every comparison is exact."""
import inspect
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import nms_edge_cases as C
from tests import nms_per_class_cases as P
from tests.helpers import nms_stress_set
from yolo_v3_tf2_amd.nms_per_class import nms_padded_per_class_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _brute_force(boxes, scores, classes, M, T, S):
    """The rule, one scalar fp32 operation at a time, nothing shared with the restatement: every box keeps its place (masked ones
    become zero boxes with score 0 * s), Python's sort on (-score, index), a flat list of kept boxes."""
    B, N = scores.shape
    sel, nv = np.zeros((B, M), np.int32), np.zeros(B, np.int32)
    mask = lambda b, i: f32(1.0) if scores[b, i] > f32(S) else f32(0.0)
    b00 = [boxes[0, 0, k] * mask(0, 0) for k in range(4)]
    swap_y, swap_x = not (b00[0] <= b00[2]), not (b00[1] <= b00[3])

    def iou(a, b):
        i_xmin, i_xmax = max(a[1], b[1]), min(a[3], b[3])
        i_ymin, i_ymax = max(a[0], b[0]), min(a[2], b[2])
        i_area = f32(max(f32(i_xmax - i_xmin), f32(0))) * f32(max(f32(i_ymax - i_ymin), f32(0)))
        a_area = f32(f32(a[2] - a[0]) * f32(a[3] - a[1]))
        b_area = f32(f32(b[2] - b[0]) * f32(b[3] - b[1]))
        u_area = f32(f32(f32(a_area + b_area) - i_area) + f32(1e-8))
        return f32(i_area / u_area)

    for b in range(B):
        rows = []
        for i in range(N):
            m = mask(b, i)
            y1, x1, y2, x2 = (f32(v * m) for v in boxes[b, i])
            if swap_y:
                y1, y2 = y2, y1
            if swap_x:
                x1, x2 = x2, x1
            rows.append((-(float(f32(scores[b, i] * m)) + 0.0), i, (y1, x1, y2, x2), int(classes[b, i])))
        rows.sort(key=lambda r: r[:2])
        kept, n = [], 0
        for _, i, box, c in rows:
            if n == M:
                break
            if any(kc == c and iou(kb, box) >= f32(T) for kb, kc in kept):
                continue
            kept.append((box, c))
            if any(v > 0 for v in box):
                sel[b, n] = i
                n += 1
        nv[b] = n
    return sel, nv


def _same(got, want):
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert np.array_equal(got[0], want[0]), int((got[0] != want[0]).sum())


@pytest.mark.parametrize("ncls", [1, 3, 80])
def test_restatement_equals_brute_force(ncls):
    """300 stress-set boxes (exact duplicates, tied scores) per image; positive and negative S, a flipped box [0,0], M reached and not."""
    boxes, scores = nms_stress_set(np.random.default_rng(40 + ncls), 2, 300, dup_frac=0.1)
    classes = P.random_ids(ncls, scores.shape, ncls)
    flipped = boxes.copy()
    flipped[0, 0] = flipped[0, 0, [2, 3, 0, 1]]
    flipped_scores = scores.copy()
    flipped_scores[0, 0] = 0.9
    differs = 0
    for bx, sc, M, T, S in ((boxes, scores, 100, 0.5, 0.1), (boxes, scores, 40, 0.3, -1.0), (flipped, flipped_scores, 300, 0.5, 0.05),
                            (boxes, (scores - f32(0.2)).astype(f32), 300, 0.6, -0.1)):
        want = _brute_force(bx, sc, classes, M, T, S)
        _same(nms_padded_per_class_ref(bx, sc, classes, M, T, S), want)
        assert want[1].min() > 10
        differs += not np.array_equal(want[0], O.nms_padded(bx, sc, M, T, S)[0])
    assert (differs == 0) if ncls == 1 else (differs > 0), "with several classes the rule is not the agnostic one on these inputs"


def _one_class(case):
    boxes, scores, M, T, S = case
    for cid in (0, 79):
        _same(nms_padded_per_class_ref(boxes, scores, np.full(scores.shape, cid, np.int64), M, T, S), O.nms_padded(boxes, scores, M, T, S))


@pytest.mark.parametrize("name", C.CANONICAL + C.SCORES)
def test_one_class_is_the_agnostic_rule_on_the_canonical_and_score_cases(name):
    _one_class(C.canonical_case(name) if name in C.CANONICAL else C.score_case(name))


@pytest.mark.parametrize("nc", C.CANDIDATE_COUNTS)
def test_one_class_is_the_agnostic_rule_on_the_candidate_counts(nc):
    _one_class(C.count_case(nc))


@pytest.mark.parametrize("M", C.M_VALUES)
def test_one_class_is_the_agnostic_rule_where_M_is_reached(M):
    for k in (M - 1, M, M + 1):
        _one_class(C.lattice_case(M, k))


@pytest.mark.parametrize("ncls,M,S", [(1, 100, 0.1), (7, 1024, 0.1), (80, 100, -1.0), (3, 1024, -1.0)])
def test_restatement_equals_the_merge_of_per_class_oracle_runs(ncls, M, S):
    boxes, scores = nms_stress_set(np.random.default_rng(9), 2, 3000)
    classes = P.random_ids(90 + ncls, scores.shape, ncls)
    want = P.merge_of_agnostic_runs(O.nms_padded, boxes, scores, classes, M, 0.5, S)
    _same(nms_padded_per_class_ref(boxes, scores, classes, M, 0.5, S), want)
    assert want[1].min() >= min(M, 100)


def test_the_constructed_cases_say_what_they_claim():
    """The duplicates and the kept-list spill of tests/nms_per_class_cases.py, on the restatement."""
    case, missing = P.duplicates_case()
    sel, nv = nms_padded_per_class_ref(*case)
    want = [i for i in range(600) if i not in missing]
    assert nv.tolist() == [598, 598] and sel[0, :598].tolist() == want and sel[1, :598].tolist() == want
    agnostic = O.nms_padded(*case[:2], *case[3:])
    assert agnostic[1].tolist() == [596, 596]
    case, at, origin, selected = P.spill_case()
    # where the kernel meets each pair: a probe lies in a later chunk than the box it rests on, so only the kept-list pass sees it
    chunk = lambda i: i // P.CHUNK
    assert {k: (chunk(at[k]), chunk(origin[k])) for k in at} == {"D1": (11, 8), "D2": (11, 8), "P1": (11, 8), "P2": (11, 8), "P4": (11, 0),
                                                                 "P5": (11, 0), "P3": (12, 8)}
    assert chunk(at["P3"]) > chunk(at["D2"]) and all(origin[k] >= P.KEPT_CAP for k in ("D1", "D2", "P1", "P2", "P3"))
    sel, nv = nms_padded_per_class_ref(*case)
    assert nv.tolist() == [len(selected)] * 2
    assert sel[0, :nv[0]].tolist() == selected and sel[1, :nv[1]].tolist() == selected
    assert {at["P2"], at["P5"]} <= set(selected) and not {at["P1"], at["P3"], at["P4"]} & set(selected)
    # ... and the case tells a kernel with a broken class test on the spilled branch from a right one
    assert _chunked(case, None) == selected
    assert at["P2"] not in _chunked(case, True), "every spilled id taken as equal: P2 is lost"
    assert {at["P1"], at["P3"]} <= set(_chunked(case, False)), "no spilled id taken as equal: P1 and P3 come through"


def _chunked(case, spilled_equal):
    """Image 0 of a case whose sorted position is its index, walked as nms_kernel walks it: a kept box of an EARLIER chunk whose slot is
    >= KEPT_CAP is met on the spilled branch of the kept-list pass, where `spilled_equal` (None: the rule) replaces the class test."""
    from yolo_v3_tf2_amd.nms_per_class import iou_tf
    boxes, scores, classes, M, T, S = case
    assert (np.diff(scores[0]) < 0).all() and scores[0].min() > S
    kept, out = [], []                                  # kept: sorted positions, the list index being the slot
    for j in range(scores.shape[1]):
        if len(out) == M:
            break
        slots = np.arange(len(kept))
        pos = np.asarray(kept, np.int64)
        equal = classes[0, pos] == classes[0, j]
        if spilled_equal is not None:
            equal = np.where((slots >= P.KEPT_CAP) & (pos // P.CHUNK < j // P.CHUNK), spilled_equal, equal)
        if equal.any() and (iou_tf(boxes[0, pos[equal]], boxes[0, j]) >= f32(T)).any():
            continue
        kept.append(j)
        if (boxes[0, j] > 0).any():
            out.append(j)
    return out


def test_detections_at_a_higher_score_threshold_are_a_prefix_of_the_lowest():
    """What evaluate_stream's one pass rests on, under the per-class rule: a box is never affected by a box scored below it, so the
    detections at threshold t are the rows with score > t of the lowest threshold's detections, in the same order."""
    boxes, scores = nms_stress_set(np.random.default_rng(12), 2, 3000)
    classes = P.random_ids(12, scores.shape, 7)
    thresholds = [0.02, 0.05, 0.1, 0.2, 0.4]
    for M in (100, 1024):
        low, low_n = nms_padded_per_class_ref(boxes, scores, classes, M, 0.5, thresholds[0])
        counts = []
        for t in thresholds:
            sel, nv = nms_padded_per_class_ref(boxes, scores, classes, M, 0.5, t)
            for b in range(2):
                rows = low[b, :low_n[b]]
                assert sel[b, :nv[b]].tolist() == rows[scores[b, rows] > f32(t)].tolist(), (M, t, b)
            counts.append(int(nv.sum()))
        assert counts[-1] > 0 and (M == 100 or counts[0] > counts[-1])


def test_per_class_nms_gives_the_second_class_its_ap():
    """A rider on a horse: two ground-truth boxes of different classes with IoU >= T, and detections equal to them.  The agnostic
    rule keeps the higher-scored one, so the other class has AP 0; the per-class rule keeps both and mAP is 1.0."""
    from tests.evaluate_cases import pack_rows
    from yolo_v3_tf2_amd.evaluate_detections import average_precision, match_detections
    gt = np.array([[0.20, 0.20, 0.60, 0.80], [0.22, 0.15, 0.58, 0.70]], f32)      # (xmin, ymin, xmax, ymax)
    gt_classes = np.array([17, 0], np.int32)                                     # horse, person
    tf_boxes = gt[None, :, [1, 0, 3, 2]]                                          # the NMS reads (y1, x1, y2, x2)
    scores, classes = np.array([[0.9, 0.8]], f32), gt_classes[None].astype(np.int64)
    from yolo_v3_tf2_amd.nms_per_class import iou_tf
    assert iou_tf(tf_boxes[0, 0], tf_boxes[0, 1]) >= f32(0.5)

    def mean_ap(sel, nv):
        rows = sel[0, :nv[0]]
        packed = pack_rows(gt[rows], scores[0, rows], gt_classes[rows], 100)[None]
        records, totals = match_detections(packed, nv, gt[None], gt_classes[None], [2], 80, [0.5, 0.75])
        return average_precision(records, totals, 80, 2)

    agnostic = mean_ap(*O.nms_padded(tf_boxes, scores, 100, 0.5, 0.1))
    per_class = mean_ap(*nms_padded_per_class_ref(tf_boxes, scores, classes, 100, 0.5, 0.1))
    assert agnostic["ap"][:, 17].tolist() == [1.0, 1.0] and agnostic["ap"][:, 0].tolist() == [0.0, 0.0] and agnostic["mAP"] == 0.5
    assert per_class["ap"][:, [0, 17]].tolist() == [[1.0, 1.0]] * 2 and per_class["mAP"] == 1.0


def test_restatement_refuses_T_le_0_and_bad_shapes():
    boxes, scores = nms_stress_set(np.random.default_rng(1), 1, 10)
    classes = np.zeros((1, 10), np.int64)
    for T in (0.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="iou_threshold"):
            nms_padded_per_class_ref(boxes, scores, classes, 5, T, 0.1)
    with pytest.raises(ValueError):
        nms_padded_per_class_ref(boxes, scores, classes[:, :9], 5, 0.5, 0.1)


# ------------------------------------------------------------------------------------------------------------------- the surface
def test_python_surface():
    from yolo_v3_tf2_amd import _lib, ops, runtime
    from yolo_v3_tf2_amd.core import yolo_nms
    assert isinstance(inspect.getattr_static(runtime.Net, "nms_per_class"), property)
    assert runtime.Net.nms_per_class.fset is not None and (runtime.Net.nms_per_class.__doc__ or "").strip()
    assert str(inspect.signature(ops.nms_padded_per_class)) == "(bboxes, scores, classes, max_output_size, iou_threshold, score_threshold)"
    assert not hasattr(runtime, "nms_padded_per_class")
    assert str(inspect.signature(yolo_nms.yolo_nms_per_class)) == str(inspect.signature(yolo_nms.yolo_nms))
    assert (_lib.Y3_NMS_AGNOSTIC, _lib.Y3_NMS_PER_CLASS) == (0, 1)
    for name in ("y3_nms_padded_per_class", "y3_nms_per_class_workspace_bytes", "y3_net_set_nms_mode", "y3_net_get_nms_mode"):
        assert name in _lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "y3.h")).read()
    assert "Y3_NMS_AGNOSTIC = 0" in header and "Y3_NMS_PER_CLASS = 1" in header and "[0, 2^31)" in header


def test_abi_without_compute():
    """The workspace sizes and the argument checks that need no device: y3_nms_workspace_bytes keeps its value, the per-class one
    adds batch * n * 4 bytes; T <= 0 and a null class pointer are refused with their message."""
    from yolo_v3_tf2_amd import _lib
    lib = _lib.load()
    assert lib.y3_nms_per_class_workspace_bytes(0, 0) == 0
    for B, N in ((2, 10647), (64, 10647), (1, 1)):
        assert lib.y3_nms_per_class_workspace_bytes(B, N) == lib.y3_nms_workspace_bytes(B, N) + B * N * 4
    assert lib.y3_nms_padded_per_class(None, None, None, 1, 10, 100, 0.5, 0.1, None, None, None, 0, None) == _lib.Y3_ERR_INVALID
    assert b"y3_nms_padded_per_class" in lib.y3_last_error()
    assert lib.y3_net_set_nms_mode(None, 1) == _lib.Y3_ERR_INVALID and lib.y3_net_get_nms_mode(None) == 0


def test_yolo_nms_layer_takes_per_class(monkeypatch):
    from yolo_v3_tf2_amd.core import yolo_nms_layer as m
    calls = []
    monkeypatch.setattr(m, "yolo_nms", lambda *a: calls.append(("agnostic",) + a[1:]) or "a")
    monkeypatch.setattr(m, "yolo_nms_per_class", lambda *a: calls.append(("per_class",) + a[1:]) or "p")
    assert m.YoloNmsLayer(100, 0.5, 0.1).per_class is False and m.YoloNmsLayer(100, 0.5, 0.1, name="x", per_class=False).name == "x"
    assert m.YoloNmsLayer(100, 0.5, 0.1)(None) == "a"
    layer = m.YoloNmsLayer(50, 0.4, 0.2, per_class=True)
    assert layer.per_class is True and layer(None) == "p" and layer.call(None) == "p"
    assert calls == [("agnostic", 100, 0.5, 0.1), ("per_class", 50, 0.4, 0.2), ("per_class", 50, 0.4, 0.2)]


def test_model_switch_and_detect_model_follow_it():
    """YoloModel.set_nms_per_class beside the other switches (no device net is made here); DetectModel reads it per call."""
    from yolo_v3_tf2_amd.core.parse_model import YoloModel
    model = YoloModel(program=None)
    assert model.nms_per_class is False
    model.set_nms_per_class()
    assert model.nms_per_class is True
    for off in (False, None):
        model.set_nms_per_class(off)
        assert model.nms_per_class is False
    with pytest.raises(TypeError):
        model.set_nms_per_class(1)


def test_yaml_key_and_command_line_flag(tmp_path, monkeypatch):
    import yaml
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev, inference
    # inference: popped in main(), kept as an attribute, not a parameter of __call__
    seen = {}
    assert "nms_per_class" not in inspect.signature(inference.Inference.__call__).parameters
    monkeypatch.setattr(inference.Inference, "__call__", lambda self, **kw: seen.update(per_class=self.nms_per_class, kw=kw))
    for text, want in (("nms_per_class: true\nbatch_size: 2\n", True), ("batch_size: 2\n", None), ("nms_per_class: false\nbatch_size: 2\n", False)):
        path = tmp_path / "detect.yaml"
        path.write_text(text)
        inference.main(["--config", str(path)])
        assert seen["per_class"] is want and seen["kw"] == {"batch_size": 2}
    assert inference.Inference.nms_per_class is None
    # the packaged files stay as they are
    for name in ("detect_config_coco.yaml", "evaluate_config.yaml"):
        assert "nms_per_class" not in yaml.safe_load(open(os.path.join(ROOT, "config", name)))
    # evaluate_yolov3: the flag, and the key of either config
    parser = ev._arg_parser()
    assert parser.parse_args([]).nms_per_class is False and parser.parse_args(["--nms-per-class"]).nms_per_class is True
    assert inspect.signature(ev.evaluate).parameters["nms_per_class"].default is False
    got = []
    monkeypatch.setattr(ev, "evaluate", lambda cfg, thr, **kw: got.append(kw["nms_per_class"]) or [])
    detect, evaluate = tmp_path / "d.yaml", tmp_path / "e.yaml"
    detect.write_text("batch_size: 2\n")
    for text, argv, want in (("evaluate_nms_score_thresholds: [0.1]\n", [], False), ("evaluate_nms_score_thresholds: [0.1]\n", ["--nms-per-class"], True),
                             ("evaluate_nms_score_thresholds: [0.1]\nnms_per_class: true\n", [], True)):
        evaluate.write_text(text)
        ev.main(["--config", str(detect), "--evaluate-config", str(evaluate)] + argv)
        assert got[-1] is want
