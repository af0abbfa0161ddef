"""Multi-label detections on the host (no GPU): the NumPy restatement multilabel.candidates_ref against a brute-force loop; the
consequences that tie the rule to the single-label path, and through it to the oracle; a product tie built by hand; the one-pass
property under both NMS rules; truncation; the argument checks of the C entry points that need no device; the Python surface, the
YAML keys and the command-line flags.  Every comparison is exact."""
import inspect
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import multilabel_cases as MC
from yolo_v3_tf2_amd.core.yolo_decode_layer import yolo_decode_hw_host
from yolo_v3_tf2_amd.multilabel import candidates_ref, detect_multi_label_ref, pack_candidates_ref, rows_above
from yolo_v3_tf2_amd.nms_per_class import nms_padded_per_class_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _decoded(hw, nc, B, seed=0):
    return yolo_decode_hw_host(MC.random_grids(hw, nc, B, seed), MC.anchors_table(), nc)


def _brute(bboxes, conf, probs, S, K):
    B, N, nc = probs.shape
    out = (np.zeros((B, K, 4), f32), np.zeros((B, K), np.int64), np.zeros((B, K), f32), np.zeros((B, K), np.int32), np.zeros(B, np.int32))
    for b in range(B):
        k = 0
        for n in range(N):
            for c in range(nc):
                score = f32(f32(conf[b, n, 0]) * f32(probs[b, n, c]))
                if score > f32(S):
                    if k < K:
                        out[0][b, k], out[1][b, k], out[2][b, k], out[3][b, k] = bboxes[b, n], c, score, n
                    k += 1
        out[4][b] = k
    return out


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(g.view(np.int32) if g.dtype == np.float32 else g, w.view(np.int32) if w.dtype == np.float32 else w)


@pytest.mark.parametrize("nc", [1, 3, 5, 81])
def test_restatement_equals_brute_force(nc):
    dec = _decoded(MC.SQUARE, nc, 3)
    total = candidates_ref(*dec, MC.S_RANDOM, 1)[4]
    assert (total > 1).all() and (total < MC.boxes_per_image(MC.SQUARE) * nc).all()
    for S, K in ((MC.S_RANDOM, int(total.max())), (MC.S_RANDOM, int(total.min()) - 1), (MC.S_RANDOM, 1), (-1.0, 100), (0.9, 7)):
        _same(candidates_ref(*dec, S, K), _brute(*dec, S, K))
    with pytest.raises(ValueError):
        candidates_ref(*dec, 0.1, 0)


def test_nan_scores_and_negative_thresholds():
    bb, conf, probs = (a.copy() for a in _decoded(MC.SQUARE, 5, 2))
    conf[0, 3], probs[1, 7, 2], probs[0, 9, 4] = np.nan, np.nan, np.inf
    every = MC.boxes_per_image(MC.SQUARE) * 5
    got = candidates_ref(bb, conf, probs, -1.0, every)
    _same(got, _brute(bb, conf, probs, -1.0, every))
    assert got[4].tolist() == [every - 5, every - 1] and not np.isnan(got[2]).any()


# ------------------------------------------------------------------------------------------------ the consequences
@pytest.mark.parametrize("shape", sorted(MC.GRIDS))
def test_every_box_keeps_its_single_label_score(shape):
    """K >= total: box n has a candidate iff its single-label score (the oracle's conf * max prob) is > S; its largest candidate score
    equals that score bit for bit (fp32 multiplication by conf >= 0 is monotone); the class of that candidate is the arg-max class
    unless two products tie -- then it is the lowest class among the tied, which may differ.  Such boxes are counted apart."""
    hw, nc, B = MC.GRIDS[shape], 80, 3
    bb, conf, probs = _decoded(hw, nc, B)
    _, cls, scores, _, _ = O.yolo_nms((bb, conf, probs), 10, 0.5, MC.S_RANDOM)
    N = MC.boxes_per_image(hw)
    cand = candidates_ref(bb, conf, probs, MC.S_RANDOM, N * nc)
    ties = multi = 0
    for b in range(B):
        t = cand[4][b]
        src, ccls, csc = cand[3][b, :t], cand[1][b, :t], cand[2][b, :t]
        assert np.array_equal(np.unique(src), np.flatnonzero(scores[b] > f32(MC.S_RANDOM)))
        for n in np.unique(src):
            mine = src == n
            multi += mine.sum() >= 2
            assert csc[mine].max().view(np.int32) == scores[b, n].view(np.int32)
            first = ccls[mine][np.argmax(csc[mine])]
            if first != cls[b, n]:
                ties += 1
                assert first < cls[b, n]
    assert multi > 50, "many boxes carry two or more labels on these inputs"
    print(f"{shape}: {multi} boxes with two or more labels, {ties} whose largest product ties with a lower class than the arg-max")


def test_product_tie():
    """Two classes whose products with conf round to the same fp32 although the probabilities differ (tests/multilabel_cases.py: found
    once by search over random fp32 triples).  arg-max says the class of the larger probability; the largest candidate is the lower
    class of the tied pair.  Both are candidates, in class order, with the same score bits."""
    c, lo, hi = f32(MC.TIE_CONF), f32(MC.TIE_P_LO), f32(MC.TIE_P_HI)
    assert lo < hi and f32(c * lo) == f32(c * hi)
    bb = np.array([[[0.1, 0.2, 0.3, 0.4]]], f32)
    conf, probs = np.array([[[c]]], f32), np.array([[[0.01, lo, hi, 0.02]]], f32)
    _, cls, scores, _, _ = O.yolo_nms((bb, conf, probs), 10, 0.5, 0.1)
    assert cls[0, 0] == 2 and scores[0, 0] == f32(c * hi)
    cand = candidates_ref(bb, conf, probs, 0.1, 4)
    assert cand[4][0] == 2 and cand[1][0, :2].tolist() == [1, 2] and cand[2][0, 0].view(np.int32) == cand[2][0, 1].view(np.int32)
    assert cand[1][0][np.argmax(cand[2][0])] == 1 != cls[0, 0]
    packed, nv, _ = detect_multi_label_ref(bb, conf, probs, 0.1, 4, 10, 0.5)        # per class: both labels survive, the tie by index
    assert nv[0] == 2 and packed[0, :2, 5].tolist() == [1, 2] and packed[0, :2, 6].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ one pass
THRESHOLDS = [0.1, 0.15, 0.2, 0.3, 0.5, 0.7, 0.9]


@pytest.mark.parametrize("per_class", [True, False])
def test_one_pass_serves_every_threshold(per_class):
    """total <= K at the lowest threshold: the candidates at S' > S are the candidates at S with score > S' in the same order, the
    padded NMS never lets a row be affected by a row scored below it, so the detections at S' are the rows with score > S' of the
    detections at S -- with max_boxes binding (M = 10) and not (M = 1024), under both NMS rules (the agnostic one: the C oracle's)."""
    hw, nc, B = MC.RECT, 5, 3
    bb, conf, probs = _decoded(hw, nc, B, seed=3)
    K = MC.boxes_per_image(hw) * nc
    low_cand = candidates_ref(bb, conf, probs, THRESHOLDS[0], K)
    for M in (10, 1024):
        low = detect_multi_label_ref(bb, conf, probs, THRESHOLDS[0], K, M, 0.5, per_class, O.nms_padded)
        assert (low[1] == 10).all() if M == 10 else (low[1] > 10).all() and (low[1] < low[2]).all()
        counts = []
        for t in THRESHOLDS:
            cand = candidates_ref(bb, conf, probs, t, K)
            for b in range(B):
                keep = low_cand[2][b, :low_cand[4][b]] > f32(t)
                assert cand[4][b] == keep.sum()
                for i in range(4):
                    assert np.array_equal(cand[i][b, :cand[4][b]], low_cand[i][b, :low_cand[4][b]][keep])
            got = detect_multi_label_ref(bb, conf, probs, t, K, M, 0.5, per_class, O.nms_padded)
            want = rows_above(low[0], low[1], t)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), (M, t)
            counts.append(int(got[1].sum()))
        assert counts[-1] > 0 and (M == 10 or counts[0] > counts[-1])
    if per_class:       # two rows of an image share their box: what the single-label rule cannot return
        rows = low[0][0, :low[1][0], 6]
        assert len(set(rows.tolist())) < len(rows)


def test_truncation():
    """K = total - 1, total, total + 1 and K = 1: the stored candidates are the first min(total, K) of the full list, total is uncapped;
    a truncated image breaks the one-pass property, which is why evaluate_stream refuses it."""
    hw, nc = MC.SQUARE, 5
    bb, conf, probs = _decoded(hw, nc, 1, seed=5)
    full = candidates_ref(bb, conf, probs, MC.S_RANDOM, MC.boxes_per_image(hw) * nc)
    total = int(full[4][0])
    for K in (total - 1, total, total + 1, 1):
        got = candidates_ref(bb, conf, probs, MC.S_RANDOM, K)
        assert got[4][0] == total
        m = min(total, K)
        for i in range(4):
            assert np.array_equal(got[i][0, :m], full[i][0, :m]) and not got[i][0, m:].any()
    K = total // 2       # the one-pass property fails: a candidate above S' behind the cut is missing from the pass at S
    low = detect_multi_label_ref(bb, conf, probs, MC.S_RANDOM, K, 1024, 0.5)
    high = detect_multi_label_ref(bb, conf, probs, 0.5, K, 1024, 0.5)
    assert low[2][0] > K and not np.array_equal(rows_above(low[0], low[1], 0.5)[0], high[0])


def test_rider_and_horse_share_a_box():
    """README's argument one step earlier: ONE box that is the best 'person' and the best 'horse' box.  Single-label gives it one of
    the two labels; multi-label with per-class NMS returns both, and the second class gets its AP."""
    from yolo_v3_tf2_amd.evaluate_detections import average_precision, match_detections
    gt = np.array([[0.20, 0.20, 0.60, 0.80]], f32)
    bb = gt[None]
    conf = np.array([[[0.9]]], f32)
    probs = np.zeros((1, 1, 80), f32)
    probs[0, 0, 0], probs[0, 0, 17] = 0.8, 0.7
    packed, nv, totals = detect_multi_label_ref(bb, conf, probs, 0.1, 1 * 80, 100, 0.5)
    assert totals[0] == 2 and nv[0] == 2 and packed[0, :2, 5].tolist() == [0, 17] and packed[0, :2, 6].tolist() == [0, 0]
    gt2, cls2 = np.repeat(gt, 2, 0)[None], np.array([[0, 17]], np.int32)
    rec, tot = match_detections(packed, nv, gt2, cls2, [2], 80, [0.5])
    assert average_precision(rec, tot, 80, 1)["mAP"] == 1.0
    _, cls, scores, sel, n1 = O.yolo_nms((bb, conf, probs), 100, 0.5, 0.1)
    single = pack_candidates_ref((bb, cls, scores, np.zeros((1, 1), np.int32), None), sel, n1)
    rec, tot = match_detections(single, n1, gt2, cls2, [2], 80, [0.5])
    assert n1[0] == 1 and average_precision(rec, tot, 80, 1)["mAP"] == 0.5


# ------------------------------------------------------------------------------------------------ the surface
def test_python_surface():
    from yolo_v3_tf2_amd import _lib, ops, runtime
    from yolo_v3_tf2_amd.core import yolo_nms
    for name in ("multi_label", "multi_label_capacity", "multi_label_totals"):
        prop = inspect.getattr_static(runtime.Net, name)
        assert isinstance(prop, property) and (prop.__doc__ or "").strip()
    assert runtime.Net.multi_label.fset is not None and runtime.Net.multi_label_capacity.fset is not None
    assert runtime.Net.multi_label_totals.fset is None
    assert str(inspect.signature(ops.decode_candidates)) == "(grids, anchors_table, nclasses, score_threshold, capacity, out=None, ws=None)"
    assert not hasattr(runtime, "decode_candidates") and not hasattr(runtime, "multilabel")
    assert list(inspect.signature(yolo_nms.yolo_nms_multi_label).parameters)[:5] == \
        ["outputs", "yolo_max_boxes", "nms_iou_threshold", "nms_score_threshold", "capacity"]
    for name in ("y3_decode_candidates_workspace_bytes", "y3_yolo_decode_candidates_hw", "y3_class_candidates", "y3_candidate_sources",
                 "y3_net_set_multi_label", "y3_net_get_multi_label", "y3_net_get_multi_label_capacity", "y3_net_read_multi_label_totals"):
        assert name in _lib.SYMBOLS


def test_abi_without_compute():
    """The workspace size and the argument checks that need no device: every refusal comes before the first launch."""
    import ctypes as C
    from yolo_v3_tf2_amd import _lib
    lib = _lib.load()
    gs = (C.c_int32 * 6)(13, 13, 26, 26, 52, 52)
    assert lib.y3_decode_candidates_workspace_bytes(gs, 64, 80) == 64 * 10647 * 4
    assert lib.y3_decode_candidates_workspace_bytes(gs, 0, 80) == 0 and lib.y3_decode_candidates_workspace_bytes(None, 1, 80) == 0
    assert lib.y3_decode_candidates_workspace_bytes((C.c_int32 * 6)(13, 13, 0, 26, 52, 52), 1, 80) == 0
    fake = C.c_void_p(4096)       # never dereferenced: each call below is refused by an earlier check
    grids = (C.c_void_p * 3)(4096, 4096, 4096)
    a = np.zeros(18, f32).ctypes.data_as(C.POINTER(C.c_float))

    def call(grids=grids, gs=gs, B=1, nc=80, a=a, K=10, boxes=fake, ws=fake, ws_bytes=1 << 30):
        return lib.y3_yolo_decode_candidates_hw(grids, gs, B, nc, a, 0.1, K, boxes, fake, fake, fake, fake, ws, ws_bytes, None)

    for kw, word in ((dict(grids=None), b"null pointer"), (dict(boxes=None), b"null pointer"), (dict(B=0), b"at least 1"),
                     (dict(K=0), b"at least 1"), (dict(nc=0), b"at least 1"), (dict(B=3, K=2**30), b"below 2^31"),
                     (dict(gs=(C.c_int32 * 6)(13, 13, 26, 26, 20000, 20000)), b"below 2^31"), (dict(nc=641), b"LDS"),
                     (dict(boxes=C.c_void_p(4100)), b"16-byte aligned"), (dict(grids=(C.c_void_p * 3)(4100, 4096, 4096)), b"16-byte aligned"),
                     (dict(ws=None), b"workspace too small"), (dict(ws_bytes=10647 * 4 - 1), b"workspace too small")):
        assert call(**kw) == _lib.Y3_ERR_INVALID, kw
        msg = lib.y3_last_error()
        assert b"y3_yolo_decode_candidates_hw" in msg and word in msg, (kw, msg)
    assert lib.y3_candidate_sources(None, None, None, 1, 1, 1, None) == _lib.Y3_ERR_INVALID and b"y3_candidate_sources" in lib.y3_last_error()
    assert lib.y3_candidate_sources(fake, fake, fake, 1, 0, 1, None) == _lib.Y3_ERR_INVALID
    assert lib.y3_class_candidates(None, None, None, 1, 1, 1, 0.1, 1, None, None, None, None, None, None, 0, None) == _lib.Y3_ERR_INVALID
    assert b"y3_class_candidates" in lib.y3_last_error()
    assert lib.y3_net_set_multi_label(None, 1, 0) == _lib.Y3_ERR_INVALID and b"y3_net_set_multi_label" in lib.y3_last_error()
    assert lib.y3_net_get_multi_label(None) == 0 and lib.y3_net_get_multi_label_capacity(None) == 0
    assert lib.y3_net_read_multi_label_totals(None, 1, None, None) == _lib.Y3_ERR_INVALID


def test_yolo_nms_layer_takes_multi_label(monkeypatch):
    from yolo_v3_tf2_amd.core import yolo_nms_layer as m
    calls = []
    monkeypatch.setattr(m, "yolo_nms", lambda *a: calls.append(("agnostic",) + a[1:]) or "a")
    monkeypatch.setattr(m, "yolo_nms_multi_label", lambda *a: calls.append(("multi",) + a[1:]) or "m")
    layer = m.YoloNmsLayer(100, 0.5, 0.1)
    assert layer.multi_label is False and layer.multi_label_capacity == 0 and layer(None) == "a"
    layer = m.YoloNmsLayer(50, 0.4, 0.2, multi_label=True, multi_label_capacity=300, per_class=True)
    assert layer.multi_label is True and layer(None) == "m"
    assert calls == [("agnostic", 100, 0.5, 0.1), ("multi", 50, 0.4, 0.2, 300, True)]


def test_model_switch():
    """YoloModel.set_multi_label beside the other switches (no device net is made here); DetectModel reads it per call."""
    from yolo_v3_tf2_amd.core.parse_model import YoloModel
    model = YoloModel(program=None)
    assert model.multi_label is False and model.multi_label_capacity == 0
    model.set_multi_label()
    assert model.multi_label is True and model.multi_label_capacity == 0
    model.set_multi_label(True, 500)
    assert (model.multi_label, model.multi_label_capacity) == (True, 500)
    for off in (False, None):
        model.set_multi_label(off)
        assert model.multi_label is False
    for bad in ((1, 0), (True, -1), (True, 2.5), (True, True)):
        with pytest.raises(TypeError):
            model.set_multi_label(*bad)


def test_yaml_keys_and_command_line_flags(tmp_path, monkeypatch):
    import yaml
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev, inference
    seen = {}
    assert "multi_label" not in inspect.signature(inference.Inference.__call__).parameters
    monkeypatch.setattr(inference.Inference, "__call__",
                        lambda self, **kw: seen.update(on=self.multi_label, capacity=self.multi_label_capacity, kw=kw))
    for text, want in (("multi_label: true\nmulti_label_capacity: 300\nbatch_size: 2\n", (True, 300)), ("batch_size: 2\n", (None, 0)),
                       ("multi_label: false\nbatch_size: 2\n", (False, 0))):
        path = tmp_path / "detect.yaml"
        path.write_text(text)
        inference.main(["--config", str(path)])
        assert (seen["on"], seen["capacity"]) == want and seen["kw"] == {"batch_size": 2}
    assert inference.Inference.multi_label is None and inference.Inference.multi_label_capacity == 0
    for name in ("detect_config_coco.yaml", "evaluate_config.yaml"):      # the packaged files stay as they are
        assert "multi_label" not in yaml.safe_load(open(os.path.join(ROOT, "config", name)))
    # evaluate_yolov3: the flags, the keys of either config, and the host route's refusal
    parser = ev._arg_parser()
    args = parser.parse_args(["--on-device", "--multi-label", "--multi-label-capacity", "400"])
    assert parser.parse_args([]).multi_label is False and args.multi_label is True and args.multi_label_capacity == 400
    params = inspect.signature(ev.evaluate).parameters
    assert params["multi_label"].default is False and params["multi_label_capacity"].default == 0
    with pytest.raises(ValueError, match="multi_label needs on_device=True"):
        ev.evaluate({"multi_label": True}, [0.1])
    with pytest.raises(ValueError, match="multi_label needs on_device=True"):
        ev.evaluate({}, [0.1], multi_label=True)
    with pytest.raises(SystemExit):
        ev.main(["--multi-label"])
    got = []
    monkeypatch.setattr(ev, "evaluate", lambda cfg, thr, **kw: got.append((kw["multi_label"], kw["multi_label_capacity"])) or [])
    detect, evaluate = tmp_path / "d.yaml", tmp_path / "e.yaml"
    detect.write_text("batch_size: 2\n")
    base = "evaluate_nms_score_thresholds: [0.1]\n"
    for text, argv, want in ((base, ["--on-device"], (False, 0)), (base, ["--on-device", "--multi-label"], (True, 0)),
                             (base, ["--on-device", "--multi-label", "--multi-label-capacity", "9"], (True, 9)),
                             (base + "multi_label: true\nmulti_label_capacity: 70\n", ["--on-device"], (True, 70))):
        evaluate.write_text(text)
        ev.main(["--config", str(detect), "--evaluate-config", str(evaluate)] + argv)
        assert got[-1] == want


def test_on_device_evaluate_sets_the_model_switch(monkeypatch):
    """_evaluate_on_device up to 'the model's switch is set': create_model is replaced by a stand-in that records the calls."""
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev

    class Stop(Exception):
        pass

    calls = []

    class Model:
        def __getattr__(self, name):
            if name == "_device_net":
                raise Stop
            return lambda *a: calls.append((name,) + a)

    class Detect:
        model = Model()

    monkeypatch.setattr(ev, "create_model", lambda *a: Detect())
    cfg = dict(image_size=64, batch_size=2, model_config_file="", nms_iou_threshold=0.5, yolo_max_boxes=100)
    with pytest.raises(Stop):
        ev._evaluate_on_device(cfg, [0.1], 0.5, 1, None, True, MC.anchors_table(), 80, multi_label=True, multi_label_capacity=321)
    assert ("set_multi_label", True, 321) in calls
