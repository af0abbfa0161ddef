"""Evaluation sweep, host tier (no GPU): evaluate_detections.sweep_counters against the existing EvaluateDetections class, the
prefix property of the greedy padded NMS that lets one detect pass serve every score threshold, the argument checks of
y3_evaluate_detections, and pack_ground_truth."""
import os

import numpy as np
import pytest

from tests.evaluate_cases import batch_of, recipe, reference_counters, unit_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("preds", "gts", "tp", "fp", "fn")


@pytest.mark.parametrize("case", unit_cases(), ids=lambda c: c[0])
def test_sweep_counters_equals_the_host_class_on_the_unit_cases(case):
    from yolo_v3_tf2_amd.evaluate_detections import counters_from_row, sweep_counters
    name, nc, iou, thresholds, images, want = case
    data = batch_of(images)
    got = sweep_counters(*data, nc, iou, thresholds)
    assert got.dtype == np.int64 and got.shape == (len(thresholds), 5 * nc + 2)
    assert np.array_equal(got, reference_counters(*data, nc, iou, thresholds)), name
    first = counters_from_row(got[0], nc)
    assert sorted(first) == sorted(KEYS + ("errors", "examples"))
    for k, v in want.items():
        assert np.array_equal(first[k], v), (name, k, first[k], v)


def test_one_class_turns_the_error_images_into_counted_ones():
    from yolo_v3_tf2_amd.evaluate_detections import counters_from_row, sweep_counters
    name, nc, iou, thresholds, images, _ = [c for c in unit_cases() if c[0] == "bad ground-truth classes"][0]
    data = batch_of(images)
    plain = counters_from_row(sweep_counters(*data, nc, iou, thresholds)[0], nc)
    one = sweep_counters(*data, nc, iou, thresholds, one_class=True)
    assert np.array_equal(one, reference_counters(*data, nc, iou, thresholds, one_class=True))
    c = counters_from_row(one[0], nc)
    assert (plain["errors"], plain["examples"]) == (2, 1) and (c["errors"], c["examples"]) == (0, 3)
    assert c["tp"].tolist() == [3, 0, 0] and c["gts"].tolist() == [6, 0, 0] and c["fn"].tolist() == [3, 0, 0]
    # the second threshold (0.95) leaves no prediction: everything is a false negative
    c = counters_from_row(one[1], nc)
    assert c["preds"].sum() == 0 and c["fn"].tolist() == [6, 0, 0] and c["examples"] == 3


def test_a_bad_prediction_class_is_an_error_image_at_the_thresholds_that_see_it():
    """EvaluateDetections raises there; sweep_counters (and the kernel) define it: errors += 1 at every threshold whose rows
    hold the class, ordinary counting at the others."""
    from yolo_v3_tf2_amd.evaluate_detections import EvaluateDetections, counters_from_row, sweep_counters
    box = [[.1, .1, .5, .5]]
    data = batch_of([(box * 2, [0.9, 0.4], [1, 7], box, [1])])
    with pytest.raises(IndexError):
        EvaluateDetections(3, 0.5).evaluate(box * 2, [1, 7], box, [1])
    got = sweep_counters(*data, 3, 0.5, [0.1, 0.5])
    low, high = counters_from_row(got[0], 3), counters_from_row(got[1], 3)
    assert (low["errors"], low["examples"], int(low["preds"].sum())) == (1, 0, 0)
    assert (high["errors"], high["examples"]) == (0, 1) and high["tp"].tolist() == [0, 1, 0]
    assert np.array_equal(sweep_counters(*data, 3, 0.5, [0.1], one_class=True)[0], [2, 0, 0, 1, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1])


@pytest.mark.parametrize("shape", [(5, 5, 1, 1), (9, 100, 7, 7), (70, 100, 33, 80)])
@pytest.mark.parametrize("one_class", [False, True])
def test_sweep_counters_equals_the_host_class_on_the_recipe(shape, one_class):
    from yolo_v3_tf2_amd.evaluate_detections import sweep_counters
    B, M, G, nc = shape
    data = recipe(sum(shape), B, M, G, nc)
    thresholds = [0.05, 0.3, 0.6, 0.95, 1.0]
    got = sweep_counters(*data, nc, 0.5, thresholds, one_class=one_class)
    assert np.array_equal(got, reference_counters(*data, nc, 0.5, thresholds, one_class=one_class))
    assert got[-1, :nc].sum() == 0 and got[0, :nc].sum() > 0          # no prediction above 1.0, some above 0.05


def test_counters_from_row_refuses_another_width():
    from yolo_v3_tf2_amd.evaluate_detections import counters_from_row
    with pytest.raises(ValueError):
        counters_from_row(np.zeros(17, np.int64), 4)


def _tied_set(seed, B, N):
    """Random boxes with forced score ties: the scores are drawn from 40 values."""
    rng = np.random.default_rng(seed)
    c, s = rng.random((B, N, 2)), rng.uniform(0.05, 0.4, (B, N, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2], -1).astype(np.float32)
    scores = (rng.integers(0, 40, (B, N)) / np.float32(40)).astype(np.float32)
    return boxes, scores


@pytest.mark.parametrize("M", [100, 10])
def test_higher_thresholds_are_prefixes_of_the_lowest_one(M):
    """The property one detect pass for all thresholds rests on: oracle.nms_padded at 0.1 / 0.2 / 0.5 / 0.9 equals, index for
    index, the rows with score > t of its result at 0.004, capped the same way."""
    from oracle import oracle as O
    d = np.load(os.path.join(ROOT, "tests", "golden", "nms_stress_n3000.npz"))
    for boxes, scores in ((d["boxes"], d["scores"]), _tied_set(11, 3, 300)):
        sel0, nv0 = O.nms_padded(boxes, scores, M, 0.5, 0.004)
        assert (nv0 > 0).all()
        seen = set()
        for t in (0.1, 0.2, 0.5, 0.9):
            sel, nv = O.nms_padded(boxes, scores, M, 0.5, t)
            for b in range(len(boxes)):
                rows = sel0[b, :nv0[b]]
                keep = rows[scores[b, rows] > np.float32(t)]
                assert nv[b] == len(keep) and np.array_equal(sel[b, :nv[b]], keep), (M, t, b)
                seen.add(int(nv[b]))
        # (under the cap of 10 most cuts are hidden: there the test is about the cap being applied the same way)
        assert M == 10 or len(seen) > 2, "the thresholds must cut the list at different lengths"


# a pointer that is never dereferenced: every check fails on the host before any HIP call
_FAKE = 0x10000


def _call(lib, **kw):
    import ctypes as C
    thr = (C.c_float * 16)(*([0.1] * 16))
    a = dict(packed=_FAKE, nv=_FAKE, batch=2, max_boxes=100, gt_boxes=_FAKE, gt_classes=_FAKE, gt_count=_FAKE, max_gt=10, nclasses=80,
             thr=thr, n_thr=5, counters=_FAKE)
    a.update(kw)
    return lib.y3_evaluate_detections(a["packed"], a["nv"], a["batch"], a["max_boxes"], a["gt_boxes"], a["gt_classes"], a["gt_count"],
                                      a["max_gt"], a["nclasses"], 0.5, a["thr"], a["n_thr"], 0, a["counters"], None)


@pytest.mark.parametrize("bad", [dict(packed=None), dict(nv=None), dict(gt_boxes=None), dict(gt_classes=None), dict(gt_count=None),
                                 dict(thr=None), dict(counters=None), dict(batch=0), dict(max_boxes=0), dict(max_boxes=1025),
                                 dict(max_gt=0), dict(max_gt=1025), dict(nclasses=0), dict(nclasses=4097), dict(n_thr=0),
                                 dict(n_thr=17)], ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_bad_arguments_are_refused_on_the_host(bad):
    from yolo_v3_tf2_amd import _lib
    lib = _lib.load()
    assert _call(lib, **bad) == _lib.Y3_ERR_INVALID
    msg = lib.y3_last_error()
    assert b"y3_evaluate_detections" in msg and len(msg) > len(b"y3_evaluate_detections: "), msg


def test_pack_ground_truth():
    from yolo_v3_tf2_amd import runtime
    rng = np.random.default_rng(3)
    gts = [(rng.random((3, 4), dtype=np.float32), [4, 5, 6]), (np.zeros((0, 4), np.float32), []), (rng.random((1, 4)), np.array([7]))]
    boxes, classes, count = runtime.pack_ground_truth(gts)
    assert (boxes.shape, classes.shape, count.shape) == ((3, 3, 4), (3, 3), (3,))
    assert (boxes.dtype, classes.dtype, count.dtype) == (np.float32, np.int32, np.int32)
    assert count.tolist() == [3, 0, 1] and classes.tolist() == [[4, 5, 6], [0, 0, 0], [7, 0, 0]]
    assert np.array_equal(boxes[0], gts[0][0]) and not boxes[1].any() and not boxes[2, 1:].any()
    assert np.array_equal(boxes[2, 0], gts[2][0][0].astype(np.float32))
    wide = runtime.pack_ground_truth(gts, max_gt=5)
    assert wide[0].shape == (3, 5, 4) and np.array_equal(wide[0][:, :3], boxes) and not wide[0][:, 3:].any()
    with pytest.raises(runtime.Y3Error):
        runtime.pack_ground_truth(gts, max_gt=2)
    with pytest.raises(runtime.Y3Error):
        runtime.pack_ground_truth([(np.zeros((2, 4)), [1])])
    # into a caller's buffers, which held something else
    out = (np.full((3, 3, 4), 9, np.float32), np.full((3, 3), 9, np.int32), np.full((3,), 9, np.int32))
    got = runtime.pack_ground_truth(gts, out=out)
    assert all(g is o for g, o in zip(got, out)) and all(np.array_equal(g, w) for g, w in zip(got, (boxes, classes, count)))
    with pytest.raises(runtime.Y3Error):
        runtime.pack_ground_truth(gts, out=(out[0], out[1].astype(np.int64), out[2]))
    # images without any box at all still give a row to point at
    assert runtime.pack_ground_truth([(np.zeros((0, 4)), [])])[0].shape == (1, 1, 4)


def test_no_cpu_fallback():
    import torch
    from yolo_v3_tf2_amd import runtime
    packed, nv, gb, gc, cnt = (torch.from_numpy(a) for a in recipe(1, 2, 5, 3, 4))
    with pytest.raises(runtime.Y3Error):
        runtime.evaluate_detections(packed, nv, gb, gc, cnt, 4, 0.5, [0.1])
