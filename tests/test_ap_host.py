"""Average precision, host tier (no GPU): evaluate_detections.match_detections -- the NumPy restatement of y3_match_detections --
against hand-written expectations and an independent brute-force loop; the AP integral against known answers; and the
conditions that make the recipe of tests/test_ap_gpu.py a test of the matching and not of its trivial paths."""
import numpy as np
import pytest

from tests.ap_cases import (INVALID, MAIN_SHAPE, RECIPE_NC, RECIPE_SEED, THRESHOLDS, brute_force, expected_records, recipe,
                            unit_cases)


def _masks_of(records, nv):
    """records [B,M,2] -> per image the masks of its valid rows, None for an image whose rows are all invalid although nv > 0"""
    out = []
    for b in range(len(records)):
        valid = records[b, :, 1] != INVALID
        out.append((records[b, valid, 1] >> 16).tolist() if valid.any() or nv[b] <= 0 else None)
    return out


@pytest.mark.parametrize("case", unit_cases(), ids=lambda c: c[0])
def test_restatement_on_the_unit_cases(case):
    from yolo_v3_tf2_amd.evaluate_detections import match_detections
    name, nc, thresholds, data, expected = case
    records, totals = match_detections(*data, nc, thresholds)
    want_records, want_totals = expected_records(case)
    assert records.dtype == np.uint32 and totals.dtype == np.int64
    assert np.array_equal(records, want_records), (name, _masks_of(records, data[1]))
    assert np.array_equal(totals, want_totals)
    for one_class in (False, True):
        records, totals = match_detections(*data, nc, thresholds, one_class=one_class)
        brute = brute_force(*data, nc, thresholds, one_class=one_class)
        M = records.shape[1]
        for b, masks in enumerate(brute):
            if masks is None:
                assert (records[b, :, 1] == INVALID).all() and not records[b, :, 0].any()
            else:
                n = len(masks)
                assert (records[b, :n, 1] >> 16).tolist() == masks and (records[b, n:, 1] == INVALID).all()
                assert (records[b, :n, 1] & 0xFFFF).tolist() == ([0] * n if one_class else data[0][b, :n, 5].tolist())
                assert np.array_equal(records[b, :n, 0], data[0][b, :n, 4].view(np.uint32)) and not records[b, n:, 0].any()
        assert totals[nc] == sum(m is None for m in brute) and totals[nc + 1] == sum(m is not None for m in brute)
    if name == "bad classes":
        assert totals[nc] == 0 and totals[nc + 1] == 5 and totals[0] == 10, "with one_class no class is bad"


@pytest.mark.parametrize("K", [1, 10, 16])
@pytest.mark.parametrize("shape", [(2, 16, 1), (3, 16, 7), (3, 40, 65), (2, 100, 130)])
def test_restatement_equals_the_brute_force_loop_on_the_recipe(shape, K):
    from yolo_v3_tf2_amd.evaluate_detections import match_detections
    data = recipe(RECIPE_SEED + 1, *shape)
    for one_class in (False, True):
        records, totals = match_detections(*data, RECIPE_NC, THRESHOLDS[K], one_class=one_class)
        assert _masks_of(records, data[1]) == brute_force(*data, RECIPE_NC, THRESHOLDS[K], one_class=one_class)
        assert totals[RECIPE_NC + 1] == shape[0] and totals[:RECIPE_NC].sum() == data[4].sum()


@pytest.mark.parametrize("K", [10, 16])
@pytest.mark.parametrize("shape", [MAIN_SHAPE, (5, 257, 130)])
def test_the_recipe_is_not_trivial(shape, K):
    """Conditions on the inputs, judged by the restatement alone: every mask bit is set in some valid row and clear in some valid
    row; some mask is not a prefix of the thresholds (a row matched at a higher threshold and not at a lower one); some row is
    matched to a box that is not the highest-IoU box of its class (the better one was taken)."""
    from yolo_v3_tf2_amd.evaluate_detections import EvaluateDetections, match_detections
    data = recipe(RECIPE_SEED, *shape)
    packed, nv, gb, gc, cnt = data
    records, totals, matches = match_detections(*data, RECIPE_NC, THRESHOLDS[K], return_matches=True)
    valid = records[..., 1] != INVALID
    masks = (records[..., 1] >> 16)[valid]
    assert valid.sum() == nv.sum() and nv[0] == shape[1] and cnt[0] == shape[2] and totals[RECIPE_NC] == 0
    for k in range(K):
        bit = (masks >> k) & 1
        assert bit.any() and not bit.all(), k
    prefix = [(1 << j) - 1 for j in range(K + 1)]
    non_prefix = sum(int(m) not in prefix for m in masks)
    second = 0
    boxes = packed[..., :4].copy().view(np.float32)
    for b, r, k in zip(*np.nonzero(matches >= 0)):
        same = np.flatnonzero(gc[b, :cnt[b]] == packed[b, r, 5])
        iou = EvaluateDetections.iou_alg(boxes[b, r], gb[b, same])
        second += iou[same == matches[b, r, k]][0] < iou.max()
    print(shape, K, "rows", int(valid.sum()), "non-prefix masks", non_prefix, "second-best matches", int(second))
    assert non_prefix > 0 and second > 0


# ------------------------------------------------------------------------------------------------ the AP integral
def _records(rows, M=None):
    """[(score, class, mask)] of one image -> records [1,M,2]"""
    M = M or max(len(rows), 1)
    rec = np.zeros((1, M, 2), np.uint32)
    rec[..., 1] = INVALID
    for r, (s, c, m) in enumerate(rows):
        rec[0, r] = (np.float32(s).view(np.uint32), c | (m << 16))
    return rec


def test_average_precision_known_answers():
    from yolo_v3_tf2_amd.evaluate_detections import average_precision
    # one class, two ground-truth boxes, rows TP, FP, TP by score: precision 1 up to recall 0.5 (51 samples), 2/3 up to 1 (50)
    out = average_precision(_records([(0.9, 0, 1), (0.8, 0, 0), (0.7, 0, 1)], M=5), [2, 0, 1], 1, 1)
    want = (51 * 1.0 + 50 * 2 / 3) / 101
    assert out["ap"].shape == (1, 1) and out["ap"].dtype == np.float64
    assert abs(out["ap"][0, 0] - want) < 1e-15 and abs(want - 0.8349834983498351) < 1e-15
    assert out["map"].tolist() == [out["ap"][0, 0]] and out["mAP"] == out["ap"][0, 0] and (out["images"], out["errors"]) == (1, 0)
    # the record order does not matter when the scores differ: the same rows, shuffled
    out2 = average_precision(_records([(0.7, 0, 1), (0.9, 0, 1), (0.8, 0, 0)]), [2, 0, 1], 1, 1)
    assert out2["ap"][0, 0] == out["ap"][0, 0]
    # all TP -> 1.0; no detection -> 0.0; a class without ground truth -> NaN, left out of the means; its detections change nothing
    out = average_precision(_records([(0.9, 0, 0b11), (0.8, 0, 0b11), (0.5, 2, 0)]), [2, 3, 0, 4, 1], 3, 2)
    assert out["ap"][:, 0].tolist() == [1.0, 1.0] and out["ap"][:, 1].tolist() == [0.0, 0.0] and np.isnan(out["ap"][:, 2]).all()
    assert out["map"].tolist() == [0.5, 0.5] and out["mAP"] == 0.5 and (out["images"], out["errors"]) == (1, 4)
    # bit k belongs to threshold k: TP at threshold 0 only
    out = average_precision(_records([(0.9, 0, 0b01)]), [1, 0, 1], 1, 2)
    assert out["ap"][:, 0].tolist() == [1.0, 0.0] and out["mAP"] == 0.5
    # half the boxes found, no false positive: 51 of the 101 samples (recall 0 .. 0.5) at precision 1
    out = average_precision(_records([(0.9, 0, 1)]), [2, 0, 1], 1, 1)
    assert abs(out["ap"][0, 0] - 51 / 101) < 1e-15
    # nothing at all
    out = average_precision(np.zeros((0, 4, 2), np.uint32), [0, 0, 0], 1, 1)
    assert np.isnan(out["ap"]).all() and np.isnan(out["mAP"]) and out["images"] == 0
    with pytest.raises(ValueError):
        average_precision(_records([]), [1, 0], 1, 1)


def test_average_precision_ties_follow_the_record_order():
    """Equal scores: the sort is stable, the earlier record comes first."""
    from yolo_v3_tf2_amd.evaluate_detections import average_precision
    tp_first = average_precision(_records([(0.5, 0, 1), (0.5, 0, 0)]), [1, 0, 1], 1, 1)["ap"][0, 0]
    fp_first = average_precision(_records([(0.5, 0, 0), (0.5, 0, 1)]), [1, 0, 1], 1, 1)["ap"][0, 0]
    assert tp_first == 1.0 and fp_first == 0.5


def test_average_precision_is_unchanged_under_a_permutation_of_the_images():
    from yolo_v3_tf2_amd.evaluate_detections import average_precision, match_detections
    data = recipe(RECIPE_SEED, 6, 40, 9)
    scores = np.concatenate([data[0][b, :n, 4].view(np.float32) for b, n in enumerate(data[1])])
    assert len(np.unique(scores)) == len(scores), "no two scores are equal"
    records, totals = match_detections(*data, RECIPE_NC, THRESHOLDS[10])
    want = average_precision(records, totals, RECIPE_NC, 10)
    assert 0.0 < want["mAP"] < 1.0 and want["map"][0] > want["map"][-1] and want["images"] == 6
    perm = np.random.default_rng(3).permutation(6)
    got = average_precision(records[perm], totals, RECIPE_NC, 10)
    assert np.array_equal(got["ap"], want["ap"]) and got["mAP"] == want["mAP"]
    # per-batch calls add up to the one call
    a, ta = match_detections(*[x[:4] for x in data], RECIPE_NC, THRESHOLDS[10])
    b, tb = match_detections(*[x[4:] for x in data], RECIPE_NC, THRESHOLDS[10])
    assert np.array_equal(np.concatenate([a, b]), records) and np.array_equal(ta + tb, totals)


def test_evaluate_refuses_ap_without_the_device_route():
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev
    with pytest.raises(ValueError, match="on_device"):
        ev.evaluate({}, [0.1], ap=True)
    with pytest.raises(SystemExit):
        ev.main(["--ap"])


def test_ap_iou_thresholds():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd.evaluate_detections import AP_IOU_THRESHOLDS
    assert np.array_equal(runtime.ap_iou_thresholds(True), np.linspace(0.5, 0.95, 10).astype(np.float32))
    assert runtime.ap_iou_thresholds(True) is AP_IOU_THRESHOLDS
    got = runtime.ap_iou_thresholds([0.5, 0.75])
    assert got.dtype == np.float32 and got.tolist() == [0.5, 0.75]
    for bad in ([], [0.5] * 17, [float("nan")], [float("inf")]):
        with pytest.raises(runtime.Y3Error):
            runtime.ap_iou_thresholds(bad)
