"""Average precision on the GPU: ap_match_kernel (y3_match_detections) against its host restatement match_detections, which
tests/test_ap_host.py ties to hand-written expectations and a brute-force loop; Net.evaluate_stream(ap=) and
evaluate(on_device=True, ap=) against the calls composed by hand; graph capture; the argument checks.  Records and totals are
integers: every comparison is np.array_equal, no tolerance."""
import ctypes as C

import numpy as np
import pytest

from tests.ap_cases import INVALID, RECIPE_NC, RECIPE_SEED, THRESHOLDS, recipe, unit_cases

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

POISON = np.uint32(0xDEADBEEF).view(np.int32).item()


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _match(rt, data, nc, thresholds, one_class=False, totals=None):
    """The call into a poisoned records buffer with one guard image on either side -> (records uint32 [B,M,2], totals)."""
    B, M = data[0].shape[:2]
    buf = torch.full((B + 2, M, 2), POISON, dtype=torch.int32, device="cuda")
    _, totals = rt.match_detections(*[_cuda(a) for a in data], nc, thresholds, one_class=one_class, records=buf[1:-1], gt_totals=totals)
    got = buf.cpu().numpy()
    assert (got[0] == POISON).all() and (got[-1] == POISON).all(), "a record outside the batch was written"
    return got[1:-1].view(np.uint32), totals


@pytest.mark.parametrize("case", unit_cases(), ids=lambda c: c[0])
def test_kernel_on_the_unit_cases(rt, case):
    from yolo_v3_tf2_amd.evaluate_detections import match_detections
    name, nc, thresholds, data, _ = case
    for one_class in (False, True):
        want, want_totals = match_detections(*data, nc, thresholds, one_class=one_class)
        got, totals = _match(rt, data, nc, thresholds, one_class)
        assert np.array_equal(got, want), (name, one_class)
        assert totals.dtype == torch.int64 and np.array_equal(totals.cpu().numpy(), want_totals), (name, one_class)


@pytest.mark.parametrize("M", [1, 16, 100, 257])
@pytest.mark.parametrize("G", [1, 63, 64, 65, 130])
def test_kernel_equals_the_restatement_on_the_recipe(rt, G, M):
    """Ground truth of 1, 63, 64, 65 and 130 rows (one lane slot, the edges of the first, three slots), 1 to 257 packed rows,
    batches of 1 and 5, 1, 10 and 16 IoU thresholds (1, 10 and 16 waves), one_class off and on.  Every record row is written:
    the buffer is poisoned and compared whole.  A second call on the same totals doubles them."""
    from yolo_v3_tf2_amd.evaluate_detections import match_detections
    for B in (1, 5):
        data = recipe(RECIPE_SEED, B, M, G)
        for K in (1, 10, 16):
            for one_class in (False, True):
                want, want_totals = match_detections(*data, RECIPE_NC, THRESHOLDS[K], one_class=one_class)
                got, totals = _match(rt, data, RECIPE_NC, THRESHOLDS[K], one_class)
                assert np.array_equal(got, want), (B, K, one_class)
                assert np.array_equal(totals.cpu().numpy(), want_totals)
                again, totals = _match(rt, data, RECIPE_NC, THRESHOLDS[K], one_class, totals=totals)
                assert np.array_equal(again, want), "a second run gives the same records"
                assert np.array_equal(totals.cpu().numpy(), 2 * want_totals), "gt_totals accumulates"


def test_kernel_at_the_largest_admitted_sizes(rt):
    """max_boxes = max_gt = 1024, nclasses = 4096, 16 thresholds: 60 KB of LDS and 1024 threads, the largest launch there is."""
    from yolo_v3_tf2_amd.evaluate_detections import match_detections
    data = recipe(RECIPE_SEED, 2, 1024, 1024, nc=4096)
    assert data[1][0] == 1024 and data[4][0] == 1024
    want, want_totals = match_detections(*data, 4096, THRESHOLDS[16])
    got, totals = _match(rt, data, 4096, THRESHOLDS[16])
    assert np.array_equal(got, want) and np.array_equal(totals.cpu().numpy(), want_totals)
    assert ((want[..., 1] != INVALID) & (want[..., 1] >> 16 != 0)).sum() > 100


def test_an_image_gives_the_same_records_anywhere_in_the_batch(rt):
    data = recipe(RECIPE_SEED, 5, 100, 65)
    whole, _ = _match(rt, data, RECIPE_NC, THRESHOLDS[10])
    for b in (0, 3):
        alone, _ = _match(rt, [a[b:b + 1] for a in data], RECIPE_NC, THRESHOLDS[10])
        assert np.array_equal(alone[0], whole[b])
    swapped, _ = _match(rt, [a[::-1] for a in data], RECIPE_NC, THRESHOLDS[10])
    assert np.array_equal(swapped[::-1], whole)


def test_match_under_graph_capture(rt):
    """y3_match_detections only enqueues: captured once, replayed twice on new rows; the records are those of the last rows and
    the totals the sum."""
    from yolo_v3_tf2_amd.evaluate_detections import match_detections
    first, second = recipe(RECIPE_SEED, 3, 100, 65), recipe(RECIPE_SEED + 5, 3, 100, 65)
    bufs = [_cuda(a) for a in first]
    records = torch.full((3, 100, 2), POISON, dtype=torch.int32, device="cuda")
    totals = torch.zeros(RECIPE_NC + 2, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rt.match_detections(*bufs, RECIPE_NC, THRESHOLDS[10])             # warm-up
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rt.match_detections(*bufs, RECIPE_NC, THRESHOLDS[10], records=records, gt_totals=totals)
    totals.zero_()
    want_totals = 0
    for data in (first, second):
        for buf, a in zip(bufs, data):
            buf.copy_(_cuda(a))
        records.fill_(POISON)
        g.replay()
        torch.cuda.synchronize()
        want, t = match_detections(*data, RECIPE_NC, THRESHOLDS[10])
        want_totals = want_totals + t
        assert np.array_equal(records.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(totals.cpu().numpy(), want_totals)


def test_argument_checks_leave_the_buffers_untouched(rt):
    """Each host check returns Y3_ERR_INVALID with its message before anything is enqueued."""
    from yolo_v3_tf2_amd import _lib
    lib = _lib.load()
    packed, nv, gb, gc, cnt = (_cuda(a) for a in recipe(RECIPE_SEED, 2, 5, 4))
    records = torch.full((2, 5, 2), POISON, dtype=torch.int32, device="cuda")
    totals = torch.full((RECIPE_NC + 2,), 7, dtype=torch.int64, device="cuda")
    thr = np.array([0.5, 0.75], np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    p = lambda t: C.c_void_p(t.data_ptr())
    good = dict(packed=p(packed), nv=p(nv), batch=2, M=5, gb=p(gb), gc=p(gc), cnt=p(cnt), G=4, nc=RECIPE_NC, thr=fp(thr), K=2,
                one_class=0, records=p(records), totals=p(totals))

    def call(**kw):
        a = dict(good, **kw)
        return lib.y3_match_detections(a["packed"], a["nv"], a["batch"], a["M"], a["gb"], a["gc"], a["cnt"], a["G"], a["nc"], a["thr"],
                                       a["K"], a["one_class"], a["records"], a["totals"], _lib.stream_ptr())

    bad = [(dict(batch=0), b"batch"), (dict(M=0), b"max_boxes"), (dict(M=1025), b"max_boxes"), (dict(G=0), b"max_gt"),
           (dict(G=1025), b"max_gt"), (dict(nc=0), b"nclasses"), (dict(nc=4097), b"nclasses"), (dict(K=0), b"n_iou"),
           (dict(K=17), b"n_iou"), (dict(thr=fp(np.array([0.5, np.nan], np.float32))), b"not finite"),
           (dict(thr=fp(np.array([np.inf, 0.5], np.float32))), b"not finite")]
    bad += [(dict([(k, None)]), b"null pointer") for k in ("packed", "nv", "gb", "gc", "cnt", "thr", "records", "totals")]
    bad += [(dict(records=C.c_void_p(records.data_ptr() + 4)), b"aligned")]
    for kw, word in bad:
        assert call(**kw) == _lib.Y3_ERR_INVALID, kw
        msg = lib.y3_last_error()
        assert b"y3_match_detections" in msg and word in msg, (kw, msg)
    torch.cuda.synchronize()
    assert (records.cpu().numpy() == POISON).all() and (totals.cpu().numpy() == 7).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not (records.cpu().numpy() == POISON).any() and totals.cpu().numpy()[RECIPE_NC + 1] == 7 + 2
    # the Python wrapper refuses what it can see itself
    for kw in (dict(records=records[:1]), dict(records=records.long()), dict(gt_totals=totals[:-1]), dict(gt_totals=totals.int()),
               dict(records=records.cpu())):
        with pytest.raises(rt.Y3Error):
            rt.match_detections(packed, nv, gb, gc, cnt, RECIPE_NC, thr, **kw)
    with pytest.raises(rt.Y3Error):
        rt.match_detections(packed, nv, gb, gc, cnt, RECIPE_NC, [0.5] * 17)


# ---------------------------------------------------------------------------------------------------------------------------
# Net.evaluate_stream(ap=): the frames and the ground truth of tests/test_evaluate_gpu.py
def _counting(lib, name, calls):
    class Counting:
        def __getattr__(self, attr):
            fn = getattr(lib, attr)
            if attr != name:
                return fn

            def counted(*a):
                calls.append(a[2])
                return fn(*a)
            return counted
    return Counting()


@pytest.mark.parametrize("letterbox", [False, True])
def test_evaluate_stream_ap_equals_the_calls_composed_by_hand(rt, program, weights, anchors, letterbox):
    """Batches of 4, 4 and 3 frames at S = 160: evaluate_stream(ap=True) == per batch Net.detect (+ unletterbox_detections),
    match_detections on the device, then average_precision over the concatenated records on the host; the device records equal
    the restatement's on the same rows.  The counters are those of the ap=None call, which makes no y3_match_detections call."""
    from tests.test_evaluate_gpu import STREAM_S, STREAM_THRESHOLDS, _detect, _ground_truth_from, _stream_batches
    from yolo_v3_tf2_amd.evaluate_detections import AP_IOU_THRESHOLDS, average_precision, match_detections
    S, batches = STREAM_S, _stream_batches()
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(4, S)
    rng = np.random.default_rng(5)
    detections = [_detect(rt, net, b, anchors, S, min(STREAM_THRESHOLDS), letterbox) for b in batches]
    gts = [_ground_truth_from(*d, rng, first=4 * i) for i, d in enumerate(detections)]
    G = max(len(c) for g in gts for _, c in g)
    for one_class in (False, True):
        records, totals, host_records, host_totals = [], None, [], 0
        for (packed, nv), gt in zip(detections, gts):
            gb, gc, cnt = rt.pack_ground_truth(gt, G)
            rec, totals = rt.match_detections(_cuda(packed), _cuda(nv), _cuda(gb), _cuda(gc), _cuda(cnt), 80, AP_IOU_THRESHOLDS,
                                              one_class=one_class, gt_totals=totals)
            records.append(rec.cpu().numpy().view(np.uint32))
            r, t = match_detections(packed, nv, gb, gc, cnt, 80, AP_IOU_THRESHOLDS, one_class=one_class)
            host_records.append(r)
            host_totals = host_totals + t
        records, totals = np.concatenate(records), totals.cpu().numpy()
        assert np.array_equal(records, np.concatenate(host_records)) and np.array_equal(totals, host_totals)
        want = average_precision(records, totals, 80, 10)
        calls = []
        real, net.lib = net.lib, _counting(net.lib, "y3_match_detections", calls)
        try:
            plain = net.evaluate_stream(batches, gts, anchors, 100, 0.5, STREAM_THRESHOLDS, 80, one_class=one_class, letterbox=letterbox)
            assert calls == [], "ap=None makes no y3_match_detections call"
            counters, got = net.evaluate_stream(batches, gts, anchors, 100, 0.5, STREAM_THRESHOLDS, 80, one_class=one_class,
                                                letterbox=letterbox, ap=True)
            assert calls == [4, 4, 3], "one y3_match_detections call per batch"
        finally:
            net.lib = real
        assert isinstance(plain, np.ndarray) and np.array_equal(counters, plain)
        assert sorted(got) == ["ap", "errors", "images", "mAP", "map"] and got["ap"].shape == (10, 80)
        assert np.array_equal(got["ap"], want["ap"], equal_nan=True) and np.array_equal(got["map"], want["map"])
        assert got["mAP"] == want["mAP"] and (got["images"], got["errors"]) == (11, 0)
        masks = (records[..., 1] >> 16)[records[..., 1] != INVALID]
        print(letterbox, one_class, "rows", len(masks), "matched at 0.5", int((masks & 1).sum()), "at 0.95", int((masks >> 9).sum()),
              "mAP", got["mAP"], "AP50", got["map"][0])
        assert 0.0 < got["mAP"] < 1.0 and got["map"][0] > got["map"][-1], "the ground truth is made from jittered detections"
    # "both" follows the plain variant; a sequence means those thresholds; loss and ap come back in that order
    (c0, c1), both = net.evaluate_stream(batches, gts, anchors, 100, 0.5, STREAM_THRESHOLDS, 80, one_class="both", letterbox=letterbox,
                                         ap=True, depth=3)
    plain_ap = net.evaluate_stream(batches, gts, anchors, 100, 0.5, STREAM_THRESHOLDS, 80, letterbox=letterbox, ap=True)[1]
    assert np.array_equal(both["ap"], plain_ap["ap"], equal_nan=True) and np.array_equal(c1, counters)
    two = net.evaluate_stream(batches, gts, anchors, 100, 0.5, STREAM_THRESHOLDS, 80, letterbox=letterbox, ap=[0.5, 0.75])[1]
    assert np.array_equal(two["ap"], plain_ap["ap"][[0, 5]], equal_nan=True)
    if not letterbox:
        out = net.evaluate_stream(batches, gts, anchors, 100, 0.5, STREAM_THRESHOLDS, 80, loss=True, ap=True)
        ref = net.evaluate_stream(batches, gts, anchors, 100, 0.5, STREAM_THRESHOLDS, 80, loss=True)
        assert len(out) == 3 and np.array_equal(out[0], ref[0]) and np.array_equal(out[1]["sum"], ref[1]["sum"])
        assert np.array_equal(out[2]["ap"], plain_ap["ap"], equal_nan=True)


@pytest.mark.parametrize("mode", ["bf16", "rect"])
def test_evaluate_stream_ap_on_other_plans(rt, program, weights, anchors, mode):
    """A bf16 plan and a rectangular (128 x 160) letterboxed plan: the AP equals the hand-composed route's on that plan's own
    detections, which come from detect_stream."""
    from tests.test_evaluate_gpu import _stream_batches
    from yolo_v3_tf2_amd import _lib
    from yolo_v3_tf2_amd.evaluate_detections import average_precision, match_detections
    batches = _stream_batches()[:2]
    net = rt.Net(program)
    net.load_weights(weights)
    letterbox = mode == "rect"
    net.plan(4, (128, 160) if letterbox else 160, _lib.Y3_DTYPE_BF16 if mode == "bf16" else _lib.Y3_DTYPE_F32)
    rng = np.random.default_rng(8)
    rows, gts = [], []
    for packed, nv in net.detect_stream(batches, anchors, 100, 0.5, 0.05, letterbox=letterbox):
        packed, nv = np.array(packed), np.array(nv)
        gt = []
        for b in range(len(nv)):
            keep = np.arange(0, int(nv[b]), 4)[:6]
            boxes = packed[b, keep, :4].copy().view(np.float32)
            sides = np.tile(boxes[:, 2:] - boxes[:, :2], 2)
            gt.append(((boxes + (rng.uniform(-0.03, 0.03, boxes.shape) * sides).astype(np.float32)), packed[b, keep, 5].astype(np.int32)))
        rows.append((packed, nv))
        gts.append(gt)
    G = max(len(c) for g in gts for _, c in g)
    records, totals = [], 0
    for (packed, nv), gt in zip(rows, gts):
        r, t = match_detections(packed, nv, *rt.pack_ground_truth(gt, G), 80, [0.5, 0.75, 0.9])
        records.append(r)
        totals = totals + t
    want = average_precision(np.concatenate(records), totals, 80, 3)
    _, got = net.evaluate_stream(batches, gts, anchors, 100, 0.5, [0.05, 0.2], 80, letterbox=letterbox, ap=[0.5, 0.75, 0.9])
    print(mode, "mAP", got["mAP"], got["map"])
    assert np.array_equal(got["ap"], want["ap"], equal_nan=True) and got["mAP"] == want["mAP"] and got["images"] == 8
    assert 0.0 < got["mAP"] <= 1.0


def _write_records(path, jpegs, truths):
    """One TFRecord file of the given JPEGs with per image (boxes [k,4], class ids [k]) -> the detect config that reads it."""
    import os
    from tests.test_evaluate_gpu import ROOT
    from yolo_v3_tf2_amd.core import load_tfrecords as m
    names = [l.rstrip("\n") for l in open(os.path.join(ROOT, "datasets/coco2012/coco.names"))]
    payloads = [m.make_example({"image/encoded": jpeg, "image/object/class/text": [names[c].encode() for c in classes],
                                "image/object/bbox/xmin": boxes[:, 0], "image/object/bbox/ymin": boxes[:, 1],
                                "image/object/bbox/xmax": boxes[:, 2], "image/object/bbox/ymax": boxes[:, 3]})
                for jpeg, (boxes, classes) in zip(jpegs, truths)]
    path.mkdir(exist_ok=True)
    m.write_records(str(path / "set.tfrec"), payloads)
    return dict(tfrecords_dir=str(path), image_size=128, batch_size=2, yolo_max_boxes=100, nms_iou_threshold=0.5,
                classes_name_file=os.path.join(ROOT, "datasets/coco2012/coco.names"),
                anchors_file=os.path.join(ROOT, "datasets/coco2012/anchors.txt"),
                model_config_file=os.path.join(ROOT, "config/models/yolov3/model.yaml"))


def test_driver_ap_equals_the_host_route(rt, weights, anchors, tmp_path, capsys):
    """A TFRecord set of three images (S = 128, batches of 2 and 1) whose 1, 2 and 3 ground-truth boxes are jittered copies of
    what the model detects on them (one with a changed class): evaluate(on_device=True, ap=...) == average_precision(
    match_detections(...)) on the detections the host route's model returns at the lowest score threshold."""
    from tests.evaluate_cases import pack_rows
    from tests.helpers import jpeg_bytes
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev
    from yolo_v3_tf2_amd.core import load_tfrecords as m
    from yolo_v3_tf2_amd.evaluate_detections import EvaluateDetections, average_precision, match_detections
    rng = np.random.default_rng(22)
    jpegs = [jpeg_bytes(rng, 120, 150) for _ in range(3)]
    thresholds, iou = [0.05, 0.3], [0.05, 0.5, 0.75]
    model = None

    def host_detections(cfg):
        """per image (boxes, classes, scores, num_valid) of the host route's model at the lowest threshold, and its ground truth"""
        data = list(m.parse_tfrecords(cfg["tfrecords_dir"], 128, 100, cfg["classes_name_file"]))
        out = []
        for i0 in (0, 2):      # the device route's batches: images 0-1, then image 2
            x = np.stack([d[0] for d in data[i0:i0 + 2]])
            for (bb, cc, ss, sel, nv), (_, y) in zip(zip(*model.predict(x)), data[i0:i0 + 2]):
                out.append(EvaluateDetections.gather_nms_output(bb, cc, ss, sel, nv) + (int(nv), y[y[:, 4] == 1]))
        return out

    box = np.array([[.2, .2, .6, .6]], np.float32)
    cfg = _write_records(tmp_path / "first", jpegs, [(box, [0])] * 3)
    model = ev.create_model(cfg["model_config_file"], 80, anchors, min(thresholds), 0.5, 100, None, weights)
    truths = []
    for i, (pb, pc, _, nv, _) in enumerate(host_detections(cfg)):
        assert nv >= 5
        rows = [0, 2, 4][:i + 1]
        boxes = pb[rows].astype(np.float32)
        sides = np.tile(boxes[:, 2:] - boxes[:, :2], 2)
        classes = pc[rows].astype(np.int64)
        classes[2:] = (classes[2:] + 1) % 80
        truths.append((boxes + (rng.uniform(-0.04, 0.04, boxes.shape) * sides).astype(np.float32), classes))
    cfg = _write_records(tmp_path / "second", jpegs, truths)
    capsys.readouterr()
    results, got = ev.evaluate(cfg, thresholds, evaluate_iou_threshold=0.1, weights=weights, on_device=True, ap=iou)
    printed = capsys.readouterr().out
    assert "AP50:" in printed and "AP75:" in printed and "mAP@[0.05:0.75]:" in printed
    assert [r[0] for r in results] == thresholds and results[0][3]["examples"] == 3
    records, totals = [], 0
    for pb, pc, ps, nv, y in host_detections(cfg):
        r, t = match_detections(pack_rows(pb, ps, pc, 100)[None], [nv], y[None, :, :4], y[None, :, 5].astype(np.int32), [len(y)], 80, iou)
        records.append(r)
        totals = totals + t
    want = average_precision(np.concatenate(records), totals, 80, 3)
    print("mAP", got["mAP"], got["map"], "rows", int(sum((r[..., 1] != INVALID).sum() for r in records)))
    assert np.array_equal(got["ap"], want["ap"], equal_nan=True) and np.array_equal(got["map"], want["map"])
    assert got["mAP"] == want["mAP"] and (got["images"], got["errors"]) == (3, 0) and totals[:80].sum() == 6
    assert 0.0 < got["mAP"] < 1.0, "five of the six boxes are jittered detections of their class"
