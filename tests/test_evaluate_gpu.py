"""Evaluation sweep on the GPU: evaluate_kernel (y3_evaluate_detections) against its host restatement sweep_counters, which
tests/test_evaluate_host.py ties to the existing EvaluateDetections class; Net.evaluate_stream and evaluate(on_device=True)
against the per-threshold route (one Net.detect per threshold, host counters); graph capture.  The counters are integers:
every comparison is np.array_equal."""
import os

import numpy as np
import pytest

from tests.evaluate_cases import batch_of, recipe, reference_counters, unit_cases

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _split(row, nc):
    """(tp, fp, fn, gts, preds) totals of a counters row"""
    s = lambda i: int(row[i * nc:(i + 1) * nc].sum())
    return s(2), s(3), s(4), s(1), s(0)


THRESHOLDS = {5: [0.05, 0.3, 0.6, 0.95, 1.0], 1: [0.3], 16: [round(0.02 + 0.0625 * i, 4) for i in range(16)]}


@pytest.fixture(scope="module")
def recipes():
    """The recipe of every shape, made once and left unchanged."""
    return {s: recipe(sum(s), *s) for s in [(5, 5, 1, 1), (9, 100, 7, 7), (70, 100, 33, 80), (3, 1024, 100, 80)]}


def _guarded(rt, data, nc, iou, thresholds, one_class):
    """The call on a view with one guard image on either side (filled with rows that would count if they were read)."""
    packed, nv, gb, gc, cnt = data
    pad = lambda a, fill: np.concatenate([fill[None], a, fill[None]])
    bufs = [_cuda(pad(packed, packed[0])), _cuda(pad(nv, nv[0])), _cuda(pad(gb, gb[0])), _cuda(pad(gc, gc[0])), _cuda(pad(cnt, cnt[0]))]
    before = [b.clone() for b in bufs]
    got = rt.evaluate_detections(*[b[1:-1] for b in bufs], nc, iou, thresholds, one_class=one_class)
    again = rt.evaluate_detections(*[b[1:-1] for b in bufs], nc, iou, thresholds, one_class=one_class, counters=got.clone())
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, before)), "the inputs were written"
    return got.cpu().numpy(), again.cpu().numpy()


@pytest.mark.parametrize("one_class", [0, 1])
@pytest.mark.parametrize("T", [5, 1, 16])
@pytest.mark.parametrize("shape", [(5, 5, 1, 1), (9, 100, 7, 7), (70, 100, 33, 80), (3, 1024, 100, 80)])
def test_kernel_equals_sweep_counters_on_the_recipe(rt, recipes, shape, T, one_class):
    """Rows of 1, 7, 33 and 100 ground-truth boxes, 5 to 1024 packed rows (one to four rows per thread), 1 to 80 classes, more
    images than one wave of workgroups is not needed: an image is a workgroup.  A second call on the same buffer doubles it."""
    from yolo_v3_tf2_amd.evaluate_detections import sweep_counters
    B, M, G, nc = shape
    data, thresholds = recipes[shape], THRESHOLDS[T]
    want = sweep_counters(*data, nc, 0.5, thresholds, one_class=bool(one_class))
    got, twice = _guarded(rt, data, nc, 0.5, thresholds, one_class)
    print(shape, T, one_class, [_split(r, nc)[:3] for r in got])
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(twice, 2 * want)
    assert want[:, 5 * nc + 1].tolist() == [B] * len(thresholds) and not want[:, 5 * nc].any()
    if T == 5 and not one_class:   # the test cannot pass on zeros, and sees the corners it is meant to see
        if shape != (5, 5, 1, 1):
            for t in range(3):
                tp, fp, fn, _, _ = _split(want[t], nc)
                assert tp > 0 and fp > 0 and fn > 0, (shape, thresholds[t], tp, fp, fn)
        assert _split(want[4], nc)[4] == 0, "no prediction is above 1.0"
        if shape == (9, 100, 7, 7):
            tp, _, _, gts, _ = _split(want[0], nc)
            assert tp > gts, "two predictions on one ground-truth box must both count"


def test_kernel_at_the_largest_admitted_sizes(rt):
    """max_gt = 1024 and nclasses = 4096, the limits the entry admits: 100 KB of LDS per workgroup, beyond the 64 KB a kernel
    may use without its limit being raised (the only launches that take that path).  Image 0 holds all 1024 ground-truth rows."""
    from yolo_v3_tf2_amd.evaluate_detections import sweep_counters
    B, M, G, nc = 3, 64, 1024, 4096
    data, thresholds = recipe(7, B, M, G, nc), THRESHOLDS[5]
    assert data[4][0] == G and data[1][0] == M
    want = sweep_counters(*data, nc, 0.5, thresholds)
    got, twice = _guarded(rt, data, nc, 0.5, thresholds, 0)
    assert np.array_equal(got, want) and np.array_equal(twice, 2 * want)
    tp, fp, fn, gts, _ = _split(want[0], nc)
    assert tp > 0 and fp > 0 and fn > 0 and gts >= G
    # a small launch after the large one is what it was
    small = recipe(sum((9, 100, 7, 7)), 9, 100, 7, 7)
    assert np.array_equal(rt.evaluate_detections(*[_cuda(a) for a in small], 7, 0.5, thresholds).cpu().numpy(),
                          sweep_counters(*small, 7, 0.5, thresholds))


@pytest.mark.parametrize("case", unit_cases(), ids=lambda c: c[0])
def test_kernel_on_the_unit_cases(rt, case):
    from yolo_v3_tf2_amd.evaluate_detections import sweep_counters
    name, nc, iou, thresholds, images, _ = case
    data = batch_of(images)
    for one_class in (False, True):
        want = sweep_counters(*data, nc, iou, thresholds, one_class=one_class)
        assert np.array_equal(want, reference_counters(*data, nc, iou, thresholds, one_class=one_class))
        got = rt.evaluate_detections(*[_cuda(a) for a in data], nc, iou, thresholds, one_class=one_class)
        assert np.array_equal(got.cpu().numpy(), want), (name, one_class)


def test_kernel_with_a_bad_prediction_class_stays_inside_its_counters(rt):
    """Class ids 7, -1 and 2**30 at nclasses = 3: an error image at the thresholds whose rows hold them (sweep_counters
    defines it), and nothing around the counters is written."""
    from yolo_v3_tf2_amd.evaluate_detections import sweep_counters
    box = [[.1, .1, .5, .5]]
    data = batch_of([(box * 2, [0.9, 0.4], [1, 7], box, [1]), (box * 2, [0.9, 0.4], [1, -1], box, [1]),
                     (box * 2, [0.9, 0.2], [2**30, 1], box, [1]), (box * 2, [0.9, 0.4], [1, 2], box, [1])])
    thresholds = [0.1, 0.5]
    want = sweep_counters(*data, 3, 0.5, thresholds)
    assert want[:, 15].tolist() == [3, 1] and want[:, 16].tolist() == [1, 3]
    buf = torch.full((4, 17), 5, dtype=torch.int64, device="cuda")
    rt.evaluate_detections(*[_cuda(a) for a in data], 3, 0.5, thresholds, counters=buf[1:3])
    got = buf.cpu().numpy()
    assert (got[0] == 5).all() and (got[3] == 5).all()
    assert np.array_equal(got[1:3] - 5, want)


def test_bad_arguments_raise(rt):
    data = [_cuda(a) for a in recipe(1, 3, 5, 4, 6)]
    packed, nv, gb, gc, cnt = data
    ok = rt.evaluate_detections(*data, 6, 0.5, [0.1])
    assert ok.shape == (1, 32)
    for args in ((packed.cpu(), nv, gb, gc, cnt), (packed, nv.cpu(), gb, gc, cnt), (packed.float(), nv, gb, gc, cnt),
                 (packed, nv.long(), gb, gc, cnt), (packed, nv, gb.double(), gc, cnt), (packed, nv, gb, gc.long(), cnt),
                 (packed, nv[:2], gb, gc, cnt), (packed, nv, gb[:2], gc, cnt), (packed, nv, gb, gc[:, :3], cnt),
                 (packed, nv, gb, gc, cnt[:1]), (packed[..., :6], nv, gb, gc, cnt)):
        with pytest.raises(rt.Y3Error):
            rt.evaluate_detections(*args, 6, 0.5, [0.1])
    for kw in (dict(counters=ok.int()), dict(counters=ok[:, :31]), dict(counters=ok.cpu())):
        with pytest.raises(rt.Y3Error):
            rt.evaluate_detections(*data, 6, 0.5, [0.1], **kw)
    with pytest.raises(rt.Y3Error):
        rt.evaluate_detections(*data, 6, 0.5, [0.1] * 17)
    with pytest.raises(rt.Y3Error):
        rt.evaluate_detections(*data, 5000, 0.5, [0.1])


# ---------------------------------------------------------------------------------------------------------------------------
# Net.evaluate_stream: S = 160, the frames of tests/test_letterbox_gpu.py::stream_batches
STREAM_S = 160
STREAM_THRESHOLDS = [0.05, 0.1, 0.15, 0.3]


def _stream_batches():
    from tests.test_letterbox_gpu import stream_batches
    return stream_batches()


def _staged(rt, frames, S, letterbox):
    batch = torch.zeros((len(frames), S, S, 3), device="cuda")
    for slot, img in enumerate(frames):
        rt.preprocess_image(_cuda(img), batch, slot, letterbox=letterbox)
    return batch


def _detect(rt, net, frames, anchors, S, threshold, letterbox):
    """The serial route at one threshold -> (packed, num_valid) as NumPy, boxes in the frames' own coordinates."""
    from yolo_v3_tf2_amd.core.utils import letterbox_geometry
    packed, nv = net.detect(_staged(rt, frames, S, letterbox), anchors, 100, 0.5, threshold)
    if letterbox:
        geoms = np.stack([letterbox_geometry(im.shape[0], im.shape[1], S, S) for im in frames])
        rt.unletterbox_detections(packed, nv, geoms, S)
    return packed.cpu().numpy(), nv.cpu().numpy()


def _ground_truth_from(packed, nv, rng, nc=80, first=0):
    """Per image: every fifth detected row's box, jittered, with its class (every third one changed), and two random boxes.
    Image i of the stream (i = first + its place in the batch) keeps 3 + 7 i mod 11 of those rows: unlike counts per image."""
    gts = []
    for b in range(len(packed)):
        rows = np.arange(0, int(nv[b]), 5)[:3 + (7 * (first + b)) % 11]
        boxes = packed[b, rows, :4].copy().view(np.float32)
        sides = np.tile(boxes[:, 2:] - boxes[:, :2], 2)
        boxes = boxes + (rng.uniform(-0.02, 0.02, boxes.shape) * sides).astype(np.float32)      # +-2 % of the box's sides
        classes = packed[b, rows, 5].copy()
        classes[2::3] = (classes[2::3] + 1) % nc
        c, s = rng.uniform(0.2, 0.8, (2, 2)), rng.uniform(0.1, 0.3, (2, 2))
        boxes = np.concatenate([boxes, np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32)])
        classes = np.concatenate([classes, rng.integers(0, nc, 2).astype(np.int32)])
        gts.append((boxes, classes.astype(np.int32)))
    return gts


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_evaluate_stream_equals_the_per_threshold_route(rt, program, weights, anchors, mode, letterbox):
    """evaluate_stream over batches of 4, 4 and 3 frames and four thresholds == for each threshold separately Net.detect at
    that threshold (+ unletterbox_detections), then EvaluateDetections on the host, plain and one-class.  The ground truth is
    made from the device's own detections at 0.05.  tests/test_letterbox_gpu.py records 43-100 valid rows per image at 0.05 and
    best scores of 0.19-0.27: 0.3 is the all-empty corner."""
    from yolo_v3_tf2_amd import _lib
    from yolo_v3_tf2_amd.evaluate_detections import EvaluateDetections, counters_from_row
    S, batches = STREAM_S, _stream_batches()
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(4, S, {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16}[mode])
    rng = np.random.default_rng(5)
    gts = [_ground_truth_from(*_detect(rt, net, b, anchors, S, 0.05, letterbox), rng, first=4 * i) for i, b in enumerate(batches)]
    assert len({len(c) for g in gts for _, c in g}) > 3, "unlike counts per image"
    want, want_one = [], []
    for t in STREAM_THRESHOLDS:
        ev, ev1 = EvaluateDetections(80, 0.5), EvaluateDetections(80, 0.5)
        for frames, gt in zip(batches, gts):
            packed, nv = _detect(rt, net, frames, anchors, S, t, letterbox)
            for b, (gb, gc) in enumerate(gt):
                pb, pc = packed[b, :nv[b], :4].copy().view(np.float32), packed[b, :nv[b], 5]
                ev.evaluate(pb, pc, gb, gc)
                ev1.evaluate(pb, np.zeros_like(pc), gb, np.zeros_like(gc))
        want.append(ev.counters)
        want_one.append(ev1.counters)
    print(mode, letterbox, [(int(c["tp"].sum()), int(c["fp"].sum()), int(c["fn"].sum())) for c in want])
    first = want[0]
    assert first["tp"].sum() > 0 and first["fp"].sum() > 0 and first["fn"].sum() > 0 and first["examples"] == 11
    assert want[-1]["preds"].sum() == 0
    plain, one = net.evaluate_stream(batches, gts, anchors, 100, 0.5, STREAM_THRESHOLDS, 80, one_class="both", letterbox=letterbox)
    assert plain.dtype == np.int64 and plain.shape == one.shape == (4, 402)
    for t in range(len(STREAM_THRESHOLDS)):
        for got, ref in ((counters_from_row(plain[t], 80), want[t]), (counters_from_row(one[t], 80), want_one[t])):
            for k in ("preds", "gts", "tp", "fp", "fn", "errors", "examples"):
                assert np.array_equal(got[k], ref[k]), (t, k)
    # the single forms give the halves of the pair
    assert np.array_equal(net.evaluate_stream(batches, gts, anchors, 100, 0.5, STREAM_THRESHOLDS, 80, letterbox=letterbox), plain)
    assert np.array_equal(net.evaluate_stream(batches, gts, anchors, 100, 0.5, STREAM_THRESHOLDS, 80, one_class=True, depth=3,
                                              letterbox=letterbox), one)


def test_evaluate_stream_makes_one_detect_call_per_batch(rt, program, weights, anchors):
    """The structural guarantee: three batches and four thresholds are three y3_net_detect calls (the per-threshold route makes
    twelve)."""
    batches = _stream_batches()
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(4, STREAM_S)
    gts = [[(np.array([[.2, .2, .6, .6]], np.float32), np.array([3], np.int32))] * len(b) for b in batches]
    calls = []

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if name != "y3_net_detect":
                return fn

            def counted(*a):
                calls.append(a[2])
                return fn(*a)
            return counted

    real = net.lib
    net.lib = Counting(real)
    try:
        out = net.evaluate_stream(batches, gts, anchors, 100, 0.5, STREAM_THRESHOLDS, 80)
    finally:
        net.lib = real
    assert calls == [4, 4, 3]
    assert out[:, 401].tolist() == [11] * 4 and out[:, 80:160].sum(axis=1).tolist() == [11] * 4
    # frames and ground truth drawn from iterators, in step: the same counters
    lazy = net.evaluate_stream(iter(batches), iter(gts), anchors, 100, 0.5, STREAM_THRESHOLDS, 80, max_batch=4,
                               max_blob_bytes=max(rt.packed_nbytes(b) for b in batches), max_gt=5)
    assert np.array_equal(lazy, out)


def test_evaluate_stream_refuses_what_it_cannot_pair(rt, program, weights, anchors):
    batches = _stream_batches()
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(4, STREAM_S)
    gt = (np.array([[.2, .2, .6, .6]], np.float32), np.array([3], np.int32))
    with pytest.raises(rt.Y3Error):
        net.evaluate_stream(batches, [[gt] * 4, [gt] * 4, [gt] * 2], anchors, 100, 0.5, [0.1], 80)
    with pytest.raises(rt.Y3Error):
        net.evaluate_stream(batches, [[gt] * 4], anchors, 100, 0.5, [0.1], 80)
    with pytest.raises(rt.Y3Error, match="more entries"):
        net.evaluate_stream(batches, [[gt] * len(b) for b in batches] + [[gt]], anchors, 100, 0.5, [0.1], 80)
    with pytest.raises(rt.Y3Error, match="max_gt"):
        net.evaluate_stream(batches, iter([[gt] * len(b) for b in batches]), anchors, 100, 0.5, [0.1], 80)
    with pytest.raises(rt.Y3Error):
        net.evaluate_stream(batches, [[gt] * len(b) for b in batches], anchors, 100, 0.5, [0.1], 80, one_class="each")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
def _write_set(tmp_path, boxes_per_image, seed):
    from tests.helpers import jpeg_bytes
    from yolo_v3_tf2_amd.core import load_tfrecords as m
    rng = np.random.default_rng(seed)
    names = [l.rstrip("\n") for l in open(os.path.join(ROOT, "datasets/coco2012/coco.names"))]
    payloads = []
    for i, k in enumerate(boxes_per_image):
        lo = (rng.random((k, 2)) * 0.5).astype(np.float32)
        hi = lo + 0.3
        payloads.append(m.make_example({"image/encoded": jpeg_bytes(rng, 120, 150),
                                        "image/object/class/text": [names[i + 7 * j].encode() for j in range(k)],
                                        "image/object/bbox/xmin": lo[:, 0], "image/object/bbox/ymin": lo[:, 1],
                                        "image/object/bbox/xmax": hi[:, 0], "image/object/bbox/ymax": hi[:, 1]}))
    tmp_path.mkdir(exist_ok=True)
    m.write_records(str(tmp_path / "set.tfrec"), payloads)
    return dict(tfrecords_dir=str(tmp_path), image_size=128, batch_size=2, yolo_max_boxes=100, nms_iou_threshold=0.5,
                classes_name_file=os.path.join(ROOT, "datasets/coco2012/coco.names"),
                anchors_file=os.path.join(ROOT, "datasets/coco2012/anchors.txt"),
                model_config_file=os.path.join(ROOT, "config/models/yolov3/model.yaml"))


def _same_results(a, b):
    assert [r[0] for r in a] == [r[0] for r in b]
    for (_, ra, pa, ca, oa), (_, rb, pb, cb, ob) in zip(a, b):
        assert np.array_equal(ra, rb) and np.array_equal(pa, pb) and ra.dtype == rb.dtype
        for x, y in ((ca, cb), (oa, ob)):
            assert sorted(x) == sorted(y)
            for k in x:
                assert np.array_equal(x[k], y[k]), k


def test_driver_on_device_equals_the_host_route(rt, weights, tmp_path):
    """The TFRecord set of tests/test_gpu_parity.py::test_evaluate_driver_counters_match_oracle (four images of two boxes, S =
    128, thresholds 0.05 and 0.3, IoU 0.1): evaluate(on_device=True) == evaluate(on_device=False) in every counter of both
    dicts and in recall / precision."""
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev
    cfg = _write_set(tmp_path / "even", [2, 2, 2, 2], 21)
    host = ev.evaluate(cfg, [0.05, 0.3], evaluate_iou_threshold=0.1, weights=weights)
    dev = ev.evaluate(cfg, [0.05, 0.3], evaluate_iou_threshold=0.1, weights=weights, on_device=True)
    _same_results(dev, host)
    assert dev[0][3]["examples"] == 4 and dev[0][3]["gts"].sum() == 8 and dev[0][3]["preds"].sum() > 0
    assert dev[0][4]["gts"].tolist()[0] == 8
    # max_batches and one_class=False mean what they mean on the host route: the first batch only, one-class counters left at zero
    first = ev.evaluate(cfg, [0.05], evaluate_iou_threshold=0.1, weights=weights, max_batches=1, one_class=False, on_device=True)
    assert first[0][3]["examples"] == 2 and first[0][3]["gts"].sum() == 4 and 0 < first[0][3]["preds"].sum() < dev[0][3]["preds"].sum()
    assert first[0][4]["examples"] == 0 and not any(first[0][4][k].any() for k in ("preds", "gts", "tp", "fp", "fn"))


def test_driver_on_device_batches_images_with_unlike_box_counts(rt, weights, anchors, tmp_path):
    """Images of 1, 2 and 3 boxes (the host route cannot stack them into one batch): the device route == a per-image host loop
    over Net.detect at each threshold."""
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev
    from yolo_v3_tf2_amd.core import load_tfrecords as m
    from yolo_v3_tf2_amd.evaluate_detections import EvaluateDetections
    cfg = _write_set(tmp_path / "ragged", [1, 2, 3], 22)
    thresholds = [0.05, 0.3]
    dev = ev.evaluate(cfg, thresholds, evaluate_iou_threshold=0.1, weights=weights, on_device=True)
    data = list(m.parse_tfrecords(cfg["tfrecords_dir"], 128, 100, cfg["classes_name_file"]))
    want = []
    for t in thresholds:
        model = ev.create_model(cfg["model_config_file"], 80, anchors, t, 0.5, 100, None, weights)
        ref, ref1 = EvaluateDetections(80, 0.1), EvaluateDetections(80, 0.1)
        for i0 in (0, 2):      # the device route's batches: images 0-1, then image 2
            x = np.stack([d[0] for d in data[i0:i0 + 2]])
            for (bb, cc, ss, sel, nv), (_, y) in zip(zip(*model.predict(x)), data[i0:i0 + 2]):
                y = y[y[:, 4] == 1]
                pb, pc, _ = EvaluateDetections.gather_nms_output(bb, cc, ss, sel, nv)
                ref.evaluate(pb, pc, y[:, :4], y[:, 5].astype(np.int32))
                ref1.evaluate(pb, np.zeros_like(pc), y[:, :4], np.zeros(len(y), np.int32))
        r, p = ev.calc_recal_precision(ref.counters)
        want.append((t, r, p, ref.counters, ref1.counters))
    _same_results(dev, want)
    assert dev[0][3]["examples"] == 3 and dev[0][3]["gts"].sum() == 6


def test_detect_and_evaluate_in_one_graph(rt, program, weights, anchors):
    """Net.detect + evaluate_detections captured once and replayed twice after new pixels: the counters equal the sum of the
    two eager results."""
    S, B, thresholds = 96, 3, [0.05, 0.1, 0.2]
    rng = np.random.default_rng(12)
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(B, S)
    images = torch.zeros((B, S, S, 3), device="cuda")
    first = _cuda(rng.random((B, S, S, 3), dtype=np.float32))
    packed, nv = net.detect(first, anchors, 100, 0.5, thresholds[0])
    gts = _ground_truth_from(packed.cpu().numpy(), nv.cpu().numpy(), rng)
    gb, gc, cnt = (_cuda(a) for a in rt.pack_ground_truth(gts))
    counters = torch.zeros((len(thresholds), 402), dtype=torch.int64, device="cuda")

    def step(x, acc):
        p, n = net.detect(x, anchors, 100, 0.5, thresholds[0])
        return rt.evaluate_detections(p, n, gb, gc, cnt, 80, 0.5, thresholds, counters=acc)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(images, torch.zeros_like(counters))             # warm-up
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(images, counters)
    counters.zero_()
    eager = []
    for k in range(2):
        x = first if k == 0 else _cuda(rng.random((B, S, S, 3), dtype=np.float32))
        eager.append(step(x, None).cpu().numpy())
        images.copy_(x)
        g.replay()
    torch.cuda.synchronize()
    assert not np.array_equal(eager[0], eager[1]), "the two replays must see different pixels"
    assert eager[0][0, 160:240].sum() > 0, "true positives at the lowest threshold"
    assert np.array_equal(counters.cpu().numpy(), eager[0] + eager[1])
