"""YOLOv3-tiny on the device: the max-pool kernel (csrc/maxpool.hip) against maxpool2x2_ref, the two-head network in fp32 against the
walker of tests/tiny_cases.py, the detection routes on two heads composed by hand, the streams, a 16-bit net with pools, and what
plan refuses.  Integer / index outputs and everything the pools, the up-sample and the concat move must match bit for bit; the bars
of the convs are those of tests/helpers.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import tiny_cases as TC  # noqa: E402
from tests.helpers import NETWORK_GRID_BAR, bf16_tile_bar, f32_conv_bar, oracle_launch  # noqa: E402
from yolo_v3_tf2_amd import _lib  # noqa: E402
from yolo_v3_tf2_amd.graph import AuxOp, ConvOp  # noqa: E402
from yolo_v3_tf2_amd.maxpool import maxpool2x2_ref  # noqa: E402

NC = 80
CANVASES = (96, (96, 64))         # grids 3, 6 and (3, 2), (6, 4)
BATCH = 2
# A score threshold inside the narrow score range of the random-init tiny heads (0.0047 .. 0.011 at these sizes): on the CPU the walker
# + oracle.yolo_nms count at it 66 / 60 / 67 of 135 boxes kept at 96 x 96 and 27 / 29 / 26 of 90 at 96 x 64 (0.006: the cap of 100;
# 0.008: 20).  Every use asserts that rows were found.
LOW = 0.007


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    _lib.require_gpu()
    return runtime


def _cuda(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


@pytest.fixture(scope="module")
def program():
    return TC.tiny_program(NC)


@pytest.fixture(scope="module")
def anchors():
    return TC.tiny_anchors()


_walks = {}


def _reference(program, canvas, batch=BATCH):
    """(weights, images, the walker's tensors): computed once per canvas, shared and left unchanged."""
    hw = (canvas, canvas) if isinstance(canvas, int) else canvas
    if (hw, batch) not in _walks:
        w, x = TC.tiny_inputs(program, batch, hw)
        vals = TC.walk(program, w, x)
        x.setflags(write=False)
        for v in vals.values():
            v.setflags(write=False)
        _walks[(hw, batch)] = (w, x, vals)
    return _walks[(hw, batch)]


def _net(rt, program, weights, batch, canvas, keep=False, setup=None, dtype=None):
    net = rt.Net(program)
    net.load_weights(weights)
    if setup:
        setup(net)
    net.keep_activations(keep)
    net.plan(batch, canvas, dtype)
    return net


# ---------------------------------------------------------------------------------------------- the kernel
POOL_SHAPES = [(3, 12, 8, 32), (2, 13, 13, 512), (2, 13, 7, 96), (1, 1, 1, 32), (1, 2, 2, 32)]
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _pool_on_device(rt, x, stride, fmt):
    """x through ops.maxpool2x2 in the element type `fmt`, into a destination that held 7.0 everywhere -> fp32 NumPy."""
    from yolo_v3_tf2_amd import ops
    xd = _cuda(x).to(TORCH_DT[fmt])
    assert np.array_equal(xd.float().cpu().numpy(), x), "the test data is exact in every element type"
    B, H, W, C = x.shape
    out = torch.full((B, H // stride, W // stride, C), 7.0, dtype=TORCH_DT[fmt], device="cuda")
    got = ops.maxpool2x2(xd, stride, out=out)
    assert got is out
    return out.float().cpu().numpy()


@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_kernel_equals_the_restatement(rt, shape, stride, fmt):
    """ops.maxpool2x2 == maxpool2x2_ref, every element, into a destination that held 7.0 everywhere: the last-row and last-column
    clamps, the 1x1 case, more than one workgroup (13 x 13 x 512), a pixel of 24 vectors (96 channels), in the three element types."""
    if stride == 2 and (shape[1] % 2 or shape[2] % 2):
        from yolo_v3_tf2_amd import ops
        with pytest.raises(rt.Y3Error, match="even extents"):
            ops.maxpool2x2(torch.zeros(shape, device="cuda"), 2)
        return
    for kind in ("normal", "negative", "inf"):
        x = TC.pool_data(shape, kind)
        got = _pool_on_device(rt, x, stride, fmt)
        assert np.array_equal(got, maxpool2x2_ref(x, stride)), (kind, shape, stride, fmt)
        if kind == "negative":
            assert (got < 0).all()          # a maximum that starts from 0 would not be


def test_maxpool_kernel_grid_arithmetic_at_416(rt):
    x = TC.pool_data((2, 416, 416, 32), "normal")
    for stride in (2, 1):
        assert np.array_equal(_pool_on_device(rt, x, stride, "f32"), maxpool2x2_ref(x, stride)), stride


def test_maxpool_kernel_under_graph_capture(rt):
    from yolo_v3_tf2_amd import ops
    x = TC.pool_data((2, 13, 7, 96), "negative")
    xd = _cuda(x)
    outs = [torch.full((2, 13, 7, 96), 7.0, device="cuda"), torch.full((2, 6, 4, 96), 7.0, device="cuda")]
    x2 = _cuda(TC.pool_data((2, 12, 8, 96), "inf"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.maxpool2x2(xd, 1, out=outs[0])
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.maxpool2x2(xd, 1, out=outs[0])
        ops.maxpool2x2(x2, 2, out=outs[1])
    for _ in range(2):
        for o in outs:
            o.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(outs[0].cpu().numpy(), maxpool2x2_ref(x, 1))
        assert np.array_equal(outs[1].cpu().numpy(), maxpool2x2_ref(x2.cpu().numpy(), 2))


# ---------------------------------------------------------------------------------------------- the network in fp32
@pytest.mark.parametrize("canvas", CANVASES)
def test_tiny_every_launch_teacher_forced_and_free_running(rt, program, canvas):
    """With keep_activations: every conv launch against the oracle on the DEVICE's own input (real-width channels read back, the real
    weights) under f32_conv_bar; every pool, up-sample and concat output array_equal to the restatement of the device's own input; the
    free-running head grids within NETWORK_GRID_BAR of the walker; the pad channels of conv0's tensor and of pool 0's exactly zero."""
    from oracle import oracle as O
    w, x, vals = _reference(program, canvas)
    net = _net(rt, program, w, BATCH, canvas, keep=True)
    assert net.heads == 2 and net.lib.y3_net_heads(net._h) == 2
    grids = net.forward(_cuda(x))
    assert len(grids) == 2 and [tuple(g.shape[1:3]) for g in grids] == [tuple(v) if not isinstance(v, int) else (v, v) for v in net.grid_sizes()]
    dev = {program.input_tensor: np.asarray(x)}
    for o, g in zip(program.outputs, grids):
        dev[o] = g.reshape(BATCH, g.shape[1], g.shape[2], -1).cpu().numpy()

    def tensor(t):
        if t not in dev:
            dev[t] = net.read_tensor(t, BATCH).cpu().numpy()
            assert dev[t].shape[-1] == program.tensors[t].channels        # the real channels
        return dev[t]

    kinds = []
    for op in program.ops:
        if isinstance(op, ConvOp):
            ref = oracle_launch(O, op, w, tensor, acc64=True)
            got = tensor(op.dst)
            err, bar = float(np.abs(got - ref).max()), f32_conv_bar(ref)
            assert got.shape == ref.shape and float(np.abs(ref).max()) > 0.05 and err <= bar, (op.conv_index, err, bar)
        else:
            assert isinstance(op, AuxOp)
            kinds.append(op.kind)
            src = [tensor(t) for t in op.inputs]
            ref = {"maxpool_s2": lambda: maxpool2x2_ref(src[0], 2), "maxpool_s1": lambda: maxpool2x2_ref(src[0], 1),
                   "upsample": lambda: O.upsample2x(src[0]), "concat": lambda: O.concat(src[0], src[1])}[op.kind]()
            assert np.array_equal(tensor(op.dst), ref), op
    assert kinds == ["maxpool_s2"] * 5 + ["maxpool_s1", "upsample", "concat"]
    for t in (program.conv_ops()[0].dst, program.conv_ops()[1].src0):
        stored = net._read_tensor("", torch.float32, t, BATCH, stored=True).cpu().numpy()
        assert stored.shape[-1] == 32 and np.array_equal(stored[..., :16], tensor(t)) and not stored[..., 16:].any(), t
        assert np.abs(stored[..., :16]).max() > 0.1
    for o, g in zip(program.outputs, grids):
        err = float(np.abs(g.cpu().numpy() - vals[o].reshape(g.shape)).max())
        print(f"tiny {canvas}: head at 1/{program.tensors[o].div}: free-running deviation {err:.2e} (bar {NETWORK_GRID_BAR:.0e})")
        assert err <= NETWORK_GRID_BAR, (o, err)
    assert net.flops_per_image() == program.flops_per_image(net.canvas)


def test_tiny_forward_invariants(rt, program):
    """Two forwards are bit-equal; image 0 alone equals image 0 of the batch; one and two lanes are bit-equal; a graph replay equals the
    eager call; a plan without keep_activations (buffers reused) equals the one with."""
    w, x, _ = _reference(program, 96, batch=3)
    xd = _cuda(x)
    net = _net(rt, program, w, 3, 96)
    net.set_lanes(1)
    a = [g.clone() for g in net.forward(xd)]
    b = net.forward(xd)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    one = net.forward(xd[:1].contiguous())
    assert all(torch.equal(p[:1], q) for p, q in zip(a, one))
    net.set_lanes(2)
    two = net.forward(xd)
    assert all(torch.equal(p, q) for p, q in zip(a, two))
    kept = _net(rt, program, w, 3, 96, keep=True).forward(xd)
    assert all(torch.equal(p, q) for p, q in zip(a, kept))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net.forward(xd)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net.forward(xd)
    for o in out:
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(a, out))


def test_tiny_low_latency_one_image_stays_within_the_bar(rt, program):
    """set_low_latency acts on the convs by its own rules and never refuses the net; the heads stay within NETWORK_GRID_BAR."""
    w, x, vals = _reference(program, 96)
    net = _net(rt, program, w, 1, 96, setup=lambda n: n.set_low_latency(True))
    grids = net.forward(_cuda(x[:1]))
    print("tiny low latency: K slices per conv", [net.split_k(s) for s in range(len(net.conv_ops))])
    for o, g in zip(program.outputs, grids):
        assert float(np.abs(g.cpu().numpy() - vals[o][:1].reshape(g.shape)).max()) <= NETWORK_GRID_BAR


# ---------------------------------------------------------------------------------------------- detections on two heads
def _composed(rt, net, xd, anchors, M, iou, S):
    grids = net.forward(xd)
    bb, cc, ss = rt.yolo_decode_scores(grids, anchors, NC)
    sel, nv = rt.nms_padded(bb, ss, M, iou, S)
    return grids, (bb, cc, ss), (sel, nv), rt.pack_detections(bb, cc, ss, sel, nv)


@pytest.mark.parametrize("canvas", CANVASES)
def test_tiny_detect_equals_the_calls_composed_by_hand_on_both_routes(rt, program, anchors, canvas):
    """Net.detect on the two-head net == forward + yolo_decode_scores + nms_padded + pack_detections, bit for bit: with the heads
    decoding their own tiles (the default plan: both heads are 1x1 convs of 255 channels on Cin % 64 == 0) and on the composed route
    (keep_activations); forward_decode likewise; N follows the two heads."""
    from yolo_v3_tf2_amd.input_stage import rect_anchors
    w, x, _ = _reference(program, canvas)
    a = anchors if isinstance(canvas, int) else rect_anchors(anchors, max(canvas), canvas)
    xd = _cuda(x)
    want = None
    for keep in (False, True):
        net = _net(rt, program, w, BATCH, canvas, keep=keep)
        grids, (bb, cc, ss), (sel, nv), packed = _composed(rt, net, xd, a, 100, 0.5, LOW)
        N = sum(3 * gh * gw for gh, gw in net._grid_hw())
        assert bb.shape == (BATCH, N, 4) and N == (135 if isinstance(canvas, int) else 90)
        for _ in range(2):
            p2, n2 = net.detect(xd, a, 100, 0.5, LOW)
            assert torch.equal(n2, nv) and torch.equal(p2, packed) and int(nv.min()) > 0
        fb, fc, fs = net.forward_decode(xd, a)
        assert torch.equal(fb, bb) and torch.equal(fc, cc) and torch.equal(fs, ss)
        if want is None:
            want = packed.clone()
        assert torch.equal(packed, want), "the fused-head route and the composed route give the same rows"
    with pytest.raises(rt.Y3Error, match="2 x 3"):
        net.detect(xd, np.zeros((3, 3, 2), np.float32), 100, 0.5, LOW)


def test_tiny_detect_matches_the_oracle_on_the_walkers_grids(rt, program, anchors):
    """Boxes and scores within the existing bars of oracle.yolo_decode / yolo_nms on the walker's grids; the NMS on the device's own
    boxes is bit-exact; every selection difference is attributed to a near-tie (oracle/flip_attribution.py)."""
    from oracle import oracle as O
    from tests.test_gpu_parity import _boxes_close, _selection_explained
    w, x, vals = _reference(program, 96)
    net = _net(rt, program, w, BATCH, 96)
    xd = _cuda(x)
    bb, cc, ss = net.forward_decode(xd, anchors)
    packed, nv = net.detect(xd, anchors, 100, 0.5, LOW)
    gb, gc, gs = bb.cpu().numpy(), cc.cpu().numpy(), ss.cpu().numpy()
    _, _, _, idx = rt.unpack_detections(packed)
    gsel, gnv = idx.cpu().numpy().astype(np.int32), nv.cpu().numpy()
    rb, rc, rs, rsel, rnv = O.yolo_nms(O.yolo_decode(TC.head_grids(program, vals), anchors, NC), 100, 0.5, LOW)
    assert _boxes_close(gb, rb) and float(np.abs(gs - rs).max()) <= 1e-4
    s2, n2 = O.nms_padded(gb, gs, 100, 0.5, LOW)
    assert np.array_equal(n2, gnv) and all(np.array_equal(s2[i, :n2[i]], gsel[i, :n2[i]]) for i in range(BATCH))
    sel_full = np.zeros_like(s2)
    for i in range(BATCH):
        sel_full[i, :gnv[i]] = gsel[i, :gnv[i]]
    _selection_explained((rb, rc, rs, rsel, rnv), (gb, gc, gs, sel_full, gnv), 0.5, LOW)
    assert int(rnv.min()) > 0


def test_tiny_per_class_nms_and_multi_label(rt, program, anchors):
    """Per-class NMS and multi-label detections on the two-head net == nms_padded_per_class_ref / detect_multi_label_ref over the
    device's own decode, bit for bit."""
    from yolo_v3_tf2_amd.multilabel import detect_multi_label_ref
    from yolo_v3_tf2_amd.nms_per_class import nms_padded_per_class_ref
    w, x, _ = _reference(program, 96)
    net = _net(rt, program, w, BATCH, 96)
    xd = _cuda(x)
    grids = [g.clone() for g in net.forward(xd)]
    bb, cc, ss = rt.yolo_decode_scores(grids, anchors, NC)
    net.nms_per_class = True
    packed, nv = net.detect(xd, anchors, 50, 0.3, LOW)
    sel, n = nms_padded_per_class_ref(bb.cpu().numpy(), ss.cpu().numpy(), cc.cpu().numpy(), 50, 0.3, LOW)
    want = rt.pack_detections(bb, cc, ss, _cuda(sel), _cuda(n))
    assert np.array_equal(nv.cpu().numpy(), n) and torch.equal(packed, want) and int(n.min()) > 0
    db, dc, dp = rt.yolo_decode(grids, anchors, NC)
    for per_class in (True, False):
        net.nms_per_class = per_class
        net.multi_label = True
        mp, mn = net.detect(xd, anchors, 50, 0.3, LOW)
        totals = net.multi_label_totals.cpu().numpy()
        net.multi_label = False
        N = bb.shape[1]
        rp, rn, rt_ = detect_multi_label_ref(db.cpu().numpy(), dc.cpu().numpy(), dp.cpu().numpy(), LOW, N, 50, 0.3, per_class=per_class)
        assert np.array_equal(mn.cpu().numpy(), rn) and np.array_equal(mp.cpu().numpy(), rp) and np.array_equal(totals[:BATCH], rt_)
        assert int(rn.min()) > 0 and (rt_ > (ss.cpu().numpy() > LOW).sum(1)).all(), "some box carries more than one label"


# ---------------------------------------------------------------------------------------------- streams
STREAM_S = 160
STREAM_THRESHOLDS = [LOW, 0.008, 0.009]      # at 160 x 160 the CPU counts 100 rows per frame at the first, 10 .. 100 at the second, 0 .. 37 at the third


def _frames():
    rng = np.random.default_rng(96)
    shapes = [(120, 200, 3), (90, 60, 3), (160, 160, 4)]
    return [[rng.integers(0, 256, shapes[k], dtype=np.uint8) for k in ks] for ks in ([0, 1, 2], [2, 1])]


@pytest.mark.parametrize("letterbox", [False, True])
def test_tiny_streams_equal_the_calls_composed_by_hand(rt, program, anchors, letterbox):
    """Five frames in batches of 3 and 2: detect_stream == preprocess_image per slot -> Net.detect (-> unletterbox_detections);
    evaluate_stream's counters == sweep_counters on those rows, its ap=True == match_detections + average_precision on them; loss=True
    on two heads raises."""
    from tests.test_evaluate_gpu import _detect, _ground_truth_from
    from yolo_v3_tf2_amd.evaluate_detections import AP_IOU_THRESHOLDS, average_precision, match_detections, sweep_counters
    w, _ = TC.tiny_inputs(program, 1, (32, 32))
    net = _net(rt, program, w, 3, STREAM_S)
    batches = _frames()
    dets = [_detect(rt, net, b, anchors, STREAM_S, LOW, letterbox) for b in batches]
    got = list(net.detect_stream(batches, anchors, 100, 0.5, LOW, letterbox=letterbox))
    assert len(got) == 2
    for (gp, gn), (wp, wn) in zip(got, dets):
        assert np.array_equal(gn, wn) and np.array_equal(gp, wp) and int(wn.min()) > 0
    rng = np.random.default_rng(7)
    gts = [_ground_truth_from(*d, rng, first=3 * i) for i, d in enumerate(dets)]
    G = max(len(c) for g in gts for _, c in g)
    counters, records, totals = 0, [], 0
    for (packed, nv), gt in zip(dets, gts):
        gb, gc, cnt = rt.pack_ground_truth(gt, G)
        counters = counters + sweep_counters(packed, nv, gb, gc, cnt, NC, 0.5, STREAM_THRESHOLDS)
        r, t = match_detections(packed, nv, gb, gc, cnt, NC, AP_IOU_THRESHOLDS)
        records.append(r)
        totals = totals + t
    want_ap = average_precision(np.concatenate(records), totals, NC, len(AP_IOU_THRESHOLDS))
    plain = net.evaluate_stream(batches, gts, anchors, 100, 0.5, STREAM_THRESHOLDS, NC, letterbox=letterbox)
    assert np.array_equal(plain, counters) and plain.any()
    c2, ap = net.evaluate_stream(batches, gts, anchors, 100, 0.5, STREAM_THRESHOLDS, NC, letterbox=letterbox, ap=True)
    assert np.array_equal(c2, counters)
    assert np.array_equal(ap["ap"], want_ap["ap"], equal_nan=True) and ap["mAP"] == want_ap["mAP"] and (ap["images"], ap["errors"]) == (5, 0)
    if not letterbox:
        with pytest.raises(rt.Y3Error, match="three-head"):
            net.evaluate_stream(batches, gts, anchors, 100, 0.5, STREAM_THRESHOLDS, NC, loss=True)


def test_tiny_detect_stream_with_tiles_equals_the_composed_calls(rt, program, anchors):
    """Sliced inference on the two-head net: detect_stream with Net.tiles == pack, preprocess_tiles, Net.detect on the tile batch and
    merge_tile_detections made by hand (the composition of tests/test_tiles_gpu.py), every word; per-class NMS with a merge threshold
    of its own as well."""
    from tests.test_tiles_gpu import NET_IOU, NET_M, NET_S, TILES, _composed, _same, _stream_batches
    w, _ = TC.tiny_inputs(program, 1, (32, 32))
    net = _net(rt, program, w, 3, NET_S)
    batches = _stream_batches()[:2]
    for per_class, merge_iou in ((False, None), (True, 0.3)):
        net.nms_per_class, net.tiles, net.merge_iou_threshold = per_class, TILES, merge_iou
        rows = [tuple(np.array(a) for a in r) for r in net.detect_stream(batches, anchors, NET_M, NET_IOU, LOW, letterbox=True)]
        assert len(rows) == 2
        for frames, got in zip(batches, rows):
            want, _, T = _composed(rt, net, frames, anchors, True, merge_iou=NET_IOU if merge_iou is None else merge_iou, score=LOW)
            assert T == 7
            _same(got, want)
            assert (got[1] > 0).all()


def test_tiny_through_the_drop_in_layer(rt, program, anchors):
    """core.parse_model.YoloModel + inference.DetectModel on the tiny program and its six anchors == Net.detect's rows."""
    from yolo_v3_tf2_amd.core.parse_model import YoloModel
    from yolo_v3_tf2_amd.inference import DetectModel
    w, x, _ = _reference(program, 96)
    m = YoloModel(program)
    m.set_weights_dict(w)
    gb, gc, gs, gsel, gnv = DetectModel(m, anchors, NC, 100, 0.5, LOW).predict(np.array(x))
    net = _net(rt, program, w, BATCH, 96)
    packed, nv = net.detect(_cuda(x), anchors, 100, 0.5, LOW)
    boxes, scores, classes, idx = rt.unpack_detections(packed)
    assert np.array_equal(gnv, nv.cpu().numpy()) and gb.shape == (BATCH, 135, 4)
    for i in range(BATCH):
        n = int(gnv[i])
        assert n > 0 and np.array_equal(gsel[i, :n], idx[i, :n].cpu().numpy())
        assert np.array_equal(gb[i][gsel[i, :n]], boxes[i, :n].cpu().numpy()) and np.array_equal(gs[i][gsel[i, :n]], scores[i, :n].cpu().numpy())


def test_tiny_inference_driver_reads_the_tiny_config(rt, program, anchors, tmp_path):
    """Inference()(**config/detect_config_tiny.yaml) -- the tiny model.yaml and the six-row anchors file -- gives the detections of
    Net.detect on the same image, bit for bit."""
    import os
    import yaml
    from yolo_v3_tf2_amd.core.utils import load_image_u8
    from yolo_v3_tf2_amd.inference import Inference
    S = 160
    cfg = yaml.safe_load(open(os.path.join(TC.ROOT, "config/detect_config_tiny.yaml")))
    cfg.update(image_size=S, nms_score_threshold=LOW, output_dir=str(tmp_path / "out"), input_weights_path=None,
               **{k: os.path.join(TC.ROOT, cfg[k]) for k in ("model_config_file", "anchors_file", "image_file_path", "classes_name_file")})
    w, _ = TC.tiny_inputs(program, 1, (32, 32))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        results = Inference()(**cfg, weights=w)
    finally:
        os.chdir(cwd)
    assert len(results) == 1
    bboxes, classes, scores, _ = results[0]
    batch = torch.empty((1, S, S, 3), dtype=torch.float32, device="cuda")
    rt.preprocess_image(torch.from_numpy(load_image_u8(cfg["image_file_path"])).cuda(), batch, 0)
    net = _net(rt, program, w, 1, S)
    packed, nv = net.detect(batch, anchors, cfg["yolo_max_boxes"], cfg["nms_iou_threshold"], LOW)
    n = int(nv[0])
    db, ds, dc, _ = (t[0, :n].cpu().numpy() for t in rt.unpack_detections(packed))
    assert n > 0 and len(bboxes) == n
    assert np.array_equal(np.asarray(bboxes, np.float32), db) and np.array_equal(np.asarray(scores, np.float32), ds)
    assert np.array_equal(np.asarray(classes).astype(np.int64), dc.astype(np.int64))


def test_tiny_evaluate_driver_on_device_equals_the_host_route(rt, program, tmp_path):
    """evaluate_yolov3.evaluate(on_device=True) on the tiny model config == the host route in every counter."""
    import os
    from tests.helpers import jpeg_bytes
    from tests.test_evaluate_gpu import _same_results
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev
    from yolo_v3_tf2_amd.core import load_tfrecords as m
    names = [ln.strip() for ln in open(os.path.join(TC.ROOT, "datasets/coco2012/coco.names")) if ln.strip()]
    rng = np.random.default_rng(23)
    payloads = []
    for i in range(4):
        lo = (rng.random((2, 2)) * 0.5).astype(np.float32)
        hi = lo + 0.3
        payloads.append(m.make_example({"image/encoded": jpeg_bytes(rng, 60, 75),
                                        "image/object/class/text": [names[(7 * i + j) % NC].encode() for j in range(2)],
                                        "image/object/bbox/xmin": lo[:, 0], "image/object/bbox/ymin": lo[:, 1],
                                        "image/object/bbox/xmax": hi[:, 0], "image/object/bbox/ymax": hi[:, 1]}))
    d = tmp_path / "set"
    d.mkdir()
    m.write_records(str(d / "set.tfrec"), payloads)
    cfg = dict(tfrecords_dir=str(d), image_size=96, batch_size=2, yolo_max_boxes=100, nms_iou_threshold=0.5,
               classes_name_file=os.path.join(TC.ROOT, "datasets/coco2012/coco.names"), anchors_file=TC.TINY_ANCHORS,
               model_config_file=TC.TINY_MODEL)
    w, _ = TC.tiny_inputs(program, 1, (32, 32))
    thresholds = [0.006, LOW]      # both inside the score range of these frames: rows at either
    host = ev.evaluate(cfg, thresholds, evaluate_iou_threshold=0.1, weights=w)
    dev = ev.evaluate(cfg, thresholds, evaluate_iou_threshold=0.1, weights=w, on_device=True)
    _same_results(dev, host)
    c = dev[0][3]
    assert c["examples"] == 4 and c["gts"].sum() == 8 and c["preds"].sum() > 0
    assert 0 < dev[1][3]["preds"].sum() <= c["preds"].sum()


# ---------------------------------------------------------------------------------------------- a 16-bit net with pools
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_pools_in_a_16_bit_net(rt, mode):
    """3 -> 32, pool, 32 -> 64, pool, 64 -> 128, pool (stride 1), two heads, in a bf16 and an fp16 plan with keep_activations.  Each
    pool output equals the restatement of the device's stored input, bit for bit (the conversion to fp32 is exact).  Each conv against
    the oracle on the device's own stored input, weights rounded to the format (the Cin = 3 layer: fp32 weights): an fp32 head output
    under bf16_tile_bar (fp16: under the tighter f32_conv_bar, the bar tests/test_f16_tile_matrix_gpu.py holds such an output to); a
    stored output against the oracle's value rounded to the format within one unit of the format's last place + 1e-5 of the tensor's
    magnitude -- the teacher-forced rule of the 16-bit suites: bf16_tile_bar speaks of an fp32 output, and one rounding of a stored
    value is already 2^-9 of it."""
    from oracle import oracle as O
    from tests.f16_oracle import f16_emulation, f16_ulp_elem, round_f16
    from tests.test_odd_widths_gpu import _bf16_ulp_elem
    p, pools = TC.pool_net_program()
    assert p.stored == [t.channels for t in p.tensors] and len(p.outputs) == 2
    B, canvas = 2, (24, 16)
    w, x = TC.tiny_inputs(p, B, canvas)
    net = _net(rt, p, w, B, canvas, keep=True, dtype=_lib.Y3_DTYPE_BF16 if mode == "bf16" else _lib.Y3_DTYPE_F16)
    grids = net.forward(_cuda(x))
    assert [tuple(g.shape) for g in grids] == [(B, 6, 4, 64), (B, 6, 4, 128)]
    dev = {p.input_tensor: x}
    for o, g in zip(p.outputs, grids):
        dev[o] = g.cpu().numpy()

    def tensor(t):
        if t not in dev:
            dev[t] = net.read_tensor(t, B).cpu().numpy()
        return dev[t]

    rnd, ulp = (O.round_bf16, _bf16_ulp_elem) if mode == "bf16" else (round_f16, f16_ulp_elem)
    npool = 0
    for op in p.ops:
        if isinstance(op, AuxOp):
            src = tensor(op.inputs[0])
            assert np.array_equal(rnd(src), src), "what is stored is 16-bit"
            assert np.array_equal(tensor(op.dst), maxpool2x2_ref(src, 2 if op.kind == "maxpool_s2" else 1)), op
            npool += 1
            continue
        w16 = op.cin != 3
        if mode == "f16":
            with f16_emulation():
                ref = oracle_launch(O, op, w, tensor, acc64=True, bf16_weights=w16)
        else:
            ref = oracle_launch(O, op, w, tensor, acc64=True, bf16_weights=w16)
        got = tensor(op.dst)
        assert float(np.abs(ref).max()) > 0.1
        if op.dst in p.outputs:
            err, bar = float(np.abs(got - ref).max()), bf16_tile_bar(ref) if mode == "bf16" else f32_conv_bar(ref)
            assert err <= bar, (mode, op.conv_index, err, bar)
        else:
            exp = rnd(ref)
            diff = np.abs(got.astype(np.float64) - exp.astype(np.float64))
            assert (diff <= ulp(got, exp) + 1e-5 * float(np.abs(exp).max())).all(), (mode, op.conv_index)
    assert npool == 3 and [o.dst for o in p.ops if isinstance(o, AuxOp)] == pools


# ---------------------------------------------------------------------------------------------- refusals
def test_plan_refuses_pools_in_the_plane_split_and_int8_modes(rt):
    """F32X3, F32X2 and I8 on a net that holds a pool: Y3_ERR_INVALID naming the op, nothing planned; the same net then plans and runs
    in fp32."""
    p, _ = TC.pool_net_program()
    w, x = TC.tiny_inputs(p, 1, (16, 16))
    net = rt.Net(p)
    net.load_weights(w)
    for dt in (_lib.Y3_DTYPE_F32X3, _lib.Y3_DTYPE_F32X2, _lib.Y3_DTYPE_I8):
        with pytest.raises(rt.Y3Error, match=r"y3_net_plan: the net holds a max-pool op \(Y3_AUX_MAXPOOL2X2") as e:
            net.plan(1, 16, dt)
        assert "(-1)" in str(e.value) and net.max_batch == 0
        assert net.lib.y3_net_flops_per_image(net._h) == 0.0, "no plan was made"
    net.plan(1, 16)
    grids = net.forward(_cuda(x))
    vals = TC.walk(p, w, x)
    for o, g in zip(p.outputs, grids):
        assert float(np.abs(g.cpu().numpy() - vals[o]).max()) <= NETWORK_GRID_BAR


def test_real_tiny_in_bf16_is_refused_by_the_existing_message(rt, program):
    w, _ = TC.tiny_inputs(program, 1, (32, 32))
    net = rt.Net(program)
    net.load_weights(w)
    for dt, name in ((_lib.Y3_DTYPE_BF16, "bf16"), (_lib.Y3_DTYPE_F16, "fp16")):
        with pytest.raises(rt.Y3Error, match=rf"conv 1 \(Cin 32, c0 -1, Cout 32\) has no {name} tile"):
            net.plan(1, 96, dt)
    net.plan(1, 96)
    assert len(net.forward(torch.zeros((1, 96, 96, 3), device="cuda"))) == 2
