"""The network on the device at class counts other than 80 (tests/class_count_cases.py; the 80-class case is the rest of the suite).

Which head kernel runs follows from the rule of heads_can_decode (csrc/y3_forward.cpp; class_count_cases.head_route): the three head
convs have 3 * (5 + nc) channels; only when those pad to exactly 256 (nc = 70 and 79 here: 225 and 252 channels) do forward_decode /
detect run the fused head, which decodes its own tile and never stores the grid.  Every other class count (1, 3, 7, 37: 18, 24,
36, 126 channels in cout_pad 32 / 32 / 64 / 128; 81: 258 channels in cout_pad 288) takes the composed route: an ordinary 1x1 conv with
bias that stores a ragged, even-width fp32 grid, then the stand-alone decode.  A plan that keeps its activations (the teacher-forced
tests) and net.forward() run the ordinary conv at every class count, so nc = 70 / 79 exercise both kernels.

Bars are the ones the 80-class tests use, through the same code (tests/helpers.py: check_f32_conv, bf16_tile_bar, NETWORK_GRID_BAR;
tests/test_i8_gpu.py::_check_convs, bit-exact)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import class_count_cases as K  # noqa: E402
from tests.f16_oracle import f16_emulation  # noqa: E402
from tests.helpers import NETWORK_GRID_BAR, bf16_tile_bar, check_f32_conv, jpeg_bytes, oracle_launch  # noqa: E402
from yolo_v3_tf2_amd import _lib  # noqa: E402

CLASS_COUNTS = (1, 3, 7, 37, 70, 79, 81)
DTYPES = {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16, "f16": _lib.Y3_DTYPE_F16, "i8": _lib.Y3_DTYPE_I8,
          "f32x3": _lib.Y3_DTYPE_F32X3, "f32x2": _lib.Y3_DTYPE_F32X2}
SCORE_THRESHOLD = 0.005      # synthetic heads: objectness bias -4, scores of 0.005 ... 0.09 (measured on the oracle)


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the shared inputs are read-only


def _net(rt, nc, mode, B, canvas, keep=False):
    """A net of K.program(nc) planned in `mode`; an int8 plan is calibrated on the two 64 x 64 images of the case first."""
    net = rt.Net(K.program(nc))
    net.load_weights(K.weights(nc))
    scales = net.calibrate_i8(_cuda(K.images())) if mode == "i8" else None
    net.keep_activations(keep)
    net.plan(B, canvas, DTYPES[mode])
    return net, scales


# ---------------------------------------------------------------------------------------------- heads, teacher-forced
@pytest.mark.parametrize("mode", list(DTYPES))
@pytest.mark.parametrize("nc", CLASS_COUNTS)
def test_head_convs_teacher_forced(rt, nc, mode):
    """Each head conv restated by the oracle from the conv's own input tensor on the device, under the mode's per-layer bar."""
    from oracle import oracle as O
    p, w = K.program(nc), K.weights(nc)
    x, _ = K.oracle_grids(nc)
    B = x.shape[0]
    net, scales = _net(rt, nc, mode, B, K.S, keep=True)
    grids = net.forward(_cuda(x))
    torch.cuda.synchronize()
    heads = K.head_ops(p)
    for g, o, s in zip(grids, heads, (2, 4, 8)):
        assert tuple(g.shape) == (B, s, s, 3, 5 + nc) and bool(torch.isfinite(g).all())
    if mode == "i8":
        from tests.test_i8_gpu import _check_convs
        first = min(net.conv_ops.index(o) for o in heads)
        assert net.i8_first_conv() == 9 and first == 58
        assert _check_convs(net, p, w, scales, B, grids, first) == len(net.conv_ops) - first      # convs 58 .. 74, the heads among them
        print(f"class-count heads nc={nc} i8 ({K.head_route(nc)} route): convs 58..74 bit-exact")
        return
    outs = {t: g.cpu().numpy().reshape(B, g.shape[1], g.shape[2], -1) for t, g in zip(p.outputs, grids)}
    tensor = lambda t: net.read_tensor(t, B).cpu().numpy()  # noqa: E731
    for o in heads:
        if mode == "f16":
            with f16_emulation():
                y = oracle_launch(O, o, w, tensor, acc64=True, bf16_weights=True)
        else:
            y = oracle_launch(O, o, w, tensor, acc64=True, bf16_weights=(mode == "bf16"))
        got = outs[o.dst]
        assert got.shape == y.shape == (B, x.shape[1] // o.out_div, x.shape[2] // o.out_div, 3 * (5 + nc))
        print(f"class-count heads nc={nc} {mode} ({K.head_route(nc)} route) conv{o.conv_index} cout {o.cout}: "
              f"deviation {float(np.abs(got - y).max()):.3e}", end=" ")      # printed before it is asserted
        _, bar = check_f32_conv(got, y, (nc, mode, o.conv_index))
        print(f"bar {bar:.3e}")
        assert float(np.abs(y).max()) > 0.5      # not a comparison of two empty buffers


# ---------------------------------------------------------------------------------------------- free running
@pytest.mark.parametrize("nc", CLASS_COUNTS)
def test_network_grids_match_oracle_at_class_count(rt, nc):
    x, ref = K.oracle_grids(nc)
    net, _ = _net(rt, nc, "f32", x.shape[0], K.S)
    got = net.forward(_cuda(x))
    torch.cuda.synchronize()
    for r, g in zip(ref, got):
        assert tuple(g.shape) == r.shape
        err = float(np.abs(g.cpu().numpy() - r).max())
        print(f"class-count free-running nc={nc} f32 grid {r.shape[1]}: deviation {err:.3e} bar {NETWORK_GRID_BAR:.0e}")
        assert err <= NETWORK_GRID_BAR


# ---------------------------------------------------------------------------------------------- routes
def _composed(rt, net, x, anchors, nc):
    """forward -> yolo_decode_scores -> nms_padded -> pack_detections, the four calls one by one."""
    grids = net.forward(x)
    bb, cc, ss = rt.yolo_decode_scores(grids, anchors, nc)
    sel, nv = rt.nms_padded(bb, ss, 100, 0.5, SCORE_THRESHOLD)
    return bb, cc, ss, rt.pack_detections(bb, cc, ss, sel, nv), nv


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16", "i8"])
@pytest.mark.parametrize("nc", CLASS_COUNTS)
def test_routes_equal_the_composed_pipeline(rt, anchors, nc, mode):
    """forward_decode == forward + yolo_decode_scores and detect == the four-call composition, bit for bit, twice, with one and
    two lanes (B = 3: unequal parts), on a square and a (64, 96) plan; image 0 alone == image 0 of the batch.  nc = 70 / 79 run the
    fused heads here, the others the composed route (module docstring)."""
    B = 3
    net, _ = _net(rt, nc, mode, B, K.S)
    for canvas in (K.S, (K.S, 96)):
        hw = (canvas, canvas) if isinstance(canvas, int) else canvas
        x = _cuda(K.images(B, hw))
        net.plan(B, canvas, DTYPES[mode])
        for lanes in (1, 2):
            net.set_lanes(lanes)
            bb, cc, ss, want, nv = _composed(rt, net, x, anchors, nc)
            assert tuple(bb.shape) == (B, 3 * sum(gh * gw for gh, gw in net._grid_hw()), 4)
            assert int(nv.min()) > 0 and int(cc.max()) < nc and int(cc.min()) >= 0
            for _ in range(2):
                fb, fc, fs = net.forward_decode(x, anchors)
                packed, nv2 = net.detect(x, anchors, 100, 0.5, SCORE_THRESHOLD)
                torch.cuda.synchronize()
                assert torch.equal(fb, bb) and torch.equal(fc, cc) and torch.equal(fs, ss), (nc, mode, canvas, lanes, "forward_decode")
                assert torch.equal(nv2, nv) and torch.equal(packed, want), (nc, mode, canvas, lanes, "detect")
            x0 = x[0:1].contiguous()
            fb0, fc0, fs0 = net.forward_decode(x0, anchors)
            p0, n0 = net.detect(x0, anchors, 100, 0.5, SCORE_THRESHOLD)
            torch.cuda.synchronize()
            assert torch.equal(fb0, bb[0:1]) and torch.equal(fc0, cc[0:1]) and torch.equal(fs0, ss[0:1]), (nc, mode, canvas, lanes, "image 0 alone")
            assert torch.equal(n0, nv[0:1]) and torch.equal(p0, want[0:1]), (nc, mode, canvas, lanes, "detect of image 0 alone")


@pytest.mark.parametrize("nc,mode", [(79, "bf16"), (7, "f32")], ids=["fused-nc79-bf16", "composed-nc7-f32"])
def test_detect_replayed_from_a_graph_at_class_count(rt, anchors, nc, mode):
    """detect captured into a graph (two lanes: forked streams inside the capture) and replayed == the eager result."""
    B = 3
    assert K.head_route(nc) == ("fused" if nc == 79 else "composed")
    net, _ = _net(rt, nc, mode, B, K.S)
    net.set_lanes(2)
    x = _cuda(K.images(B))
    want, nv = net.detect(x, anchors, 100, 0.5, SCORE_THRESHOLD)
    torch.cuda.synchronize()
    want, nv = want.clone(), nv.clone()
    assert int(nv.min()) > 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net.detect(x, anchors, 100, 0.5, SCORE_THRESHOLD)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gp, gn = net.detect(x, anchors, 100, 0.5, SCORE_THRESHOLD)
    for _ in range(2):
        gp.zero_()
        gn.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(gn, nv) and torch.equal(gp, want)


# ---------------------------------------------------------------------------------------------- forced tiles on the heads
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("nc", [1, 7, 37])
def test_every_fitting_tile_on_the_head_convs(rt, nc, mode):
    """Every built tile that fits a head conv (the rule tests/test_tile_setters_gpu.py restates, which the setter must agree with)
    forced on it: the ragged, even-width fp32 store of every tile.  fp32: the same bits as the heuristic tile.  bf16: the bar of
    test_bf16_every_tile against the oracle's restatement of the head conv from its own device input."""
    from oracle import oracle as O
    from tests.test_tile_matrix_gpu import MODES
    from tests.test_tile_setters_gpu import _accepts
    dtype, table, tiles, setter, _ = MODES[mode]
    p, w = K.program(nc), K.weights(nc)
    x, _ = K.oracle_grids(nc)
    B = x.shape[0]
    xd = _cuda(x)
    net, _ = _net(rt, nc, mode, B, K.S, keep=True)
    base = [g.clone() for g in net.forward(xd)]
    torch.cuda.synchronize()
    heads = K.head_ops(p)
    slots = [net.conv_ops.index(o) for o in heads]
    ref = None
    if mode == "bf16":
        tensor = lambda t: net.read_tensor(t, B).cpu().numpy()  # noqa: E731
        ref = [oracle_launch(O, o, w, tensor, acc64=True, bf16_weights=True) for o in heads]
    ran = 0
    for tile in tiles:
        forced = []
        for slot, o in zip(slots, heads):
            fits = _accepts(_lib, mode, p, net.conv_ops, o, tile)
            try:
                getattr(net, setter)(slot, tile)
                took = True
            except rt.Y3Error as e:
                assert "tile does not" in str(e), str(e)
                took = False
            assert took == fits, (nc, mode, tile, o.conv_index, "the setter and the fitting rule disagree")
            if took:
                forced.append(o)
        if forced:
            net.plan(B, K.S, dtype)
            got = net.forward(xd)
            torch.cuda.synchronize()
            for k, o in enumerate(heads):
                if o not in forced:
                    continue
                ran += 1
                if mode == "f32":
                    assert torch.equal(got[k], base[k]), (nc, tile, o.conv_index, float((got[k] - base[k]).abs().max()))
                else:
                    g = got[k].cpu().numpy().reshape(ref[k].shape)
                    err = float(np.abs(g - ref[k]).max())
                    assert err <= bf16_tile_bar(ref[k]), (nc, tile, o.conv_index, err, bf16_tile_bar(ref[k]))
        for slot in slots:
            getattr(net, setter)(slot, -1)
    print(f"class-count forced tiles nc={nc} {mode}: {ran} (head conv, tile) launches")
    # not vacuous: every head took a tile (nc = 1 and 3 pad to 32 channels, which only the 32-wide tiles divide)
    assert ran == sum(_accepts(_lib, mode, p, net.conv_ops, o, t) for o in heads for t in tiles) >= 3


# ---------------------------------------------------------------------------------------------- drivers
NAMES3 = ("circle", "square", "triangle")


def _names_file(tmp_path):
    path = tmp_path / "three.names"
    path.write_text("".join(n + "\n" for n in NAMES3))
    return str(path)


def test_inference_driver_with_three_classes(rt, anchors, tmp_path):
    """Inference()(**yaml) with a three-line class-names file: the detections of Net.detect on the same image, bit for bit."""
    import yaml
    from yolo_v3_tf2_amd.core.utils import load_image_u8
    from yolo_v3_tf2_amd.inference import Inference
    cfg = yaml.safe_load(open(os.path.join(K.ROOT, "config/detect_config_coco.yaml")))
    cfg.update(image_size=K.S, nms_score_threshold=SCORE_THRESHOLD, classes_name_file=_names_file(tmp_path),
               output_dir=str(tmp_path / "out"), model_config_file=K.MODEL, input_weights_path=None,
               anchors_file=os.path.join(K.ROOT, cfg["anchors_file"]), image_file_path=os.path.join(K.ROOT, cfg["image_file_path"]))
    ypath = tmp_path / "detect3.yaml"
    ypath.write_text(yaml.safe_dump(cfg))
    cfg = yaml.safe_load(ypath.read_text())
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        results = Inference()(**cfg, weights=K.weights(3))
    finally:
        os.chdir(cwd)
    assert len(results) == 1
    bboxes, classes, scores, names = results[0]
    batch = torch.empty((1, K.S, K.S, 3), dtype=torch.float32, device="cuda")
    rt.preprocess_image(torch.from_numpy(load_image_u8(cfg["image_file_path"])).cuda(), batch, 0)
    net, _ = _net(rt, 3, "f32", 1, K.S)
    packed, nv = net.detect(batch, anchors, cfg["yolo_max_boxes"], cfg["nms_iou_threshold"], SCORE_THRESHOLD)
    torch.cuda.synchronize()
    n = int(nv[0])
    db, ds, dc, _ = (t[0, :n].cpu().numpy() for t in rt.unpack_detections(packed))
    assert n > 0 and len(bboxes) == n
    assert np.array_equal(np.asarray(bboxes, np.float32), db) and np.array_equal(np.asarray(scores, np.float32), ds)
    assert np.array_equal(np.asarray(classes).astype(np.int64), dc.astype(np.int64)) and int(dc.max()) < 3
    assert list(names) == [NAMES3[int(c)] for c in dc]
    lines = open(os.path.join(cfg["output_dir"], "detect.txt")).read().strip().splitlines()
    assert len(lines) == 1 and lines[0].count("%") == n


def test_evaluate_driver_with_three_classes(rt, tmp_path):
    """evaluate(on_device=True) == the host route in every counter, on four 64 x 64 images of two boxes with a three-line names file."""
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev
    from yolo_v3_tf2_amd.core import load_tfrecords as m
    from tests.test_evaluate_gpu import _same_results
    rng = np.random.default_rng(23)
    payloads = []
    for i in range(4):
        lo = (rng.random((2, 2)) * 0.5).astype(np.float32)
        hi = lo + 0.3
        payloads.append(m.make_example({"image/encoded": jpeg_bytes(rng, 60, 75),
                                        "image/object/class/text": [NAMES3[(i + j) % 3].encode() for j in range(2)],
                                        "image/object/bbox/xmin": lo[:, 0], "image/object/bbox/ymin": lo[:, 1],
                                        "image/object/bbox/xmax": hi[:, 0], "image/object/bbox/ymax": hi[:, 1]}))
    d = tmp_path / "set"
    d.mkdir()
    m.write_records(str(d / "set.tfrec"), payloads)
    cfg = dict(tfrecords_dir=str(d), image_size=K.S, batch_size=2, yolo_max_boxes=100, nms_iou_threshold=0.5,
               classes_name_file=_names_file(tmp_path), anchors_file=os.path.join(K.ROOT, "datasets/coco2012/anchors.txt"),
               model_config_file=K.MODEL)
    thresholds = [0.004, 0.008]
    host = ev.evaluate(cfg, thresholds, evaluate_iou_threshold=0.1, weights=K.weights(3))
    dev = ev.evaluate(cfg, thresholds, evaluate_iou_threshold=0.1, weights=K.weights(3), on_device=True)
    _same_results(dev, host)
    c = dev[0][3]
    assert c["examples"] == 4 and c["gts"].sum() == 8 and c["preds"].sum() > 0 and len(c["gts"]) == 3
    assert 0 < dev[1][3]["preds"].sum() <= c["preds"].sum()
