"""The fused stem of YOLOv3-tiny on the GPU (csrc/conv_tiny_stem.hip; include/y3.h, y3_net_set_tiny_stem_fusion): pool 1's tensor read
through identity heads against the chains of tests/tiny_stem_cases.py in fp32, bf16 and fp16; real tiny planned in bf16 and fp16 with every
launch behind the stem teacher-forced; the invariants of a forward; what the switch does and does not act on; a stream and the evaluate
driver in bf16.  The caps and their basis: tests/tiny_stem_cases.py, tests/test_tiny_stem_host.py."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import tiny_cases as TC  # noqa: E402
from tests import tiny_stem_cases as C  # noqa: E402
from tests.helpers import bf16_tile_bar, f32_conv_bar, oracle_launch  # noqa: E402
from yolo_v3_tf2_amd import _lib  # noqa: E402
from yolo_v3_tf2_amd.graph import AuxOp, ConvOp  # noqa: E402
from yolo_v3_tf2_amd.maxpool import maxpool2x2_ref  # noqa: E402

NC = 80
LOW = 0.007          # inside the score range of the random-init tiny heads (tests/test_tiny_gpu.py)
DT = {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16, "f16": _lib.Y3_DTYPE_F16}


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    _lib.require_gpu()
    return runtime


@pytest.fixture(scope="module")
def tiny():
    return TC.tiny_program(NC)


def _cuda(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _net(rt, program, weights, batch, canvas, fmt="f32", fused=True, keep=False, setup=None):
    net = rt.Net(program)
    net.load_weights(weights)
    if fused is not None:          # None: the setter is never called
        net.set_tiny_stem_fusion(fused)
    if setup:
        setup(net)
    net.keep_activations(keep)
    net.plan(batch, canvas, DT[fmt])
    return net


def _pool1_through_the_heads(rt, case, variant, fmt, fused=True):
    """pool 1's stored values of a case, read through the two identity heads (which must agree and carry zeros behind channel 31)."""
    p, w, x, _ = C.stem_inputs(case, variant)
    (H, W), B = C.CASES[case]
    net = _net(rt, p, w, B, (H, W), fmt, fused)
    assert net.tiny_stem_fused == int(bool(fused))
    a, b = (g.cpu().numpy() for g in net.forward(_cuda(x)))
    assert np.array_equal(a, b) and not a[..., 32:].any()
    return np.ascontiguousarray(a[..., :32])


# ---------------------------------------------------------------------------------------------- 1. fp32
@pytest.mark.parametrize("case,variant", C.GPU_CASES)
def test_fp32_fused_and_unfused_within_the_conv_bar_of_the_double_sum_chain(rt, case, variant):
    """Pool 1's values through the identity heads against the double-sum chain, with the switch on and with it off, under f32_conv_bar (the
    bar of one fp32 conv launch of K <= 4608; both Ks here are far below).  Observed on the MI355X, the largest deviation as a fraction of
    the bar, fused / unfused: s32_b1 0.026 / 0.020, r64x96_b3 0.031 / 0.031, r160x128_b2 0.029 / 0.024, signs 0.039 / 0.036, img255 0.027 /
    0.027 (profiles/tiny_stem.txt)."""
    ref = C.references(case, variant)["f64"]
    bar = f32_conv_bar(ref)
    for fused in (True, False):
        got = _pool1_through_the_heads(rt, case, variant, "f32", fused)
        err = float(np.abs(got - ref).max())
        print(f"tiny stem fp32 {case} / {variant} {'fused' if fused else 'unfused'}: {err:.3e} = {err / bar:.4f} of the bar {bar:.3e}")
        assert got.shape == ref.shape and err <= bar, (case, variant, fused, err, bar)
    if variant == "signs":
        assert float((got < 0).mean()) > 0.9


# ---------------------------------------------------------------------------------------------- 2. bf16 and fp16
@pytest.mark.parametrize("fmt", C.FORMATS)
@pytest.mark.parametrize("case,variant", C.GPU_CASES)
def test_16_bit_fused_within_the_caps_of_the_rounded_double_sum_chain(rt, case, variant, fmt):
    ref = C.references(case, variant)[fmt]
    got = _pool1_through_the_heads(rt, case, variant, fmt)
    differ, beyond, worst = C.compare(fmt, got, ref)
    print(f"tiny stem {fmt} {case} / {variant}: differ {differ:.4e} (cap {C.CAPS[fmt][0]:.4e})  beyond one ulp {beyond:.4e} (cap {C.CAPS[fmt][1]:.4e})  "
          f"worst {worst:.3f} of ulp + 2^{-8 if fmt == 'bf16' else -11} of the magnitude")
    assert got.shape == ref.shape
    assert differ <= C.CAPS[fmt][0] and beyond <= C.CAPS[fmt][1], (fmt, case, variant, differ, beyond)
    assert worst <= 1.0, (fmt, case, variant, worst)
    if variant == "signs":
        assert float((got < 0).mean()) > 0.9, "whole pooling windows are negative: no maximum started from 0, no pool ran before leaky"


# ---------------------------------------------------------------------------------------------- 3. real tiny in the 16-bit modes
def _rounding(fmt):
    from oracle import oracle as O
    from tests.f16_oracle import round_f16
    return (O.round_bf16, C.bf16_ulp_elem) if fmt == "bf16" else (round_f16, C.ULP["f16"])


def _teacher_forced_head(fmt, op, w, tensor):
    from oracle import oracle as O
    from tests.f16_oracle import f16_emulation
    if fmt == "f16":
        with f16_emulation():
            return oracle_launch(O, op, w, tensor, acc64=True, bf16_weights=True)
    return oracle_launch(O, op, w, tensor, acc64=True, bf16_weights=True)


@pytest.mark.parametrize("fmt", C.FORMATS)
@pytest.mark.parametrize("canvas", [96, (96, 64)])
def test_real_tiny_plans_and_runs_in_16_bit_with_the_switch(rt, tiny, canvas, fmt):
    """plan succeeds and tiny_stem_fused is 1; with keep_activations every conv behind the stem against the oracle on the device's own
    stored input (weights rounded to the format): a stored output within one ulp + 1e-5 of the magnitude of the rounded oracle value, an
    fp32 head under bf16_tile_bar (fp16: f32_conv_bar) -- the bars of tests/test_tiny_gpu.py's 16-bit pool net; every pool, up-sample and
    concat array_equal to its restatement; read_tensor on a tensor inside the stem raises and names the switch."""
    from oracle import oracle as O
    B = 2
    hw = (canvas, canvas) if isinstance(canvas, int) else canvas
    w, x = TC.tiny_inputs(tiny, B, hw)
    net = _net(rt, tiny, w, B, canvas, fmt, keep=True)
    assert net.tiny_stem_fused == 1
    grids = net.forward(_cuda(x))
    dev = {tiny.input_tensor: x}
    for o, g in zip(tiny.outputs, grids):
        dev[o] = g.reshape(B, g.shape[1], g.shape[2], -1).cpu().numpy()

    def tensor(t):
        if t not in dev:
            dev[t] = net.read_tensor(t, B).cpu().numpy()
        return dev[t]

    rnd, ulp = _rounding(fmt)
    inner = [tiny.ops[0].dst, tiny.ops[1].dst, tiny.ops[2].dst]
    for t in inner:
        with pytest.raises(rt.Y3Error, match="y3_net_set_tiny_stem_fusion"):
            net.read_tensor(t, B)
    kinds, convs = [], 0
    for i, op in enumerate(tiny.ops):
        if i < 4:
            continue          # the fused launch; what it stores is pool 1's tensor, which the first conv below reads
        if isinstance(op, AuxOp):
            kinds.append(op.kind)
            src = [tensor(t) for t in op.inputs]
            assert all(np.array_equal(rnd(s), s) for s in src), "what is stored is 16-bit"
            ref = {"maxpool_s2": lambda: maxpool2x2_ref(src[0], 2), "maxpool_s1": lambda: maxpool2x2_ref(src[0], 1),
                   "upsample": lambda: O.upsample2x(src[0]), "concat": lambda: O.concat(src[0], src[1])}[op.kind]()
            assert np.array_equal(tensor(op.dst), ref), op
            continue
        assert isinstance(op, ConvOp)
        convs += 1
        ref = _teacher_forced_head(fmt, op, w, tensor)
        got = tensor(op.dst)
        assert got.shape == ref.shape and float(np.abs(ref).max()) > 0.05
        if op.dst in tiny.outputs:
            err, bar = float(np.abs(got - ref).max()), bf16_tile_bar(ref) if fmt == "bf16" else f32_conv_bar(ref)
            assert err <= bar, (fmt, op.conv_index, err, bar)
        else:
            exp = rnd(ref)
            diff = np.abs(got.astype(np.float64) - exp.astype(np.float64))
            assert (diff <= ulp(got, exp) + 1e-5 * float(np.abs(exp).max())).all(), (fmt, op.conv_index)
    assert kinds == ["maxpool_s2"] * 3 + ["maxpool_s1", "upsample", "concat"] and convs == len(tiny.conv_ops()) - 2
    pool1 = tensor(tiny.ops[3].dst)
    assert pool1.shape == (B, hw[0] // 4, hw[1] // 4, 32) and np.array_equal(rnd(pool1), pool1) and float(np.abs(pool1).max()) > 0.1


# ---------------------------------------------------------------------------------------------- 4. invariants
def _composed(rt, net, xd, anchors, M, iou, S):
    grids = net.forward(xd)
    bb, cc, ss = rt.yolo_decode_scores(grids, anchors, NC)
    sel, nv = rt.nms_padded(bb, ss, M, iou, S)
    return rt.pack_detections(bb, cc, ss, sel, nv), nv


@pytest.mark.parametrize("fmt", ["f32", "bf16"])
def test_forward_invariants_with_the_switch_on(rt, tiny, fmt):
    """Two forwards are bit-equal; image 0 alone equals image 0 of a batch of 3; two lanes equal one lane; a graph replay equals the eager
    call; detect is bit-equal to forward + decode + NMS + pack composed by hand."""
    w, x = TC.tiny_inputs(tiny, 3, (96, 96))
    xd = _cuda(x)
    net = _net(rt, tiny, w, 3, 96, fmt)
    assert net.tiny_stem_fused == 1
    net.set_lanes(1)
    a = [g.clone() for g in net.forward(xd)]
    assert all(torch.equal(p, q) for p, q in zip(a, net.forward(xd)))
    one = net.forward(xd[:1].contiguous())
    assert all(torch.equal(p[:1], q) for p, q in zip(a, one))
    net.set_lanes(2)
    assert all(torch.equal(p, q) for p, q in zip(a, net.forward(xd)))
    anchors = TC.tiny_anchors()
    packed, nv = _composed(rt, net, xd, anchors, 100, 0.5, LOW)
    p2, n2 = net.detect(xd, anchors, 100, 0.5, LOW)
    assert torch.equal(n2, nv) and torch.equal(p2, packed) and int(nv.min()) > 0
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


def test_switch_off_is_the_plan_of_a_net_that_never_heard_of_it(rt, tiny):
    w, x = TC.tiny_inputs(tiny, 2, (96, 96))
    xd = _cuda(x)
    never = _net(rt, tiny, w, 2, 96, "f32", fused=None)
    off = _net(rt, tiny, w, 2, 96, "f32", fused=False)
    assert never.tiny_stem_fused == 0 and off.tiny_stem_fused == 0
    assert all(torch.equal(p, q) for p, q in zip(never.forward(xd), off.forward(xd)))
    on = _net(rt, tiny, w, 2, 96, "f32", fused=True)
    assert on.tiny_stem_fused == 1
    for p, q in zip(never.forward(xd), on.forward(xd)):
        assert float((p - q).abs().max()) <= 1e-4


# ---------------------------------------------------------------------------------------------- 5. switch discipline
def test_the_stem_switches_do_not_act_on_each_other(rt, tiny):
    w, _ = TC.tiny_inputs(tiny, 1, (32, 32))
    net = rt.Net(tiny)
    net.load_weights(w)
    assert net.tiny_stem_fused == 0                       # before a plan
    net.set_tiny_stem_fusion(True)
    assert net.tiny_stem_fused == 0                       # the plan takes it up
    net.set_stem_fusion(0)
    net.set_stem_fusion_f16(2)
    for fmt in ("f32", "bf16", "f16"):
        net.plan(1, 96, DT[fmt])
        assert net.tiny_stem_fused == 1, fmt
    net.set_tiny_stem_fusion(False)
    net.set_stem_fusion(1)
    net.set_stem_fusion_f16(1)
    net.plan(1, 96, DT["f32"])
    assert net.tiny_stem_fused == 0
    with pytest.raises(rt.Y3Error, match="argument must be 0 or 1"):
        rt.check(net.lib.y3_net_set_tiny_stem_fusion(net._h, 2), "y3_net_set_tiny_stem_fusion")


def test_on_yolov3_the_switch_is_ignored(rt):
    """The Darknet-53 stem is not tiny's: tiny_stem_fused stays 0 and the grids are those of the plan without the switch, bit for bit, while
    the existing stem fusion of that plan is untouched."""
    from yolo_v3_tf2_amd.graph import load_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    p = load_program(os.path.join(TC.ROOT, "config/models/yolov3/model.yaml"), NC)
    net = rt.Net(p)
    net.load_weights(synthetic_weights(p, seed=5))
    xd = torch.rand((1, 64, 64, 3), device="cuda")
    net.plan(1, 64)
    a = [g.clone() for g in net.forward(xd)]
    net.set_tiny_stem_fusion(True)
    net.plan(1, 64)
    assert net.tiny_stem_fused == 0
    assert all(torch.equal(u, v) for u, v in zip(a, net.forward(xd)))


def test_without_the_switch_16_bit_tiny_is_still_refused(rt, tiny):
    w, _ = TC.tiny_inputs(tiny, 1, (32, 32))
    net = rt.Net(tiny)
    net.load_weights(w)
    net.set_tiny_stem_fusion(False)
    for fmt, name in (("bf16", "bf16"), ("f16", "fp16")):
        with pytest.raises(rt.Y3Error, match=rf"conv 1 \(Cin 32, c0 -1, Cout 32\) has no {name} tile"):
            net.plan(1, 96, DT[fmt])
        assert net.tiny_stem_fused == 0


def test_a_forced_split_inside_the_fused_stem_is_refused_by_name(rt, tiny):
    w, _ = TC.tiny_inputs(tiny, 1, (32, 32))
    net = _net(rt, tiny, w, 1, 96, "bf16")
    with pytest.raises(rt.Y3Error, match=r"conv 1 runs inside the fused tiny stem kernel \(y3_net_set_tiny_stem_fusion\), which is never split"):
        net.set_split_k_bf16(1, 2)
    assert net.split_k_bf16(1) == 1
    net32 = _net(rt, tiny, w, 1, 96, "f32")
    with pytest.raises(rt.Y3Error, match="fused tiny stem"):
        net32.set_split_k(1, 2)


def test_low_latency_bf16_with_the_fused_stem_keeps_the_heads_within_the_bf16_bar(rt, tiny):
    """set_low_latency_bf16 acts on the remaining convs by its own rules; with keep_activations the two head convs, teacher-forced from
    the device's own stored input, stay under bf16_tile_bar."""
    w, x = TC.tiny_inputs(tiny, 1, (96, 96))
    net = _net(rt, tiny, w, 1, 96, "bf16", keep=True, setup=lambda n: n.set_low_latency_bf16(True))
    assert net.tiny_stem_fused == 1
    grids = net.forward(_cuda(x))
    print("tiny bf16 low latency with the fused stem: K slices per conv", [net.split_k_bf16(s) for s in range(len(net.conv_ops))])
    assert net.split_k_bf16(0) == 1 and net.split_k_bf16(1) == 1
    heads = [op for op in tiny.ops if isinstance(op, ConvOp) and op.dst in tiny.outputs]
    assert len(heads) == 2
    for op in heads:
        g = grids[tiny.outputs.index(op.dst)]
        got = g.reshape(1, g.shape[1], g.shape[2], -1).cpu().numpy()
        ref = _teacher_forced_head("bf16", op, w, lambda t: net.read_tensor(t, 1).cpu().numpy())
        err, bar = float(np.abs(got - ref).max()), bf16_tile_bar(ref)
        assert err <= bar, (op.conv_index, err, bar)


# ---------------------------------------------------------------------------------------------- 6. streams and drivers
def test_detect_stream_with_letterbox_in_bf16_equals_detect_composed_by_hand(rt, tiny):
    from tests.test_evaluate_gpu import _detect
    from tests.test_tiny_gpu import STREAM_S, _frames
    anchors = TC.tiny_anchors()
    w, _ = TC.tiny_inputs(tiny, 1, (32, 32))
    net = _net(rt, tiny, w, 3, STREAM_S, "bf16")
    assert net.tiny_stem_fused == 1
    batches = _frames()
    dets = [_detect(rt, net, b, anchors, STREAM_S, LOW, True) for b in batches]
    got = list(net.detect_stream(batches, anchors, 100, 0.5, LOW, letterbox=True))
    assert len(got) == 2 and net.tiny_stem_fused == 1
    for (gp, gn), (wp, wn) in zip(got, dets):
        assert np.array_equal(gn, wn) and np.array_equal(gp, wp) and int(wn.min()) > 0


def test_evaluate_driver_on_device_in_bf16_with_the_yaml_key(rt, tiny, tmp_path):
    """evaluate_yolov3.evaluate(on_device=True) on the tiny model config with dtype: bf16 and tiny_fused_stem: true: its counters are those
    of sweep_counters over Net.detect composed by hand on the same frames; without the key the same config is refused by the plan."""
    from tests.helpers import jpeg_bytes
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev
    from yolo_v3_tf2_amd.core import load_tfrecords as m
    from yolo_v3_tf2_amd.evaluate_detections import sweep_counters
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
    S = 96
    cfg = dict(tfrecords_dir=str(d), image_size=S, batch_size=2, yolo_max_boxes=100, nms_iou_threshold=0.5,
               classes_name_file=os.path.join(TC.ROOT, "datasets/coco2012/coco.names"), anchors_file=TC.TINY_ANCHORS,
               model_config_file=TC.TINY_MODEL, dtype="bf16", tiny_fused_stem=True)
    w, _ = TC.tiny_inputs(tiny, 1, (32, 32))
    thresholds = [0.006, LOW]
    dev = ev.evaluate(cfg, thresholds, evaluate_iou_threshold=0.1, weights=w, on_device=True)
    anchors = TC.tiny_anchors()
    net = _net(rt, tiny, w, 2, S, "bf16")
    data = list(ev.parse_tfrecords(cfg["tfrecords_dir"], image_size=S, max_bboxes=100, class_file=cfg["classes_name_file"]))
    assert len(data) == 4
    total = 0
    for k in (0, 2):
        images = np.stack([np.asarray(data[k + j][0], np.float32) for j in range(2)])
        gt = []
        for j in range(2):
            y = np.asarray(data[k + j][1])
            y = y[y[..., 4] == 1]
            gt.append((y[:, 0:4], y[:, 5].astype(np.int32)))
        packed, nv = net.detect(_cuda(images), anchors, 100, 0.5, min(thresholds))
        gb, gc, cnt = rt.pack_ground_truth(gt, 100)
        total = total + sweep_counters(packed.cpu().numpy(), nv.cpu().numpy(), gb, gc, cnt, NC, 0.1, thresholds)
    for t in range(len(thresholds)):
        want, got = ev.counters_from_row(total[t], NC), dev[t][3]
        assert sorted(want) == sorted(got) and all(np.array_equal(want[k], got[k]) for k in want), t
    assert dev[0][3]["examples"] == 4 and dev[0][3]["preds"].sum() > 0
    with pytest.raises(rt.Y3Error, match="has no bf16 tile"):
        ev.evaluate(dict(cfg, tiny_fused_stem=None), thresholds, evaluate_iou_threshold=0.1, weights=w, on_device=True)
