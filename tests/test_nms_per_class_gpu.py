"""Per-class NMS on the device: nms_kernel<PER_CLASS> (y3_nms_padded_per_class) against the NumPy restatement
nms_per_class.nms_padded_per_class_ref, which tests/test_nms_per_class_host.py ties to a brute-force loop and to the C oracle;
with all ids equal against y3_nms_padded itself; Net.nms_per_class through detect, a captured graph, detect_stream and
evaluate_stream.  Every op call writes into output and workspace buffers filled with 0xFF.  Every comparison is exact."""
import ctypes as C_

import numpy as np
import pytest

from tests import nms_edge_cases as C
from tests import nms_per_class_cases as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from yolo_v3_tf2_amd.nms_per_class import nms_padded_per_class_ref  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _per_class(boxes, scores, classes, M, T, S):
    """ops.nms_padded_per_class into buffers of its own, all filled with 0xFF: the outputs and a workspace of exactly
    y3_nms_per_class_workspace_bytes with 256 guard bytes behind it, which must come back untouched."""
    from yolo_v3_tf2_amd import ops
    B, N = scores.shape
    need = ops._nms_workspace_bytes(B, N, per_class=True)
    buf = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    sel = torch.full((B, M), -1, dtype=torch.int32, device="cuda")
    nv = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    ops._nms(_cuda(boxes), _cuda(scores), M, T, S, out=(sel, nv), ws=buf[:need], classes=_cuda(classes))
    torch.cuda.synchronize()
    assert (buf[need:] == 0xFF).all(), "written behind the workspace"
    sel, nv = sel.cpu().numpy(), nv.cpu().numpy()
    assert all(not sel[i, n:].any() for i, n in enumerate(nv))      # rows past num_valid are zero
    return sel, nv


def _same(got, want):
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert np.array_equal(got[0], want[0]), int((got[0] != want[0]).sum())


def _agnostic(rt, boxes, scores, M, T, S):
    sel, nv = rt.nms_padded(_cuda(boxes), _cuda(scores), M, T, S)
    torch.cuda.synchronize()
    return sel.cpu().numpy(), nv.cpu().numpy()


def _all_ids_equal(rt, case):
    boxes, scores, M, T, S = case
    want = _agnostic(rt, boxes, scores, M, T, S)
    for cid in (0, 2**31 - 1):
        _same(_per_class(boxes, scores, np.full(scores.shape, cid, np.int64), M, T, S), want)
    return want[1]


# ------------------------------------------------------------------------------------------------ all ids equal: y3_nms_padded
@pytest.mark.parametrize("name", C.CANONICAL + C.SCORES)
def test_all_ids_equal_on_the_canonical_and_score_cases(rt, name):
    nv = _all_ids_equal(rt, C.canonical_case(name) if name in C.CANONICAL else C.score_case(name))
    assert nv.min() > 10


@pytest.mark.parametrize("nc", C.CANDIDATE_COUNTS)
def test_all_ids_equal_on_the_candidate_counts(rt, nc):
    assert (_all_ids_equal(rt, C.count_case(nc)) >= 1).all()


@pytest.mark.parametrize("M", C.M_VALUES)
def test_all_ids_equal_where_M_is_reached(rt, M):
    for k in (M - 1, M, M + 1):
        assert (_all_ids_equal(rt, C.lattice_case(M, k)) == min(k, M)).all()


# ------------------------------------------------------------------------------------------------ any ids: the restatement
@pytest.mark.parametrize("ncls", P.RANDOM_CLASSES)
@pytest.mark.parametrize("nc", P.RANDOM_COUNTS)
def test_random_ids_equal_the_restatement(rt, nc, ncls):
    for M in (100, 1024):
        case = P.random_case(nc, ncls, M)
        want = nms_padded_per_class_ref(*case)
        _same(_per_class(*case), want)
        agnostic = _agnostic(rt, *case[:2], *case[3:])
        assert nc < 255 or not np.array_equal(agnostic[0], want[0]), "the class ids change the selection on these inputs"


def test_ids_up_to_int32_max(rt):
    boxes, scores, _, M, T, S = P.random_case(513, 2, 1024)
    classes = P.BIG_IDS[P.random_ids(3, scores.shape, len(P.BIG_IDS))]
    assert classes.max() == 2**31 - 1
    _same(_per_class(boxes, scores, classes, M, T, S), nms_padded_per_class_ref(boxes, scores, classes, M, T, S))


@pytest.mark.parametrize("M", [100, 1024])
def test_all_ids_distinct_nothing_is_suppressed(rt, M):
    case = P.distinct_ids_case(M)
    boxes, scores = case[:2]
    got = _per_class(*case)
    _same(got, nms_padded_per_class_ref(*case))
    for b in range(2):      # the candidates in sorted order, cut at M: every stress-set box has a positive coordinate
        cand = np.flatnonzero(scores[b] > case[5])
        order = cand[np.argsort(-scores[b, cand], kind="stable")]
        assert (boxes[b, order] > 0).any(axis=1).all()
        assert got[1][b] == min(M, 513) and got[0][b, :got[1][b]].tolist() == order[:M].tolist()


def test_exact_duplicates_in_the_same_and_in_an_earlier_chunk(rt):
    case, missing = P.duplicates_case()
    sel, nv = _per_class(*case)
    want = [i for i in range(600) if i not in missing]
    assert nv.tolist() == [598, 598] and sel[0, :598].tolist() == want and sel[1, :598].tolist() == want
    _same((sel, nv), nms_padded_per_class_ref(*case))
    assert _agnostic(rt, *case[:2], *case[3:])[1].tolist() == [596, 596], "the agnostic rule drops all four duplicates"


def test_spilled_suppressors_and_their_class_ids_are_read_back(rt):
    """More than KEPT_CAP kept boxes: tests/nms_per_class_cases.spill_case says which probe rests on which spilled box, each at least one
    chunk behind it, so that the pair is met in the kept-list pass and the box and its class id come from the workspace;
    tests/test_nms_per_class_host.py shows that the case tells a broken class test on that branch from a right one."""
    case, at, _, selected = P.spill_case()
    sel, nv = _per_class(*case)
    _same((sel, nv), nms_padded_per_class_ref(*case))
    for b in range(2):
        got = sel[b, :nv[b]].tolist()
        assert got == selected
        assert {at["P2"], at["P5"]} <= set(got) and not {at["P1"], at["P3"], at["P4"]} & set(got)


def test_graph_replay_equals_eager(rt):
    from yolo_v3_tf2_amd import ops
    first, second = P.random_case(4097, 7, 100), P.random_case(513, 7, 100)
    bufs = [_cuda(a) for a in first[:3]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.nms_padded_per_class(*bufs, 100, P.T, P.S)        # warm-up: the workspace is made here
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sel, nv = ops.nms_padded_per_class(*bufs, 100, P.T, P.S)
    for case in (first, second, first):
        for buf, a in zip(bufs, case[:3]):
            buf.copy_(_cuda(a))
        sel.fill_(-1)
        nv.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        got = sel.cpu().numpy(), nv.cpu().numpy()
        _same(got, _per_class(*case))
        _same(got, nms_padded_per_class_ref(*case))


def test_argument_checks(rt):
    """Those of y3_nms_padded, a null class pointer, T <= 0, and the larger workspace; nothing is enqueued by a refused call."""
    from yolo_v3_tf2_amd import _lib, ops
    lib = _lib.load()
    boxes, scores, classes, M, T, S = P.random_case(127, 2, 100)
    B, N = scores.shape
    b, s, c = _cuda(boxes), _cuda(scores), _cuda(classes)
    sel = torch.full((B, M), -1, dtype=torch.int32, device="cuda")
    nv = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    need = lib.y3_nms_per_class_workspace_bytes(B, N)
    assert need == lib.y3_nms_workspace_bytes(B, N) + B * N * 4
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    p = lambda t: C_.c_void_p(t.data_ptr())
    good = dict(b=p(b), s=p(s), c=p(c), B=B, N=N, M=M, T=T, S=S, sel=p(sel), nv=p(nv), ws=p(ws), bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        return lib.y3_nms_padded_per_class(a["b"], a["s"], a["c"], a["B"], a["N"], a["M"], a["T"], a["S"], a["sel"], a["nv"], a["ws"],
                                           a["bytes"], _lib.stream_ptr())

    bad = [(dict([(k, None)]), b"bad argument") for k in ("b", "s", "c", "sel", "nv")]
    bad += [(dict(B=0), b"bad argument"), (dict(N=0), b"bad argument"), (dict(M=0), b"max_output_size"), (dict(M=1025), b"max_output_size"),
            (dict(b=C_.c_void_p(b.data_ptr() + 4)), b"aligned"), (dict(T=0.0), b"iou_threshold must be > 0"),
            (dict(T=-0.5), b"iou_threshold must be > 0"), (dict(T=float("nan")), b"iou_threshold must be > 0"),
            (dict(ws=None), b"workspace too small"), (dict(bytes=lib.y3_nms_workspace_bytes(B, N)), b"workspace too small")]
    for kw, word in bad:
        assert call(**kw) == _lib.Y3_ERR_INVALID, kw
        msg = lib.y3_last_error()
        assert b"y3_nms_padded_per_class" in msg and word in msg, (kw, msg)
    torch.cuda.synchronize()
    assert (sel == -1).all() and (nv == -1).all() and (ws == 0xFF).all()
    assert call() == 0
    torch.cuda.synchronize()
    _same((sel.cpu().numpy(), nv.cpu().numpy()), nms_padded_per_class_ref(boxes, scores, classes, M, T, S))
    # the Python wrapper: T <= 0 comes back as Y3Error, and it refuses the class tensors it can see are wrong
    with pytest.raises(rt.Y3Error, match="iou_threshold must be > 0"):
        ops.nms_padded_per_class(b, s, c, M, 0.0, S)
    for wrong in (c.int(), c[:, :-1], c.cpu(), c.t().contiguous().t()):
        with pytest.raises(rt.Y3Error):
            ops.nms_padded_per_class(b, s, wrong, M, T, S)


# ------------------------------------------------------------------------------------------------ the net
NET_S, NET_M, NET_SCORE = 96, 600, 0.005      # see test_net_detect_follows_the_property: where the two rules differ on this input


def _net_input():
    return np.random.default_rng(1234).random((2, NET_S, NET_S, 3), dtype=np.float32)


def _net(rt, program, weights, dtype="f32", batch=2, size=NET_S):
    from yolo_v3_tf2_amd import _lib
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(batch, size, {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16}[dtype])
    return net


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_net_detect_follows_the_property(rt, program, weights, anchors, dtype):
    """2 x 96^2, the synthetic weights, 80 classes.  At S = 0.005, M = 600 the oracle's decode of this input has 472 candidates per
    image in 48 classes; the agnostic rule keeps 461 / 459 of them and the per-class rule 470 / 470 (asserted below on the CPU), so
    the comparison cannot pass with the class ids ignored."""
    from oracle import oracle as O
    from yolo_v3_tf2_amd import ops
    x = _net_input()
    bb, cls, sc, asel, anv = O.yolo_nms(O.yolo_decode(O.forward(program, weights, x), anchors, 80), NET_M, 0.5, NET_SCORE)
    psel, pnv = nms_padded_per_class_ref(bb, sc, cls, NET_M, 0.5, NET_SCORE)
    assert (pnv > anv).all() and not np.array_equal(psel, asel), "the two rules select differently on this input"
    net, xd = _net(rt, program, weights, dtype), _cuda(x)
    assert net.nms_per_class is False
    agnostic = [t.clone() for t in net.detect(xd, anchors, NET_M, 0.5, NET_SCORE)]
    dec = net.forward_decode(xd, anchors)
    composed_agnostic = rt.pack_detections(*dec, *rt.nms_padded(dec[0], dec[2], NET_M, 0.5, NET_SCORE))
    assert torch.equal(agnostic[0], composed_agnostic)
    net.nms_per_class = True
    assert net.nms_per_class is True and net.lib.y3_net_get_nms_mode(net._h) == 1
    packed, nv = net.detect(xd, anchors, NET_M, 0.5, NET_SCORE)
    sel, nv2 = ops.nms_padded_per_class(dec[0], dec[2], dec[1], NET_M, 0.5, NET_SCORE)
    assert torch.equal(nv, nv2) and torch.equal(packed, rt.pack_detections(*dec, sel, nv2))
    assert not torch.equal(packed, agnostic[0]) and (nv > agnostic[1]).all()
    # ... and the device's selection is the restatement's on the device's own decode
    _same((sel.cpu().numpy(), nv2.cpu().numpy()),
          nms_padded_per_class_ref(dec[0].cpu().numpy(), dec[2].cpu().numpy(), dec[1].cpu().numpy(), NET_M, 0.5, NET_SCORE))
    with pytest.raises(rt.Y3Error, match="iou_threshold must be > 0"):
        net.detect(xd, anchors, NET_M, 0.0, NET_SCORE)
    # a graph captured with the property on keeps that rule after the property is switched off
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net.detect(xd, anchors, NET_M, 0.5, NET_SCORE)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gp, gn = net.detect(xd, anchors, NET_M, 0.5, NET_SCORE)
    net.nms_per_class = False
    assert net.nms_per_class is False
    gp.zero_()
    gn.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gp, packed) and torch.equal(gn, nv)
    # off again: the same net reproduces the agnostic bits
    again = net.detect(xd, anchors, NET_M, 0.5, NET_SCORE)
    assert torch.equal(again[0], agnostic[0]) and torch.equal(again[1], agnostic[1])
    for bad in (1, "on", None):
        with pytest.raises(TypeError):
            net.nms_per_class = bad


def test_detect_model_follows_the_model_switch(rt, program, weights, anchors):
    """core.parse_model.YoloModel.set_nms_per_class: both routes of inference.DetectModel give the per-class 5-tuple."""
    from yolo_v3_tf2_amd import ops
    from yolo_v3_tf2_amd.core.parse_model import YoloModel
    from yolo_v3_tf2_amd.inference import DetectModel
    x = _net_input()
    model = YoloModel(program)
    model.set_weights_dict(weights)
    outs = {}
    for fused in (False, True):
        det = DetectModel(model, anchors, 80, NET_M, 0.5, NET_SCORE, fused=fused)
        for on in (False, True, False):
            model.set_nms_per_class(on)
            assert model._device_net().nms_per_class is on
            outs[fused, on] = det.predict(x)
    for on in (False, True):
        for a, b in zip(outs[False, on], outs[True, on]):
            assert np.array_equal(a, b)
    bb, cls, sc, sel, nv = outs[True, True]
    want = ops.nms_padded_per_class(_cuda(bb), _cuda(sc), _cuda(cls), NET_M, 0.5, NET_SCORE)
    assert np.array_equal(sel, want[0].cpu().numpy()) and np.array_equal(nv, want[1].cpu().numpy())
    assert (nv > outs[True, False][4]).all()


def _host_rows(dec, M, T, S):
    """The restatement's detections of a device decode as packed rows -> (packed [B,M,7] int32, num_valid)."""
    bb, cls, sc = (t.cpu().numpy() for t in dec)
    sel, nv = nms_padded_per_class_ref(bb, sc, cls, M, T, S)
    packed = np.zeros((len(nv), M, 7), np.int32)
    for b, n in enumerate(nv):
        rows = sel[b, :n]
        packed[b, :n, :4] = bb[b, rows].view(np.int32)
        packed[b, :n, 4] = sc[b, rows].view(np.int32)
        packed[b, :n, 5] = cls[b, rows].astype(np.int32)
        packed[b, :n, 6] = rows
    return packed, nv


def test_streams_follow_the_property(rt, program, weights, anchors):
    """detect_stream and evaluate_stream(loss=True, ap=True) with the property on, batches of 4, 4 and 3 frames at S = 160: the rows
    are those of Net.detect per batch and of the restatement on the device's decode; the counters and the AP are the host classes'
    on the restatement's rows; the loss does not depend on the rule.  loss=True takes the composed route, which picks the op itself."""
    from tests.test_evaluate_gpu import STREAM_S, _ground_truth_from, _staged, _stream_batches
    from yolo_v3_tf2_amd.evaluate_detections import average_precision, match_detections, sweep_counters
    S, batches, M, low = STREAM_S, _stream_batches(), NET_M, NET_SCORE
    thresholds = [low, 0.05, 0.1]
    net = _net(rt, program, weights, batch=4, size=S)
    rows_off = [tuple(np.array(a) for a in r) for r in net.detect_stream(batches, anchors, M, 0.5, low)]
    loss_off = net.evaluate_stream(batches, [[(np.array([[.2, .2, .6, .6]], np.float32), np.array([3], np.int32))] * len(b) for b in batches],
                                   anchors, M, 0.5, thresholds, 80, loss=True)[1]
    net.nms_per_class = True
    want_rows = []
    for frames in batches:
        staged = _staged(rt, frames, S, False)
        packed, nv = net.detect(staged, anchors, M, 0.5, low)
        host = _host_rows(net.forward_decode(staged, anchors), M, 0.5, low)
        assert np.array_equal(packed.cpu().numpy(), host[0]) and np.array_equal(nv.cpu().numpy(), host[1])
        want_rows.append(host)
    rows_on = [tuple(np.array(a) for a in r) for r in net.detect_stream(batches, anchors, M, 0.5, low)]
    assert len(rows_on) == 3
    for got, want in zip(rows_on, want_rows):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert all(not np.array_equal(on[0], off[0]) for on, off in zip(rows_on, rows_off)), "the two rules give other rows in every batch here"
    rng = np.random.default_rng(5)
    gts = [_ground_truth_from(*rows, rng, first=4 * i) for i, rows in enumerate(want_rows)]
    G = max(len(c) for g in gts for _, c in g)
    counters, records, totals = 0, [], 0
    for (packed, nv), gt in zip(want_rows, gts):
        gt_packed = rt.pack_ground_truth(gt, G)
        counters = counters + sweep_counters(packed, nv, *gt_packed, 80, 0.5, thresholds)
        r, t = match_detections(packed, nv, *gt_packed, 80, [0.5, 0.75])
        records.append(r)
        totals = totals + t
    want_ap = average_precision(np.concatenate(records), totals, 80, 2)
    for loss in (False, True):      # the fused route, then the composed one
        out = net.evaluate_stream(batches, gts, anchors, M, 0.5, thresholds, 80, loss=loss, ap=[0.5, 0.75])
        got_counters, got_ap = out[0], out[-1]
        assert np.array_equal(got_counters, counters), loss
        assert np.array_equal(got_ap["ap"], want_ap["ap"], equal_nan=True) and got_ap["mAP"] == want_ap["mAP"], loss
        assert (got_ap["images"], got_ap["errors"]) == (11, 0) and 0.0 < got_ap["mAP"] <= 1.0
    loss_on = net.evaluate_stream(batches, [[(np.array([[.2, .2, .6, .6]], np.float32), np.array([3], np.int32))] * len(b) for b in batches],
                                  anchors, M, 0.5, thresholds, 80, loss=True)[1]
    assert np.array_equal(loss_on["sum"], loss_off["sum"]) and loss_on["images"] == loss_off["images"] == 11
