"""Multi-label candidates on the device: y3_yolo_decode_candidates_hw (csrc/candidates.hip) against the NumPy restatement
multilabel.candidates_ref over the arrays y3_yolo_decode_hw gives for the same grids, which tests/test_multilabel_host.py ties to a
brute-force loop and to the single-label path; Net.multi_label through detect, a captured graph, detect_stream, evaluate_stream and
tiles.  Every op call writes into output and workspace buffers filled with 0xFF with 256 guard bytes behind each.  Every comparison
is exact: there is no tolerance anywhere."""
import ctypes as C_
import warnings

import numpy as np
import pytest

from tests import multilabel_cases as MC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from yolo_v3_tf2_amd.multilabel import candidates_ref, detect_multi_label_ref  # noqa: E402

GUARD = 256


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(shape, dtype):
    """A tensor of `shape` filled with 0xFF bytes with GUARD bytes of 0xFF behind it -> (view, whole byte buffer, payload bytes)."""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    return buf[:nbytes].view(dtype).view(shape), buf, nbytes


def _candidates(grids, anchors, nc, S, K):
    """ops.decode_candidates into poisoned, guarded buffers of its own -> the five arrays as NumPy."""
    from yolo_v3_tf2_amd import ops
    B = grids[0].shape[0]
    hw = [(g.shape[1], g.shape[2]) for g in grids]
    outs = [_guarded(s, d) for s, d in (((B, K, 4), torch.float32), ((B, K), torch.int64), ((B, K), torch.float32),
                                        ((B, K), torch.int32), ((B,), torch.int32))]
    need = ops.decode_candidates_workspace_bytes(hw, B, nc)
    assert need == B * MC.boxes_per_image(hw) * 4
    ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    ops.decode_candidates([_cuda(g) for g in grids], anchors, nc, S, K, out=tuple(o[0] for o in outs), ws=ws[:need])
    torch.cuda.synchronize()
    assert (ws[need:] == 0xFF).all(), "written behind the workspace"
    for view, buf, nbytes in outs:
        assert (buf[nbytes:] == 0xFF).all(), "written behind an output"
    return tuple(o[0].cpu().numpy() for o in outs)


def _decoded(rt, grids, anchors, nc):
    return tuple(t.cpu().numpy() for t in rt.yolo_decode([_cuda(g) for g in grids], anchors, nc))


def _same(got, want, what=""):
    for name, g, w in zip(("boxes", "cls", "scores", "src", "totals"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        gv, wv = (g.view(np.int32), w.view(np.int32)) if g.dtype == np.float32 else (g, w)
        assert np.array_equal(gv, wv), (what, name, int((gv != wv).sum()))


# ------------------------------------------------------------------------------------------------ 1. random logits
@pytest.mark.parametrize("B", MC.BATCHES)
@pytest.mark.parametrize("nc", MC.CLASS_COUNTS)
@pytest.mark.parametrize("shape", sorted(MC.GRIDS))
def test_random_logits_equal_the_restatement(rt, anchors, shape, nc, B):
    hw = MC.GRIDS[shape]
    grids = MC.random_grids(hw, nc, B)
    dec = _decoded(rt, grids, anchors, nc)
    pairs = MC.boxes_per_image(hw) * nc
    full = candidates_ref(*dec, MC.S_RANDOM, pairs)
    assert (full[4] > 0).all() and (full[4] < pairs).all(), "some but not all pairs of every image are candidates"
    for K in (pairs, int(full[4].min()) - 1 if full[4].min() > 1 else 1):      # every candidate stored; every image truncated
        _same(_candidates(grids, anchors, nc, MC.S_RANDOM, K), candidates_ref(*dec, MC.S_RANDOM, K), (shape, nc, B, K))


# ------------------------------------------------------------------------------------------------ 2. planted counts
@pytest.mark.parametrize("nc", [1, 3, 80])
@pytest.mark.parametrize("shape", sorted(MC.GRIDS))
def test_planted_pairs_on_every_boundary(rt, anchors, shape, nc):
    """Exactly the planted pairs are candidates: the first and last pair of every image, both sides of every scale boundary and of
    every 64-box workgroup boundary, at B = 7."""
    hw, B = MC.GRIDS[shape], 7
    pairs = MC.boundary_pairs(hw, nc, B)
    grids = MC.planted_grids(hw, nc, B, pairs)
    K = max(sum(1 for p in pairs if p[0] == b) for b in range(B))
    got = _candidates(grids, anchors, nc, MC.S_RANDOM, K)
    _same(got, candidates_ref(*_decoded(rt, grids, anchors, nc), MC.S_RANDOM, K), (shape, nc))
    for b in range(B):
        mine = [(n, c) for bb, n, c in pairs if bb == b]
        assert got[4][b] == len(mine) >= 2
        assert list(zip(got[3][b, :len(mine)].tolist(), got[1][b, :len(mine)].tolist())) == mine


@pytest.mark.parametrize("shape", sorted(MC.GRIDS))
def test_planted_counts_around_the_capacity(rt, anchors, shape):
    """0, 1, K - 1, K, K + 1 candidates per image, and an overflowing image between two that do not overflow; then all pairs (S = -1)."""
    hw, nc, K = MC.GRIDS[shape], 5, 37
    counts = [0, 1, K - 1, K + 1, K, K + 40, 3]
    pairs = [p for b, k in enumerate(counts) for p in MC.first_pairs(hw, nc, b, k)]
    grids = MC.planted_grids(hw, nc, len(counts), pairs)
    dec = _decoded(rt, grids, anchors, nc)
    got = _candidates(grids, anchors, nc, MC.S_RANDOM, K)
    assert got[4].tolist() == counts
    _same(got, candidates_ref(*dec, MC.S_RANDOM, K), shape)
    for b, k in enumerate(counts):      # the filler behind min(total, K)
        assert not got[0][b, min(k, K):].any() and not got[1][b, min(k, K):].any() and not got[2][b, min(k, K):].any() and \
            not got[3][b, min(k, K):].any()
    every = MC.boxes_per_image(hw) * nc
    for cap in (every, every - 1, 1):
        got = _candidates(grids, anchors, nc, -1.0, cap)
        assert (got[4] == every).all()
        _same(got, candidates_ref(*dec, -1.0, cap), (shape, "all", cap))


# ------------------------------------------------------------------------------------------------ 3. the threshold on a score's own bits
def test_threshold_on_a_scores_own_bits(rt, anchors):
    hw, nc, B = MC.RECT, 5, 3
    grids = MC.random_grids(hw, nc, B)
    pairs = MC.boxes_per_image(hw) * nc
    base = _candidates(grids, anchors, nc, MC.S_RANDOM, pairs)
    k = int(base[4][1]) // 2
    s, n, c = base[2][1, k], int(base[3][1, k]), int(base[1][1, k])
    assert s > np.float32(MC.S_RANDOM)

    def has(S):
        got = _candidates(grids, anchors, nc, float(S), pairs)
        t = int(got[4][1])
        return ((got[3][1, :t] == n) & (got[1][1, :t] == c)).any()
    assert not has(s), "score > S is strict"
    assert has(np.nextafter(s, np.float32(-np.inf)))


# ------------------------------------------------------------------------------------------------ 4. non-finite logits
def test_non_finite_logits(rt, anchors):
    hw, nc, B = MC.SQUARE, 5, 3
    grids = MC.random_grids(hw, nc, B, seed=4)
    rng = np.random.default_rng(9)
    for g in grids:
        flat = g.reshape(-1, 5 + nc)
        for value in (np.nan, np.inf, -np.inf):
            rows = rng.choice(len(flat), max(2, len(flat) // 10), replace=False)
            flat[rows[::2], 4] = value                                  # objectness
            flat[rows[1::2], 5 + rng.integers(0, nc, len(rows[1::2]))] = value      # a class channel
    dec = _decoded(rt, grids, anchors, nc)
    pairs = MC.boxes_per_image(hw) * nc
    assert np.isnan(dec[1]).any() and np.isnan(dec[2]).any()
    for S in (MC.S_RANDOM, -1.0):
        got = _candidates(grids, anchors, nc, S, pairs)
        _same(got, candidates_ref(*dec, S, pairs), S)
        assert not np.isnan(got[2]).any(), "a NaN score is no candidate"
    with np.errstate(all="ignore"):
        assert (got[4] == (~np.isnan(dec[1] * dec[2])).sum(axis=(1, 2))).all(), "S < 0: every pair with a non-NaN score"


# ------------------------------------------------------------------------------------------------ 5. the two consequences
@pytest.mark.parametrize("nc", [1, 5, 80])
def test_consequences_against_decode_scores(rt, anchors, nc):
    """K = N * nc.  Box n has a candidate iff its y3_yolo_decode_scores score is > S; its largest candidate score is that score bit for
    bit; the class of that candidate is the arg-max class unless two products tie -- then it is the lowest class among the tied, which
    may differ: such boxes are counted apart.  And the candidates at S' > S are those at S with score > S', in the same order."""
    hw, B = MC.RECT, 3
    grids = MC.random_grids(hw, nc, B, seed=2)
    N = MC.boxes_per_image(hw)
    bb, cls, sc = (t.cpu().numpy() for t in rt.yolo_decode_scores([_cuda(g) for g in grids], anchors, nc))
    got = _candidates(grids, anchors, nc, MC.S_RANDOM, N * nc)
    ties = 0
    for b in range(B):
        t = int(got[4][b])
        src, ccls, csc = got[3][b, :t], got[1][b, :t], got[2][b, :t]
        assert np.array_equal(np.unique(src), np.flatnonzero(sc[b] > np.float32(MC.S_RANDOM)))
        for n in np.unique(src):
            mine = src == n
            best = csc[mine].max()
            assert best.view(np.int32) == sc[b, n].view(np.int32)
            assert np.array_equal(got[0][b, :t][mine].view(np.int32), np.tile(bb[b, n].view(np.int32), (mine.sum(), 1)))
            first = ccls[mine][np.argmax(csc[mine])]
            if first != cls[b, n]:
                ties += 1
                assert first < cls[b, n] and (csc[mine] == best).sum() >= 2
    print(f"nc={nc}: boxes whose largest product ties across classes with another arg-max: {ties}")
    for S2 in (0.2, 0.5, 0.9):
        hi = _candidates(grids, anchors, nc, S2, N * nc)
        for b in range(B):
            keep = got[2][b, :got[4][b]] > np.float32(S2)
            assert hi[4][b] == keep.sum()
            for i in range(4):
                assert np.array_equal(hi[i][b, :hi[4][b]], got[i][b, :got[4][b]][keep])


# ------------------------------------------------------------------------------------------------ 7. argument checks
def test_argument_checks(rt, anchors):
    """Every refusal of y3_yolo_decode_candidates_hw enqueues nothing: the poisoned outputs and workspace stay untouched."""
    from yolo_v3_tf2_amd import _lib
    lib = _lib.load()
    hw, nc, B, K = MC.RECT, 5, 3, 50
    N = MC.boxes_per_image(hw)
    grids = [_cuda(g) for g in MC.random_grids(hw, nc, B)]
    outs = [_guarded(s, d)[0] for s, d in (((B, K, 4), torch.float32), ((B, K), torch.int64), ((B, K), torch.float32),
                                           ((B, K), torch.int32), ((B,), torch.int32))]
    gs = (C_.c_int32 * 6)(*[v for p in hw for v in p])
    need = lib.y3_decode_candidates_workspace_bytes(gs, B, nc)
    assert need == B * N * 4
    assert lib.y3_decode_candidates_workspace_bytes(None, B, nc) == 0 and lib.y3_decode_candidates_workspace_bytes(gs, 0, nc) == 0
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    p = lambda t: C_.c_void_p(t.data_ptr())
    a = np.ascontiguousarray(anchors, np.float32)
    good = dict(grids=(C_.c_void_p * 3)(*[g.data_ptr() for g in grids]), gs=gs, B=B, nc=nc, a=a.ctypes.data_as(C_.POINTER(C_.c_float)), S=0.1,
                K=K, boxes=p(outs[0]), cls=p(outs[1]), scores=p(outs[2]), src=p(outs[3]), totals=p(outs[4]), ws=p(ws), bytes=need)

    def call(**kw):
        v = dict(good, **kw)
        return lib.y3_yolo_decode_candidates_hw(v["grids"], v["gs"], v["B"], v["nc"], v["a"], v["S"], v["K"], v["boxes"], v["cls"], v["scores"],
                                                v["src"], v["totals"], v["ws"], v["bytes"], _lib.stream_ptr())

    big = (C_.c_int32 * 6)(2, 3, 4, 6, 20000, 20000)      # N * nclasses and batch * N beyond 2^31
    bad = [(dict([(k, None)]), b"null pointer") for k in ("grids", "gs", "a", "boxes", "cls", "scores", "src", "totals")]
    bad += [(dict(B=0), b"at least 1"), (dict(K=0), b"at least 1"), (dict(nc=0), b"at least 1"), (dict(K=-3), b"at least 1"),
            (dict(boxes=C_.c_void_p(outs[0].data_ptr() + 4)), b"16-byte aligned"),
            (dict(grids=(C_.c_void_p * 3)(grids[0].data_ptr() + 4, grids[1].data_ptr(), grids[2].data_ptr())), b"16-byte aligned"),
            (dict(K=2**31 - 1), b"below 2^31"), (dict(gs=big), b"below 2^31"),
            (dict(gs=(C_.c_int32 * 6)(2, 3, 0, 6, 8, 12)), b"grid sides"),
            (dict(ws=None), b"workspace too small"), (dict(bytes=need - 1), b"workspace too small"),
            (dict(nc=641), b"LDS")]
    for kw, word in bad:
        assert call(**kw) == _lib.Y3_ERR_INVALID, kw
        msg = lib.y3_last_error()
        assert b"y3_yolo_decode_candidates_hw" in msg and word in msg, (kw, msg)
    torch.cuda.synchronize()
    assert all((o.view(torch.uint8) == 0xFF).all() for o in outs) and (ws == 0xFF).all()
    assert call() == 0
    torch.cuda.synchronize()
    dec = _decoded(rt, [g.cpu().numpy() for g in grids], anchors, nc)
    _same(tuple(o.cpu().numpy() for o in outs), candidates_ref(*dec, 0.1, K))


def test_class_candidates_equal_decode_candidates(rt, anchors):
    """The stand-alone form over decoded tensors (y3_class_candidates; core.yolo_nms.yolo_nms_multi_label, YoloNmsLayer(multi_label=True))."""
    from yolo_v3_tf2_amd import ops
    from yolo_v3_tf2_amd.core.yolo_nms import yolo_nms_multi_label
    from yolo_v3_tf2_amd.core.yolo_nms_layer import YoloNmsLayer
    for nc, B in ((1, 7), (5, 3), (81, 1)):
        grids = MC.random_grids(MC.RECT, nc, B)
        dec = rt.yolo_decode([_cuda(g) for g in grids], anchors, nc)
        pairs = MC.boxes_per_image(MC.RECT) * nc
        for K in (pairs, 11):
            got = tuple(t.cpu().numpy() for t in ops.class_candidates(*dec, MC.S_RANDOM, K))
            _same(got, _candidates(grids, anchors, nc, MC.S_RANDOM, K), (nc, B, K))
    N = MC.boxes_per_image(MC.RECT)
    out = yolo_nms_multi_label(dec, 100, 0.5, MC.S_RANDOM, 0)
    cand = ops.class_candidates(*dec, MC.S_RANDOM, N)
    sel, nv = ops.nms_padded_per_class(cand[0], cand[2], cand[1], 100, 0.5, MC.S_RANDOM)
    for a, b in zip(out, (cand[0], cand[1], cand[2], sel, nv)):
        assert torch.equal(a, b)
    layer = YoloNmsLayer(100, 0.5, MC.S_RANDOM, multi_label=True, per_class=True)
    assert all(torch.equal(a, b) for a, b in zip(layer(dec), out)) and int(nv.min()) > 0


# ------------------------------------------------------------------------------------------------ 6. the net: 64 x 64, the synthetic weights
# S = 0.03: on this input the synthetic (random-init) weights give some tens of candidates per image, below the N = 252 boxes of the plan,
# several boxes among them with two or more labels -- asserted below.  At 0.02 an image has about 490 candidates, at 0.05 four.
NET_S, NET_M, NET_IOU, NET_SCORE = 64, 100, 0.5, 0.03
NET_N = 252


def _net(rt, program, weights, dtype="f32", batch=2, size=NET_S):
    from yolo_v3_tf2_amd import _lib
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(batch, size, {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16}[dtype])
    return net


def _by_hand(net, xd, anchors, K, per_class, M=NET_M, S=NET_SCORE):
    """forward -> decode_candidates -> _nms -> pack -> index rewrite, every call made by hand -> (packed, nv, candidates)."""
    from yolo_v3_tf2_amd import ops
    grids = net.forward(xd)
    cand = ops.decode_candidates(grids, anchors, 80, S, K)
    sel, nv = ops._nms(cand[0], cand[2], M, NET_IOU, S, classes=cand[1] if per_class else None)
    packed = ops.candidate_sources(ops._pack(cand[0], cand[1], cand[2], sel, nv), nv, cand[3])
    return packed, nv, cand, grids


def _shared_boxes(packed, nv):
    """Boxes that appear in two or more valid rows of their image."""
    return sum(int((np.bincount(packed[b, :nv[b], 6], minlength=1) >= 2).sum()) for b in range(len(nv)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_net_detect_follows_the_property(rt, program, weights, anchors, dtype):
    from oracle import oracle as O
    net, xd = _net(rt, program, weights, dtype), _cuda(MC.net_input(NET_S))
    assert net.multi_label is False and net.multi_label_capacity == 0
    single = [t.clone() for t in net.detect(xd, anchors, NET_M, NET_IOU, NET_SCORE)]      # of a net that never had the switch set
    with pytest.raises(rt.Y3Error, match="no multi-label"):
        net.multi_label_totals
    for per_class in (False, True):
        net.nms_per_class = per_class
        for binding in (False, True):
            net.multi_label = True
            net.multi_label_capacity = 0
            full = net.detect(xd, anchors, NET_M, NET_IOU, NET_SCORE)
            totals = net.multi_label_totals.cpu().numpy()
            assert totals.shape == (2,) and (totals > 4).all() and (totals <= NET_N).all(), totals
            K = int(totals.min()) // 2 if binding else NET_N
            net.multi_label_capacity = K if binding else 0
            assert net.multi_label is True and net.multi_label_capacity == (K if binding else 0)
            packed, nv = net.detect(xd, anchors, NET_M, NET_IOU, NET_SCORE)
            want, want_nv, cand, grids = _by_hand(net, xd, anchors, K, per_class)
            assert torch.equal(nv, want_nv) and torch.equal(packed, want)
            assert torch.equal(net.multi_label_totals, cand[4]) and np.array_equal(cand[4].cpu().numpy(), totals)
            assert binding == bool((totals > K).all())
            if not binding:
                assert torch.equal(packed, full[0]) and torch.equal(nv, full[1])
            # ... and the restatement on the device's own decode of the same grids
            dec = tuple(t.cpu().numpy() for t in rt.yolo_decode(grids, anchors, 80))
            ref = detect_multi_label_ref(*dec, NET_SCORE, K, NET_M, NET_IOU, per_class, O.nms_padded)
            assert np.array_equal(packed.cpu().numpy(), ref[0]) and np.array_equal(nv.cpu().numpy(), ref[1]) and np.array_equal(totals, ref[2])
            p, n = packed.cpu().numpy(), nv.cpu().numpy()
            print(dtype, "per_class" if per_class else "agnostic", "K =", K, "totals", totals.tolist(), "num_valid", n.tolist(),
                  "single-label num_valid", single[1].tolist(), "boxes in two or more rows", _shared_boxes(p, n))
            if per_class and not binding:
                assert _shared_boxes(p, n) >= 3, "several boxes carry two or more labels"
                assert (n > single[1].cpu().numpy()).all()
    # a graph captured with the switch on keeps it after the switch is flipped
    net.multi_label_capacity = 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net.detect(xd, anchors, NET_M, NET_IOU, NET_SCORE)
    torch.cuda.current_stream().wait_stream(side)
    eager = [t.clone() for t in net.detect(xd, anchors, NET_M, NET_IOU, NET_SCORE)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gp, gn = net.detect(xd, anchors, NET_M, NET_IOU, NET_SCORE)
    net.multi_label = False
    net.nms_per_class = False
    assert net.multi_label is False
    gp.zero_()
    gn.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(gp, eager[0]) and torch.equal(gn, eager[1])
    # off again: the rows the net gave before the switch was ever set, bit for bit
    again = net.detect(xd, anchors, NET_M, NET_IOU, NET_SCORE)
    assert torch.equal(again[0], single[0]) and torch.equal(again[1], single[1])
    for bad in (1, "on", None):
        with pytest.raises(TypeError):
            net.multi_label = bad
    for bad in (True, 2.5, "3", None):
        with pytest.raises(TypeError):
            net.multi_label_capacity = bad
    with pytest.raises(rt.Y3Error):
        net.multi_label_capacity = -1
    net.multi_label, net.multi_label_capacity = True, NET_N + 1
    with pytest.raises(rt.Y3Error, match="exceeds"):
        net.detect(xd, anchors, NET_M, NET_IOU, NET_SCORE)
    net.nms_per_class, net.multi_label_capacity = True, 0
    with pytest.raises(rt.Y3Error, match="iou_threshold must be > 0"):
        net.detect(xd, anchors, NET_M, 0.0, NET_SCORE)


def test_detect_model_follows_the_model_switch(rt, program, weights, anchors):
    """core.parse_model.YoloModel.set_multi_label: both routes of inference.DetectModel give the 5-tuple over candidates."""
    from yolo_v3_tf2_amd.core.parse_model import YoloModel
    from yolo_v3_tf2_amd.inference import DetectModel, Inference
    x = MC.net_input(NET_S)
    model = YoloModel(program)
    model.set_weights_dict(weights)
    model.set_nms_per_class(True)
    outs = {}
    for fused in (False, True):
        det = DetectModel(model, anchors, 80, NET_M, NET_IOU, NET_SCORE, fused=fused)
        for on in (False, True):
            model.set_multi_label(on)
            assert model._device_net().multi_label is on
            outs[fused, on] = det.predict(x)
    for on in (False, True):
        for a, b in zip(outs[False, on], outs[True, on]):
            assert np.array_equal(a, b)
    bb, cls, sc, sel, nv = outs[True, True]
    assert bb.shape == (2, NET_N, 4) and cls.shape == sc.shape == (2, NET_N) and (nv > outs[True, False][4]).all()
    net = model._device_net()
    net.multi_label = True
    packed, pnv = (t.cpu().numpy() for t in net.detect(_cuda(x), anchors, NET_M, NET_IOU, NET_SCORE))
    for b in range(2):      # the gather of the reference works unchanged over the candidates
        boxes, classes, scores = Inference.gather_valid_detections_results(bb[b], cls[b], sc[b], sel[b], int(nv[b]))
        assert nv[b] == pnv[b] and np.array_equal(boxes.view(np.int32), packed[b, :nv[b], :4])
        assert np.array_equal(scores.view(np.int32), packed[b, :nv[b], 4]) and np.array_equal(classes, packed[b, :nv[b], 5])


STREAM_LOW, STREAM_M = 0.1, 600       # 160 x 160: 140 to 190 candidates per image of the N = 1575 slots, about 20 boxes with two or more labels


def test_streams_follow_the_property(rt, program, weights, anchors):
    """detect_stream and evaluate_stream(ap=..., loss False and True) with the switch on, batches of 4, 4 and 3 frames at S = 160: the rows
    are those of Net.detect per batch; the counters and the AP are the host classes' on those rows.  loss=True takes the composed route,
    which picks the candidates op itself.  Then the overflow: detect_stream warns once, evaluate_stream raises."""
    from tests.test_evaluate_gpu import STREAM_S, _ground_truth_from, _staged, _stream_batches
    from yolo_v3_tf2_amd.evaluate_detections import average_precision, match_detections, sweep_counters
    S, batches, M, low = STREAM_S, _stream_batches(), STREAM_M, STREAM_LOW
    thresholds = [low, 0.15, 0.2]
    net = _net(rt, program, weights, batch=4, size=S)
    net.nms_per_class = True
    rows_off = [tuple(np.array(a) for a in r) for r in net.detect_stream(batches, anchors, M, 0.5, low)]
    net.multi_label = True
    want_rows, totals = [], []
    for frames in batches:
        packed, nv = net.detect(_staged(rt, frames, S, False), anchors, M, 0.5, low)
        totals += net.multi_label_totals[:len(frames)].tolist()
        want_rows.append((packed.cpu().numpy(), nv.cpu().numpy()))
    assert max(totals) <= 1575 and min(totals) > 50, totals
    with warnings.catch_warnings():
        warnings.simplefilter("error")      # no image is truncated: no warning
        rows_on = [tuple(np.array(a) for a in r) for r in net.detect_stream(batches, anchors, M, 0.5, low)]
    assert len(rows_on) == 3
    for got, want in zip(rows_on, want_rows):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert all((on[1] > off[1]).all() for on, off in zip(rows_on, rows_off)), "more detections than one label per box gives"
    assert sum(_shared_boxes(*r) for r in want_rows) > 10
    rng = np.random.default_rng(5)
    gts = [_ground_truth_from(*rows, rng, first=4 * i) for i, rows in enumerate(want_rows)]
    G = max(len(c) for g in gts for _, c in g)
    counters, records, gt_totals = 0, [], 0
    for (packed, nv), gt in zip(want_rows, gts):
        gt_packed = rt.pack_ground_truth(gt, G)
        counters = counters + sweep_counters(packed, nv, *gt_packed, 80, 0.5, thresholds)
        r, t = match_detections(packed, nv, *gt_packed, 80, [0.5, 0.75])
        records.append(r)
        gt_totals = gt_totals + t
    want_ap = average_precision(np.concatenate(records), gt_totals, 80, 2)
    for loss in (False, True):      # y3_net_detect's own route, then the composed one
        out = net.evaluate_stream(batches, gts, anchors, M, 0.5, thresholds, 80, loss=loss, ap=[0.5, 0.75])
        got_counters, got_ap = out[0], out[-1]
        assert np.array_equal(got_counters, counters), loss
        assert np.array_equal(got_ap["ap"], want_ap["ap"], equal_nan=True) and got_ap["mAP"] == want_ap["mAP"], loss
        assert (got_ap["images"], got_ap["errors"]) == (11, 0) and 0.0 < got_ap["mAP"] <= 1.0
    # overflow: every image has more than 50 candidates
    net.multi_label_capacity = 50
    with pytest.warns(RuntimeWarning, match="11 image") as caught:
        cut = [tuple(np.array(a) for a in r) for r in net.detect_stream(batches, anchors, M, 0.5, low)]
    assert len([w for w in caught if "multi-label candidates" in str(w.message)]) == 1 and len(cut) == 3 and all((c[1] <= 50).all() for c in cut)
    for loss in (False, True):
        with pytest.raises(rt.Y3Error, match="more multi-label candidates than the capacity 50"):
            net.evaluate_stream(batches, gts, anchors, M, 0.5, thresholds, 80, loss=loss)


def test_detect_stream_with_tiles(rt, program, weights, anchors):
    """Sliced inference with the switch on: every tile image is detected in multi-label mode and the merge consumes the packed rows
    unchanged -- equal to the calls of tests/test_tiles_gpu._composed, whose Net.detect follows the switch."""
    from tests.test_tiles_gpu import TILES, _composed, _stream_batches
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(3, NET_S)
    batches = _stream_batches()
    net.nms_per_class, net.tiles = True, TILES
    off = [tuple(np.array(a) for a in r) for r in net.detect_stream(batches, anchors, NET_M, NET_IOU, NET_SCORE)]
    net.multi_label = True
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        rows = [tuple(np.array(a) for a in r) for r in net.detect_stream(batches, anchors, NET_M, NET_IOU, NET_SCORE)]
    differs = 0
    for frames, got, single in zip(batches, rows, off):
        want, tile_rows, T = _composed(rt, net, frames, anchors, False, score=NET_SCORE)
        assert T == 7 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        differs += int(not np.array_equal(got[0], single[0]))
    assert differs >= 1, "the merged rows differ from the single-label ones"
