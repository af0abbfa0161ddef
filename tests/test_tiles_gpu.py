"""Sliced inference on the device: preprocess_tiles on windows against preprocess_batch on contiguous crops, merge_tiles_kernel + the
existing NMS and pack against tiles.merge_tile_detections_ref (which tests/test_tiles_host.py ties to a brute-force loop), and
Net.detect_stream / evaluate_stream with Net.tiles set against the same calls composed by hand.  Destinations, outputs and workspaces are
poisoned before every call; every comparison is exact, every word."""
import ctypes as C_

import numpy as np
import pytest

from tests import tile_cases as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from yolo_v3_tf2_amd import input_stage as I, ops as OPS, tiles as TL  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.int32)


# ------------------------------------------------------------------------------------------------ the input stage
def _tile_descs(rt, descs, windows):
    """Hand-written windows per frame -> the tile descriptor array, in the order tile_cases.crops lists the crops."""
    out = np.zeros(sum(len(w) for w in windows), I.TILE_DESC_DTYPE)
    k = 0
    for d, ws in zip(descs, windows):
        for win in ws:
            out[k] = (d["offset"], d["height"], d["width"], d["channels"], d["mode"], *win)
            k += 1
    return out


def _tiles_against_crops(rt, frames, windows, mode, letterbox, canvas):
    """preprocess_tiles into slots 1 .. n of a batch of n + 2 slots filled with NaN words; -> (tiles, the same crops through preprocess_batch)."""
    blob, descs = rt.pack_images(frames, mode, letterbox=letterbox)
    tdescs = _tile_descs(rt, descs, windows)
    n = len(tdescs)
    batch = torch.full((n + 2, *canvas, 3), float("nan"), device="cuda")
    I.preprocess_tiles(_cuda(blob), tdescs, batch, 1)
    cblob, cdescs = rt.pack_images(K.crops(frames, windows), mode, letterbox=letterbox)
    want = torch.full((n, *canvas, 3), float("nan"), device="cuda")
    rt.preprocess_batch(_cuda(cblob), cdescs, want, 0)
    torch.cuda.synchronize()
    assert torch.isnan(batch[0]).all() and torch.isnan(batch[-1]).all(), "a neighbouring slot was written"
    assert not torch.isnan(want).any()
    return batch[1:-1], want, tdescs


@pytest.mark.parametrize("canvas", K.CANVASES)
@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_tiles_are_bit_equal_to_preprocess_batch_on_contiguous_crops(rt, mode, letterbox, canvas):
    """Frames 97x131x3, 64x48x4 and 1x1x3, windows including 1x1, the corners and the whole frame."""
    frames, windows = K.input_case(mode, letterbox, seed=10 * mode)
    assert all(K.fits(ch, cw, canvas) for ws in windows for _, _, ch, cw in ws)
    got, want, tdescs = _tiles_against_crops(rt, frames, windows, mode, letterbox, canvas)
    assert np.array_equal(_bits(got), _bits(want))
    if letterbox:       # the geometry is the crop's: a 1 x 1 window fills the canvas' short side, a strip is padded
        geoms = I.tile_letterbox_geometries(tdescs, canvas)
        assert (geoms[0] == [min(canvas), min(canvas), 0, (canvas[1] - min(canvas)) // 2]).all()
        assert (got[0] == 0).any() == (canvas[0] != canvas[1])


def test_tiles_on_a_canvas_that_takes_the_scalar_stores(rt):
    """5 x 7 pixels are no multiple of four: one pixel and three scalar stores per thread, as in preprocess_batch."""
    frames, windows = K.input_case(1, True, seed=3)
    got, want, _ = _tiles_against_crops(rt, frames, windows, 1, True, (5, 7))
    assert np.array_equal(_bits(got), _bits(want))


def test_more_tiles_than_one_launch_holds(rt):
    """150 windows of one frame: launches of 72, 72 and 6 tiles (preprocess_batch takes its 150 crops in the same three launches)."""
    rng = np.random.default_rng(7)
    f = K.frame((97, 131, 3), 2, 5)
    wins = []
    for _ in range(150):
        ch, cw = int(rng.integers(1, 98)), int(rng.integers(1, 132))
        wins.append((int(rng.integers(0, 97 - ch + 1)), int(rng.integers(0, 131 - cw + 1)), ch, cw))
    wins[71], wins[72], wins[143], wins[144], wins[149] = (0, 0, 97, 131), (96, 130, 1, 1), (0, 0, 1, 131), (0, 130, 97, 1), (40, 50, 7, 9)
    got, want, _ = _tiles_against_crops(rt, [f], [wins], 2, False, (64, 64))
    assert np.array_equal(_bits(got), _bits(want))


def test_preprocess_tiles_in_a_captured_graph(rt):
    frames, windows = K.input_case(1, True, seed=1)
    blob, descs = rt.pack_images(frames, 1, letterbox=True)
    tdescs = _tile_descs(rt, descs, windows)
    blob_dev = _cuda(blob)
    batch = torch.zeros((len(tdescs), 64, 96, 3), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        I.preprocess_tiles(blob_dev, tdescs, batch, 0)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        I.preprocess_tiles(blob_dev, tdescs, batch, 0)
    for seed in (2, 1):     # other pixels of the same shapes in the same blob
        frames2, _ = K.input_case(1, True, seed=seed)
        blob2, descs2 = rt.pack_images(frames2, 1, letterbox=True)
        assert np.array_equal(descs2, descs)
        blob_dev.copy_(_cuda(blob2))
        batch.fill_(float("nan"))
        g.replay()
        want = torch.zeros_like(batch)
        cblob, cdescs = rt.pack_images(K.crops(frames2, windows), 1, letterbox=True)
        rt.preprocess_batch(_cuda(cblob), cdescs, want, 0)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(batch), _bits(want))


def test_preprocess_tiles_refusals_enqueue_nothing(rt):
    frames, windows = K.input_case(1, False)
    blob, descs = rt.pack_images(frames, 1)
    tdescs = _tile_descs(rt, descs, windows)
    batch = torch.full((len(tdescs), 64, 64, 3), float("nan"), device="cuda")
    blob_dev = _cuda(blob)
    for field, value in (("y0", 97), ("cw", 132), ("ch", 0), ("channels", 5), ("mode", 7), ("offset", 10**9)):
        bad = tdescs.copy()
        bad[field][len(bad) - 1] = value
        with pytest.raises(rt.Y3Error, match=f"tile {len(bad) - 1}"):
            I.preprocess_tiles(blob_dev, bad, batch, 0)
    with pytest.raises(rt.Y3Error):
        I.preprocess_tiles(blob_dev, tdescs, batch, 1)      # one slot short
    torch.cuda.synchronize()
    assert torch.isnan(batch).all()


# ------------------------------------------------------------------------------------------------ the merge
def _layout(F, T, M):
    """Byte offsets of the candidate arrays and the selected indices in the workspace (include/y3.h: every part 16-byte aligned)."""
    N, up = T * M, lambda v: -(-v // 16) * 16
    cls = up(F * N * 16)
    scores = up(cls + F * N * 8)
    sel = up(scores + F * N * 4)
    return dict(boxes=0, cls=cls, scores=scores, sel=sel, nms=up(sel + F * M * 4))


def _merge(rt, case, per_class, T=K.T_IOU, S=K.S_LOW, check_workspace=True):
    """ops.merge_tile_detections into outputs filled with -1 and a workspace of exactly y3_merge_tiles_workspace_bytes filled with 0xFF,
    256 guard bytes behind it; the candidate arrays left in the workspace must be tile_candidates' in every word."""
    F, Tn, M = case["F"], case["T"], case["M"]
    need = OPS.merge_tiles_workspace_bytes(F, Tn, M)
    buf = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    out = (torch.full((F, M, 7), -1, dtype=torch.int32, device="cuda"), torch.full((F,), -1, dtype=torch.int32, device="cuda"))
    OPS.merge_tile_detections(_cuda(case["packed"]), _cuda(case["nv"]), case["windows"], case["geoms"], case["frame_hw"], case["canvas"],
                             T, S, per_class=per_class, out=out, ws=buf[:need])
    torch.cuda.synchronize()
    assert (buf[need:] == 0xFF).all(), "written behind the workspace"
    if check_workspace:
        lay, N, ws = _layout(F, Tn, M), Tn * M, buf.cpu().numpy()
        boxes, scores, classes = TL.tile_candidates(case["packed"], case["nv"], case["windows"], case["geoms"], case["frame_hw"], F, Tn, case["canvas"])
        assert np.array_equal(ws[:F * N * 16].view(np.int32), boxes.view(np.int32).reshape(-1))
        assert np.array_equal(ws[lay["cls"]:lay["cls"] + F * N * 8].view(np.int64), classes.reshape(-1))
        assert np.array_equal(ws[lay["scores"]:lay["scores"] + F * N * 4].view(np.int32), scores.view(np.int32).reshape(-1))
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def _ref(case, per_class, T=K.T_IOU, S=K.S_LOW):
    return TL.merge_tile_detections_ref(case["packed"], case["nv"], case["windows"], case["geoms"], case["frame_hw"], case["F"], case["T"],
                                        case["canvas"], T, S, per_class=per_class)


def _same(got, want):
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert np.array_equal(got[0], want[0]), int((got[0] != want[0]).sum())


@pytest.mark.parametrize("per_class", [False, True])
@pytest.mark.parametrize("M", [1, 100])
@pytest.mark.parametrize("T", [1, 7, 64])
def test_merge_equals_the_restatement(rt, T, M, per_class):
    """Two frames (a crowded one, both caps binding, and a sparse one) -- three with 64 tiles, so that the 192 tile images take more than one
    table -- an empty tile in each, an over-range and a negative num_valid, poisoned rows behind num_valid, letterboxed windows on 64 x 96."""
    F = 3 if T == 64 else 2
    case = K.merge_case(F, T, M, seed=40 + 2 * T)
    if T > 1:
        assert case["nv"].max() > M and (case["nv"].reshape(F, T)[:, 1] == 0).all()
    if T > 2:
        assert case["nv"].min() < 0
    got = _merge(rt, case, per_class)
    _same(got, _ref(case, per_class))
    assert T == 1 or got[1].max() == M, got[1]                  # the cap of the merge binds on the crowded frame ...
    assert T != 7 or M == 1 or 0 < got[1].min() < M, got[1]     # ... and not on the sparse one


def test_merge_of_all_empty_frames_and_of_one_empty_frame(rt):
    for per_class in (False, True):
        got = _merge(rt, K.empty_case(3, 7, 10), per_class)
        assert not got[0].any() and not got[1].any()
    case = K.merge_case(2, 7, 10, seed=2)
    case["nv"][7:] = 0
    got = _merge(rt, case, False)
    _same(got, _ref(case, False))
    assert got[1][0] > 0 and got[1][1] == 0


def test_merge_on_identity_geometries_and_whole_axis_windows(rt):
    """Every tile the whole frame, stretched: the mapping copies, tile 2 repeats tile 0 word for word and loses every row to its twin."""
    case = K.identity_case(M=30)
    for per_class in (False, True):
        got = _merge(rt, case, per_class)
        _same(got, _ref(case, per_class))
        idx = got[0][0, :got[1][0], 6]
        assert got[1][0] > 2 and not ((idx >= 60) & (idx < 90)).any()
        for row in got[0][0, :got[1][0]]:
            t, r = divmod(int(row[6]), 30)
            assert np.array_equal(row[:6], case["packed"][t, r, :6])
    # one axis whole, the other not; one axis identity, the other not (stretched windows: geometry the whole canvas)
    case = K.merge_case(2, 7, 20, seed=9, letterbox=False, canvas=(64, 64))
    _same(_merge(rt, case, False), _ref(case, False))


def test_merge_thresholds(rt):
    """Other thresholds, among them the agnostic rule's T <= 0 quirk (against the C oracle's rule: the default restatement covers T > 0 only)
    and a negative score threshold, at which the zero rows of empty tiles are candidates that are kept and never selected."""
    from oracle import oracle as O
    case = K.merge_case(2, 7, 20, seed=13)
    for T, S in ((0.3, 0.4), (0.9, 0.0), (0.5, -1.0)):
        for per_class in (False, True):
            _same(_merge(rt, case, per_class, T, S), _ref(case, per_class, T, S))
    want = TL.merge_tile_detections_ref(case["packed"], case["nv"], case["windows"], case["geoms"], case["frame_hw"], 2, 7, case["canvas"], 0.0, 0.05,
                                        agnostic_nms=O.nms_padded)
    _same(_merge(rt, case, False, 0.0, 0.05), want)


def test_merge_in_a_captured_graph(rt):
    """The tables are frozen into the graph; the rows and counts are read at replay."""
    first, second = K.merge_case(2, 7, 20, seed=1), K.merge_case(2, 7, 20, seed=3)
    assert np.array_equal(first["windows"], second["windows"]) and np.array_equal(first["geoms"], second["geoms"])
    packed, nv = _cuda(first["packed"]), _cuda(first["nv"])
    ws = torch.full((OPS.merge_tiles_workspace_bytes(2, 7, 20),), 0xFF, dtype=torch.uint8, device="cuda")
    out = (torch.empty((2, 20, 7), dtype=torch.int32, device="cuda"), torch.empty((2,), dtype=torch.int32, device="cuda"))
    args = (first["windows"], first["geoms"], first["frame_hw"], first["canvas"], K.T_IOU, K.S_LOW)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        OPS.merge_tile_detections(packed, nv, *args, per_class=True, out=out, ws=ws)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        OPS.merge_tile_detections(packed, nv, *args, per_class=True, out=out, ws=ws)
    for case in (second, first, second):
        packed.copy_(_cuda(case["packed"]))
        nv.copy_(_cuda(case["nv"]))
        out[0].fill_(-1)
        out[1].fill_(-1)
        ws.fill_(0xFF)
        g.replay()
        torch.cuda.synchronize()
        _same((out[0].cpu().numpy(), out[1].cpu().numpy()), _ref(case, True))


def test_merge_refusals_enqueue_nothing(rt):
    """Every refusal of tests/test_tiles_host.py::test_merge_checks_that_need_no_device again, on real buffers: outputs and workspace keep their
    poison, so the checks -- those of the NMS call that would follow included -- come before the first launch."""
    from yolo_v3_tf2_amd import _lib
    lib = _lib.load()
    case = K.merge_case(2, 3, 4, seed=1, canvas=(64, 64))
    packed, nv = _cuda(case["packed"]), _cuda(case["nv"])
    need = OPS.merge_tiles_workspace_bytes(2, 3, 4)
    ws = torch.full((need + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.full((2, 4, 7), -1, dtype=torch.int32, device="cuda")
    nv_out = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    p = lambda t, off=0: C_.c_void_p(t.data_ptr() + off)
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(C_.POINTER(C_.c_int32))
    good = dict(packed=p(packed), nv=p(nv), windows=case["windows"], geoms=case["geoms"], hw=case["frame_hw"], F=2, T=3, M=4, Hc=64, Wc=64,
                mode=0, iou=0.5, score=0.05, out=p(out), nv_out=p(nv_out), ws=p(ws), bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        return lib.y3_merge_tile_detections(a["packed"], a["nv"], i32(a["windows"]), i32(a["geoms"]), i32(a["hw"]), a["F"], a["T"], a["M"],
                                            a["Hc"], a["Wc"], a["mode"], a["iou"], a["score"], a["out"], a["nv_out"], a["ws"], a["bytes"],
                                            _lib.stream_ptr())

    def edited(name, row, col, value):
        t = np.array(case[name], np.int32)
        t[row, col] = value
        return t

    bad = [dict([(k, None)]) for k in ("packed", "nv", "windows", "geoms", "hw", "out", "nv_out", "ws")]
    bad += [dict(F=0), dict(T=0), dict(T=65), dict(M=0), dict(M=1025), dict(Hc=0), dict(Wc=0), dict(mode=2), dict(mode=1, iou=0.0),
            dict(mode=1, iou=float("nan")), dict(iou=0.0, score=-1.0), dict(hw=edited("frame_hw", 1, 0, 0)),
            dict(windows=edited("windows", 5, 3, 0)), dict(windows=edited("windows", 0, 2, 98)), dict(geoms=edited("geoms", 3, 0, 0)),
            dict(geoms=edited("geoms", 1, 2, 63)), dict(bytes=need - 1), dict(ws=p(ws, 8)), dict(packed=p(packed, 2)), dict(out=p(out, 1))]
    for kw in bad:
        assert call(**kw) == _lib.Y3_ERR_INVALID, kw
        assert b"y3_merge_tile_detections" in lib.y3_last_error()
    torch.cuda.synchronize()
    assert (out == -1).all() and (nv_out == -1).all() and (ws == 0xFF).all()
    assert call() == 0
    torch.cuda.synchronize()
    _same((out.cpu().numpy(), nv_out.cpu().numpy()), _ref(case, False))
    # the Python wrapper refuses the tensors and tables it can see are wrong
    for kw in (dict(windows=case["windows"][:-1]), dict(geoms=case["geoms"][:, :3]), dict(frame_hw=case["frame_hw"].reshape(-1))):
        a = dict(dict(windows=case["windows"], geoms=case["geoms"], frame_hw=case["frame_hw"]), **kw)
        with pytest.raises(rt.Y3Error):
            OPS.merge_tile_detections(packed, nv, a["windows"], a["geoms"], a["frame_hw"], 64, 0.5, 0.05)
    with pytest.raises(rt.Y3Error):
        OPS.merge_tile_detections(packed, nv[:-1], case["windows"], case["geoms"], case["frame_hw"], 64, 0.5, 0.05)
    with pytest.raises(rt.Y3Error, match="iou_threshold must be > 0"):
        OPS.merge_tile_detections(packed, nv, case["windows"], case["geoms"], case["frame_hw"], 64, 0.0, 0.05, per_class=True)


# ------------------------------------------------------------------------------------------------ the net: 64 x 64, the synthetic weights
NET_S, NET_M, NET_IOU, NET_SCORE = 64, 100, 0.5, 0.005
TILES = (2, 3, 8, True)
STREAM_SHAPES = [(97, 131, 3), (64, 48, 4), (120, 90, 3), (33, 200, 3)]


def _stream_batches():
    """Batches of 3, 3 and 2 uint8 frames over four shapes, the second batch in another order."""
    rng = np.random.default_rng(64)
    return [[rng.integers(0, 256, STREAM_SHAPES[k], dtype=np.uint8) for k in ks] for ks in ([0, 1, 2], [3, 2, 1], [0, 3])]


@pytest.fixture(scope="module")
def net(rt, program, weights):
    n = rt.Net(program)
    n.load_weights(weights)
    n.plan(3, NET_S)
    return n


def _composed(rt, net, frames, anchors, letterbox, tiles=TILES, merge_iou=NET_IOU, score=NET_SCORE):
    """One batch, every call made by hand: pack, upload once, preprocess_tiles, Net.detect on the tile batch, merge_tile_detections."""
    blob, descs = rt.pack_images(frames, 1, letterbox=letterbox)
    tdescs, windows = I.tile_descs(frames, descs, *tiles)
    T = len(tdescs) // len(frames)
    batch = torch.empty((len(tdescs), NET_S, NET_S, 3), device="cuda")
    I.preprocess_tiles(_cuda(blob), tdescs, batch, 0)
    packed, nv = net.detect(batch, anchors, NET_M, NET_IOU, score)
    frame_hw = np.array([f.shape[:2] for f in frames], np.int32)
    merged, mnv = OPS.merge_tile_detections(packed, nv, windows, I.tile_letterbox_geometries(tdescs, NET_S), frame_hw, NET_S, merge_iou, score,
                                           per_class=net.nms_per_class)
    return (merged.cpu().numpy(), mnv.cpu().numpy()), (packed.cpu().numpy(), nv.cpu().numpy()), T


@pytest.mark.parametrize("letterbox", [False, True])
def test_detect_stream_with_tiles_equals_the_composed_calls(rt, net, anchors, letterbox):
    batches = _stream_batches()
    for per_class, merge_iou in ((False, None), (True, 0.3)):
        net.nms_per_class, net.tiles, net.merge_iou_threshold = per_class, TILES, merge_iou
        try:
            assert net.tiles == TILES and net.merge_iou_threshold == merge_iou
            rows = [tuple(np.array(a) for a in r) for r in net.detect_stream(batches, anchors, NET_M, NET_IOU, NET_SCORE, letterbox=letterbox)]
            assert len(rows) == 3 and net.max_batch >= 21
            total = 0
            for frames, got in zip(batches, rows):
                want, tile_rows, T = _composed(rt, net, frames, anchors, letterbox, merge_iou=NET_IOU if merge_iou is None else merge_iou)
                assert T == 7 and got[0].shape == (len(frames), NET_M, 7) and got[1].shape == (len(frames),)
                _same(got, want)
                assert (got[1] > 0).all() and (got[1] <= np.minimum(tile_rows[1].reshape(len(frames), 7).sum(1), NET_M)).all()
                assert len({int(i) // NET_M for b in range(len(frames)) for i in got[0][b, :got[1][b], 6]}) > 1, "rows of more than one tile survive"
                total += int(got[1].sum())
            print("tiles", letterbox, per_class, [r[1].tolist() for r in rows])
        finally:
            net.nms_per_class, net.tiles, net.merge_iou_threshold = False, None, None
        assert total > 8


@pytest.mark.parametrize("letterbox", [False, True])
def test_one_whole_frame_tile_is_the_untiled_stream(rt, net, anchors, letterbox):
    """net.tiles = (1, 1, 0, False): every word of the untiled rows but the index, which counts the rows.  With letterbox=True the untiled route
    computes x * 64 / 64 on the axis that fills the canvas, where the merge copies: the same value on a power-of-two canvas."""
    batches = _stream_batches()
    plain = [tuple(np.array(a) for a in r) for r in net.detect_stream(batches, anchors, NET_M, NET_IOU, NET_SCORE, letterbox=letterbox)]
    net.tiles = (1, 1, 0, False)
    try:
        tiled = [tuple(np.array(a) for a in r) for r in net.detect_stream(batches, anchors, NET_M, NET_IOU, NET_SCORE, letterbox=letterbox)]
    finally:
        net.tiles = None
    for (pp, pn), (tp, tn) in zip(plain, tiled):
        assert np.array_equal(pn, tn) and pn.max() > 0
        assert np.array_equal(pp[:, :, :6], tp[:, :, :6])
        for b, n in enumerate(tn):
            assert tp[b, :n, 6].tolist() == list(range(n)) and not tp[b, n:].any()


def test_evaluate_stream_with_tiles_equals_the_composed_calls(rt, net, anchors):
    """Counters at three thresholds and AP at two IoUs from evaluate_stream with net.tiles set == the host classes on the rows composed by hand at the
    lowest threshold; and, the one-pass property on the device, the counters at a higher threshold == those of rows composed at that threshold."""
    from tests.test_evaluate_gpu import _ground_truth_from
    from yolo_v3_tf2_amd.evaluate_detections import average_precision, match_detections, sweep_counters
    batches, thresholds = _stream_batches(), [NET_SCORE, 0.02, 0.05]
    composed = [_composed(rt, net, frames, anchors, True)[0] for frames in batches]
    rng = np.random.default_rng(5)
    gts = [_ground_truth_from(*rows, rng, first=3 * i) for i, rows in enumerate(composed)]
    G = max(len(c) for g in gts for _, c in g)
    counters, records, totals = 0, [], 0
    for (packed, nv), gt in zip(composed, gts):
        gt_packed = rt.pack_ground_truth(gt, G)
        counters = counters + sweep_counters(packed, nv, *gt_packed, 80, 0.5, thresholds)
        r, t = match_detections(packed, nv, *gt_packed, 80, [0.5, 0.75])
        records.append(r)
        totals = totals + t
    want_ap = average_precision(np.concatenate(records), totals, 80, 2)
    net.tiles = TILES
    try:
        got_counters, got_ap = net.evaluate_stream(batches, gts, anchors, NET_M, NET_IOU, thresholds, 80, letterbox=True, ap=[0.5, 0.75])
    finally:
        net.tiles = None
    assert np.array_equal(got_counters, counters)
    assert np.array_equal(got_ap["ap"], want_ap["ap"], equal_nan=True) and got_ap["mAP"] == want_ap["mAP"]
    assert (got_ap["images"], got_ap["errors"]) == (8, 0) and 0.0 < got_ap["mAP"] <= 1.0
    assert got_counters[0, 160:240].sum() > 0, "true positives at the lowest threshold"
    for k, t in enumerate(thresholds[1:], 1):
        higher = 0
        for frames, gt in zip(batches, gts):
            packed, nv = _composed(rt, net, frames, anchors, True, score=t)[0]
            higher = higher + sweep_counters(packed, nv, *rt.pack_ground_truth(gt, G), 80, 0.5, [t])
        assert np.array_equal(got_counters[k], higher[0]), t


def test_tiles_refusals_of_the_streams(rt, net, anchors):
    batches = _stream_batches()
    gts = [[(np.array([[.2, .2, .6, .6]], np.float32), np.array([3], np.int32))] * len(b) for b in batches]
    for bad in ((0, 3, 0, False), (2, 9, 0, False), (2, 3, -1, False), (8, 8, 0, True), (2, 3, 0), 7):
        with pytest.raises(rt.Y3Error, match="tiles"):
            net.tiles = bad
    with pytest.raises(TypeError):
        net.merge_iou_threshold = "0.5"
    assert net.tiles is None and net.merge_iou_threshold is None
    net.merge_iou_threshold = 0.5
    try:
        with pytest.raises(rt.Y3Error, match="merge_iou_threshold needs tiles"):
            list(net.detect_stream(batches, anchors, NET_M, NET_IOU, NET_SCORE))
    finally:
        net.merge_iou_threshold = None
    net.tiles = TILES
    try:
        with pytest.raises(rt.Y3Error, match="loss=True cannot be combined with tiles"):
            net.evaluate_stream(batches, gts, anchors, NET_M, NET_IOU, [0.1], 80, loss=True)
        net.tiles = (2, 3, 40, True)
        with pytest.raises(rt.Y3Error, match="y3_tile_grid"):      # the 33-row frame cannot overlap by 40
            list(net.detect_stream(batches, anchors, NET_M, NET_IOU, NET_SCORE))
    finally:
        net.tiles = None
    torch.cuda.synchronize()
    # the stage itself: its own class, the slots of max_batch * T images, the handle's tables
    stage = I.TiledInputStage(NET_S, 3, max(rt.packed_nbytes(b) for b in batches), TILES)
    handle = stage.submit(batches[2], 1, letterbox=True)
    assert isinstance(stage, rt.InputStage) and isinstance(handle, rt.StagedBatch) and stage.tiles_per_image == 7
    assert handle.frames == 2 and handle.batch.shape == (14, NET_S, NET_S, 3) and stage.slots[0].batch.shape[0] == 21
    assert handle.windows.shape == handle.geometry.shape == (14, 4) and handle.frame_hw.tolist() == [[97, 131], [33, 200]]
    stage.release(handle)
    torch.cuda.synchronize()
    plain = rt.InputStage(NET_S, 3, 1 << 20).submit(batches[2], 1)
    assert plain.frames == 2 and not hasattr(plain, "windows")


# ------------------------------------------------------------------------------------------------ the drivers
def test_inference_yaml_tiles_reach_the_tiled_stream(rt, weights, anchors, tmp_path, monkeypatch):
    """`tiles: [2, 2]`, `tile_overlap: 8`, `tile_overview: true` in the inference config: the image file's detections are those of
    Net.detect_stream with net.tiles = (2, 2, 8, True) on the decoded frame, in frame coordinates."""
    import os
    import yaml
    from yolo_v3_tf2_amd.core.utils import load_image_u8
    from yolo_v3_tf2_amd.inference import Inference
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "config/detect_config_coco.yaml")))
    assert Inference.tiles_from_config(cfg) is None                     # the packaged config leaves it off
    for k in ("model_config_file", "classes_name_file", "anchors_file", "image_file_path", "images_dir"):
        cfg[k] = os.path.join(root, cfg[k])
    cfg.update(image_size=64, output_dir=str(tmp_path / "out"), input_weights_path=None, nms_score_threshold=NET_SCORE)
    monkeypatch.chdir(tmp_path)                                         # build() writes model_inference_summary.txt
    inf = Inference()
    inf.tiles = Inference.tiles_from_config({"tiles": [2, 2], "tile_overlap": 8, "tile_overview": True})
    (bboxes, classes, scores, names), = inf(weights=weights, **cfg)
    model = inf.detect_model
    assert model.model.tiles == (2, 2, 8, True)
    net = model.model._device_net()
    assert net.canvas == (64, 64) and net.max_batch == 5
    frame = load_image_u8(cfg["image_file_path"])
    assert net.tiles == (2, 2, 8, True)
    (packed, nv), = net.detect_stream([[frame]], model.anchors_table, model.yolo_max_boxes, model.nms_iou_threshold, NET_SCORE)
    n = int(nv[0])
    assert n > 0 and len(names) == n
    assert np.array_equal(bboxes.view(np.int32), packed[0, :n, :4]) and np.array_equal(scores.view(np.int32), packed[0, :n, 4])
    assert np.array_equal(classes, packed[0, :n, 5])
    assert os.path.exists(tmp_path / "out" / "detect_0.jpg")


def test_evaluate_driver_with_tiles(rt, weights, tmp_path):
    """evaluate(on_device=True, ap=..., tiles=...) on the four-image TFRecord set of tests/test_evaluate_gpu.py: the keys of the detect
    config and the argument give the same results; they are not the untiled ones; all four images are counted."""
    from tests.test_evaluate_gpu import _same_results, _write_set
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev
    cfg = _write_set(tmp_path / "even", [2, 2, 2, 2], 21)
    plain = ev.evaluate(cfg, [0.05, 0.3], evaluate_iou_threshold=0.1, weights=weights, on_device=True)
    by_arg, ap_arg = ev.evaluate(cfg, [0.05, 0.3], evaluate_iou_threshold=0.1, weights=weights, on_device=True, ap=[0.5], tiles=(2, 2, 16, True))
    by_key, ap_key = ev.evaluate(dict(cfg, tiles=[2, 2], tile_overlap=16, tile_overview=True), [0.05, 0.3], evaluate_iou_threshold=0.1,
                                 weights=weights, on_device=True, ap=[0.5])
    _same_results(by_arg, by_key)
    assert np.array_equal(ap_arg["ap"], ap_key["ap"], equal_nan=True) and ap_arg["images"] == 4
    c = by_arg[0][3]
    assert c["examples"] == 4 and c["gts"].sum() == 8 and c["preds"].sum() > 0
    assert not np.array_equal(c["preds"], plain[0][3]["preds"])
    with pytest.raises(ValueError, match="tiles"):
        ev.evaluate(cfg, [0.05], weights=weights, on_device=True, loss=True, tiles=(2, 2, 0, False))
