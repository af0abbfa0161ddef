"""Sliced inference without a GPU: the window grid (y3_tile_grid against tiles.tile_grid and the properties the rule implies), the
tiles' letterbox geometry, the restatement of the merge (tiles.merge_tile_detections_ref) against a brute-force loop, the one-pass
property over two NMS stages, and the argument checks of the new C calls that need no device."""
import ctypes as C

import numpy as np
import pytest

from tests import tile_cases as K

from yolo_v3_tf2_amd import tiles as TL  # noqa: E402
from yolo_v3_tf2_amd.core.utils import letterbox_geometry, unletterbox_boxes  # noqa: E402
from yolo_v3_tf2_amd.nms_per_class import nms_padded_per_class_ref  # noqa: E402

OVERLAPS = (0, 1, 7, 64)


def _axis_ok(starts, length, e, ov):
    starts = np.asarray(starts)
    return (starts[0] == 0 and starts[-1] + length == e and (starts >= 0).all() and (starts + length <= e).all() and
            (np.diff(starts) >= 0).all() and (starts[:-1] + length - starts[1:] >= ov).all())


# ------------------------------------------------------------------------------------------------ the grid
def test_grid_properties_for_every_frame_up_to_200():
    """Per axis the rule is separable, so every (extent, count, overlap) is checked once: inside the frame, first at 0, last ends at
    e, neighbours overlap by at least ov -- which with sorted origins is also coverage.  Then the 2-D assembly on a sample."""
    for e in range(1, 201):
        for k in range(1, 5):
            for ov in OVERLAPS:
                ov = min(ov, e)
                starts, length = TL._axis(e, k, ov)
                assert 1 <= length <= e and _axis_ok(starts, length, e, ov), (e, k, ov, starts, length)
    for h, w in ((1, 1), (1, 200), (200, 1), (97, 131), (200, 200), (7, 3)):
        for r in range(1, 5):
            for c in range(1, 5):
                for ov in OVERLAPS:
                    ov = min(ov, h, w)
                    g = TL.tile_grid(h, w, r, c, ov, True)
                    assert g.shape == (r * c + 1, 4) and g.dtype == np.int32 and g[-1].tolist() == [0, 0, h, w]
                    covered = np.zeros((h, w), bool)
                    for y0, x0, ch, cw in g[:-1]:
                        assert 0 <= y0 and 0 <= x0 and y0 + ch <= h and x0 + cw <= w and ch >= 1 and cw >= 1
                        covered[y0:y0 + ch, x0:x0 + cw] = True
                    assert covered.all()
                    grid = g[:-1].reshape(r, c, 4)      # row-major
                    assert (grid[:, :, 0] == grid[:, :1, 0]).all() and (grid[:, :, 1] == grid[:1, :, 1]).all()
                    assert _axis_ok(grid[:, 0, 0], grid[0, 0, 2], h, ov) and _axis_ok(grid[0, :, 1], grid[0, 0, 3], w, ov)
                    assert np.array_equal(TL.tile_grid(h, w, r, c, ov, False), g[:-1])


def test_library_grid_equals_the_restatement_for_every_frame_up_to_200():
    """y3_tile_grid == tiles.tile_grid for every h, w in 1..200, every grid up to 4 x 4, three overlaps (0, 7 and 64, cut to min(h, w)), with the overview tile."""
    from yolo_v3_tf2_amd import _lib
    lib = _lib.load()
    buf = (C.c_int32 * (65 * 4))()      # compared as Python lists: 480 000 grids, so no NumPy call per grid
    axes = {}
    n = 0
    for h in range(1, 201):
        for w in range(1, 201):
            for ov in (0, 7, 64):
                ov = min(ov, h, w)
                for e, k in [(h, k) for k in range(1, 5)] + [(w, k) for k in range(1, 5)]:
                    if (e, k, ov) not in axes:
                        axes[e, k, ov] = TL._axis(e, k, ov)
                for r in range(1, 5):
                    ys, lh = axes[h, r, ov]
                    for c in range(1, 5):
                        xs, lw = axes[w, c, ov]
                        T = lib.y3_tile_grid(h, w, r, c, ov, 1, buf)
                        assert T == r * c + 1
                        assert buf[:T * 4] == [v for y in ys for x in xs for v in (y, x, lh, lw)] + [0, 0, h, w], (h, w, r, c, ov)
                        n += 1
    assert n == 200 * 200 * 16 * 3
    # ... and the assembled arrays of tiles.tile_grid itself, overview on and off, on a sample
    out = np.empty((65, 4), np.int32)
    p = out.ctypes.data_as(C.POINTER(C.c_int32))
    for h, w, r, c, ov in ((1080, 1920, 2, 3, 64), (97, 131, 4, 4, 7), (1, 1, 1, 1, 0), (200, 3, 8, 3, 3), (9, 9, 8, 8, 9)):
        for overview in (0, 1):
            if r * c + overview > 64:
                continue
            T = lib.y3_tile_grid(h, w, r, c, ov, overview, p)
            assert np.array_equal(out[:T], TL.tile_grid(h, w, r, c, ov, bool(overview)))
    assert TL.tile_grid(1080, 1920, 2, 3, 64, True).tolist() == [
        [0, 0, 572, 683], [0, 618, 572, 683], [0, 1237, 572, 683], [508, 0, 572, 683], [508, 618, 572, 683], [508, 1237, 572, 683],
        [0, 0, 1080, 1920]]


REFUSED = [(0, 5, 1, 1, 0, 0), (5, 0, 1, 1, 0, 0), (5, 5, 0, 1, 0, 0), (5, 5, 1, 0, 0, 0), (50, 50, 9, 1, 0, 0), (50, 50, 1, 9, 0, 0),
           (5, 5, 1, 1, -1, 0), (5, 9, 1, 1, 6, 0), (9, 5, 2, 2, 6, 1), (50, 50, 8, 8, 0, 1), (-3, 5, 1, 1, 0, 0)]


def test_grid_refusals_are_the_same_on_both_sides():
    from yolo_v3_tf2_amd import _lib, input_stage
    lib = _lib.load()
    out = np.full((66, 4), -7, np.int32)
    for args in REFUSED:
        assert lib.y3_tile_grid(*args, out.ctypes.data_as(C.POINTER(C.c_int32))) == -1, args
        assert b"y3_tile_grid" in lib.y3_last_error()
        with pytest.raises(ValueError):
            TL.tile_grid(*args)
        with pytest.raises(_lib.Y3Error, match="y3_tile_grid"):
            input_stage.tile_grid(*args)
    assert (out == -7).all(), "a refused call writes nothing"
    assert lib.y3_tile_grid(5, 5, 1, 1, 0, 0, None) == -1
    assert lib.y3_tile_grid(50, 50, 8, 8, 0, 0, out.ctypes.data_as(C.POINTER(C.c_int32))) == 64 and (out[64:] == -7).all()
    assert lib.y3_tile_grid(5, 9, 1, 1, 5, 1, out.ctypes.data_as(C.POINTER(C.c_int32))) == 2


# ------------------------------------------------------------------------------------------------ descriptors and geometry
def test_tile_geometry_is_the_geometry_of_the_cropped_shapes():
    """y3_tile_letterbox_geometry_hw == letterbox_geometries of descriptors that name the crops as images, and == the NumPy formula."""
    from yolo_v3_tf2_amd import input_stage as I, runtime as rt
    for mode in (0, 1, 2):
        frames, windows = K.input_case(mode, True)
        _, descs = rt.pack_images(frames, mode, letterbox=True)
        tdescs = np.zeros(sum(len(w) for w in windows), I.TILE_DESC_DTYPE)
        k = 0
        for d, ws in zip(descs, windows):
            for win in ws:
                tdescs[k] = (d["offset"], d["height"], d["width"], d["channels"], d["mode"], *win)
                k += 1
        crops = K.crops(frames, windows)
        _, cdescs = rt.pack_images(crops, mode, letterbox=True)
        for canvas in K.CANVASES + [(416, 416)]:
            got = I.tile_letterbox_geometries(tdescs, canvas)
            assert np.array_equal(got, rt.letterbox_geometries(cdescs, canvas))
            assert np.array_equal(got, np.stack([letterbox_geometry(c.shape[0], c.shape[1], *canvas) for c in crops]))
        plain = tdescs.copy()
        plain["mode"] &= ~K.LETTERBOX
        assert (I.tile_letterbox_geometries(plain, (64, 96)) == [64, 96, 0, 0]).all()


def test_tile_descs_lays_out_the_grid_per_frame():
    from yolo_v3_tf2_amd import input_stage as I, runtime as rt
    frames = [K.frame(s, 1, i) for i, s in enumerate(K.FRAME_SHAPES)]
    blob, descs = rt.pack_images(frames, 1, letterbox=[True, False, True])
    tdescs, windows = I.tile_descs(frames, descs, 2, 3, 0, True)
    assert tdescs.dtype.itemsize == 40 == C.sizeof(__import__("yolo_v3_tf2_amd")._lib.TileDesc) and len(tdescs) == 21
    for i, f in enumerate(frames):
        want = TL.tile_grid(f.shape[0], f.shape[1], 2, 3, 0, True)
        assert np.array_equal(windows[i * 7:(i + 1) * 7], want)
        for t in range(7):
            d = tdescs[i * 7 + t]
            assert (d["offset"], d["height"], d["width"], d["channels"], d["mode"]) == tuple(descs[i])
            assert [d["y0"], d["x0"], d["ch"], d["cw"]] == want[t].tolist()
    with pytest.raises(rt.Y3Error, match="y3_tile_grid"):
        I.tile_descs(frames, descs, 2, 3, 2, True)       # the 1 x 1 frame cannot overlap by 2
    with pytest.raises(rt.Y3Error):
        I.tile_descs(frames[:2], descs, 2, 3, 0, True)


# ------------------------------------------------------------------------------------------------ the merge, restated
def _merge(case, per_class, T=K.T_IOU, S=K.S_LOW, **kw):
    return TL.merge_tile_detections_ref(case["packed"], case["nv"], case["windows"], case["geoms"], case["frame_hw"], case["F"], case["T"],
                                        case["canvas"], T, S, per_class=per_class, **kw)


def _brute(case, per_class, T=K.T_IOU, S=K.S_LOW):
    boxes, scores, classes = TL.tile_candidates(case["packed"], case["nv"], case["windows"], case["geoms"], case["frame_hw"], case["F"],
                                                case["T"], case["canvas"])
    sel, nv = K.brute_force_nms(boxes, scores, classes, case["M"], T, S, per_class)
    return K.rows_from(boxes, scores, classes, sel, nv, case["M"]), nv


@pytest.mark.parametrize("per_class", [False, True])
@pytest.mark.parametrize("shape", [(2, 7, 12), (1, 1, 9), (3, 5, 1), (1, 4, 30)])
def test_merge_restatement_equals_a_brute_force_loop(shape, per_class):
    """Duplicated objects in two and more tiles, equal scores, an empty tile, an over-range and a negative count, poisoned rows."""
    F, T, M = shape
    case = K.merge_case(F, T, M, seed=11 + T)
    got, want = _merge(case, per_class), _brute(case, per_class)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    assert not (got[0] == 0x7F7F7F7F).any(), "a row behind num_valid was read"
    if T > 1:
        cand_total = np.clip(case["nv"], 0, M).reshape(F, T).sum(1)
        assert (got[1][got[1] < M] < cand_total[got[1] < M]).all(), "where the cap does not bind the merge dropped duplicates"
        assert (case["nv"].reshape(F, T)[:, 1] == 0).all()
    for f in range(F):      # the index word names tile and row; the row is that tile's row, mapped
        for row in got[0][f, :got[1][f]]:
            t, r = divmod(int(row[6]), M)
            src = case["packed"][f * T + t, r]
            assert r < min(max(case["nv"][f * T + t], 0), M) and row[4] == src[4] and row[5] == src[5]


def test_the_two_rules_part_where_classes_differ():
    case = K.merge_case(2, 7, 40, seed=5)
    a, p = _merge(case, False), _merge(case, True)
    assert (p[1] >= a[1]).all() and (p[1] > a[1]).any()
    # agnostic through the per-class restatement with equal ids == the same through an agnostic rule handed in (here: the brute force)
    brute = lambda b, s, M, T, S: K.brute_force_nms(b, s, np.zeros(s.shape, np.int64), M, T, S, False)
    b = _merge(case, False, agnostic_nms=brute)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_agnostic_restatement_equals_the_c_oracle():
    """The agnostic rule the restatement uses by default (per-class rule, all ids equal) against oracle's tiled NMS on merge candidates."""
    from oracle import oracle as O
    case = K.merge_case(2, 7, 40, seed=8)
    boxes, scores, _ = TL.tile_candidates(case["packed"], case["nv"], case["windows"], case["geoms"], case["frame_hw"], 2, 7, case["canvas"])
    for T, S in ((0.5, 0.05), (0.3, 0.4), (0.9, -1.0)):
        want = O.nms_padded(boxes, scores, 40, T, S)
        got = TL.nms_padded_agnostic_ref(boxes, scores, 40, T, S)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_exact_duplicates_and_equal_scores_keep_the_lower_index():
    case = K.identity_case(M=30)
    merged, nv = _merge(case, False)
    n0 = case["nv"][0]
    assert n0 > 2 and case["nv"][2] == n0
    idx = merged[0, :nv[0], 6]
    assert not ((idx >= 2 * 30) & (idx < 3 * 30)).any(), "tile 2 repeats tile 0 word for word: every one of its rows is suppressed by its twin"
    got, want = _merge(case, True), _brute(case, True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # identity geometry and whole-axis windows: the boxes are copied bit for bit
    for row in merged[0, :nv[0]]:
        t, r = divmod(int(row[6]), 30)
        assert np.array_equal(row[:6], case["packed"][t, r, :6])


def test_empty_tiles_and_empty_frames():
    case = K.empty_case(3, 7, 10)
    for per_class in (False, True):
        merged, nv = _merge(case, per_class)
        assert not nv.any() and not merged.any()
    case = K.merge_case(2, 7, 10, seed=2)
    case["nv"][7:] = 0      # frame 1 empty, frame 0 not
    merged, nv = _merge(case, False)
    assert nv[0] > 0 and nv[1] == 0 and not merged[1].any()


@pytest.mark.parametrize("geom", [(64, 64, 0, 0), (40, 50, 12, 7), (64, 32, 0, 16), (30, 64, 17, 0)])
def test_one_whole_frame_tile_is_the_unletterboxed_input(geom):
    """T = 1, the window the whole frame: the merged rows are the input rows un-letterboxed (core.utils.unletterbox_boxes, the
    restatement of y3_unletterbox_detections_hw), apart from the index word.  Well-separated boxes, so that nothing is suppressed.
    The canvas is 64 x 64: on an axis that fills it the merge copies where unletterbox computes x * 64 / 64 -- the same value, the
    side being a power of two (include/y3.h says where the two differ)."""
    rng = np.random.default_rng(3)
    M, n = 16, 9
    packed = np.zeros((1, M, 7), np.int32)
    c = np.stack(np.meshgrid([0.2, 0.5, 0.8], [0.2, 0.5, 0.8]), -1).reshape(9, 2) + rng.uniform(-0.02, 0.02, (9, 2))
    boxes = np.concatenate([c - 0.1, c + 0.1], 1).astype(np.float32)
    scores = np.sort(rng.uniform(0.1, 0.9, n).astype(np.float32))[::-1]
    packed[0, :n, :4], packed[0, :n, 4], packed[0, :n, 5], packed[0, :n, 6] = boxes.view(np.int32), scores.view(np.int32), np.arange(n) % 3, 77
    for hw in ((97, 131), (1, 1)):
        merged, nv = TL.merge_tile_detections_ref(packed, [n], [[0, 0, *hw]], [geom], [hw], 1, 1, 64, 0.5, 0.05)
        assert nv.tolist() == [n] and merged[0, :n, 6].tolist() == list(range(n))
        assert np.array_equal(merged[0, :n, :4].view(np.float32), unletterbox_boxes(boxes, geom, 64))
        assert np.array_equal(merged[0, :, 4:6], packed[0, :, 4:6]) and not merged[0, n:].any()


# ------------------------------------------------------------------------------------------------ one pass, two stages
def test_one_pass_property_over_the_two_stages():
    """Raw per-tile candidates -> per-tile NMS at threshold t -> merge at t.  For every t of a sweep the result equals the rows with
    score > t of the result at the lowest threshold: per-tile rows are a prefix in score order (the cap M keeps a prefix), the merge is
    greedy in score order, and no box is affected by a box scored below it.  Both rules; M small enough that both caps bind."""
    rng = np.random.default_rng(21)
    F, T, M, N, canvas = 2, 5, 12, 60, (64, 96)
    frame_hw = np.array([[97, 131], [64, 48]], np.int32)
    windows = np.concatenate([K._hand_grid(h, w, T) for h, w in frame_hw])
    geoms = K.window_geoms(windows, canvas, True)
    c = rng.uniform(0.1, 0.9, (F * T, N, 2))
    s = rng.uniform(0.05, 0.5, (F * T, N, 2))
    raw = np.clip(np.concatenate([c - s / 2, c + s / 2], 2), 0, 1).astype(np.float32)
    scores = rng.uniform(0.0, 1.0, (F * T, N)).astype(np.float32)
    scores[:, ::7] = scores[:, 1:2]                 # ties
    classes = rng.integers(0, 3, (F * T, N))
    thresholds = [0.05, 0.2, 0.200001, 0.5, 0.8, 0.97, 1.0]
    for per_class in (False, True):
        results = []
        for t in thresholds:
            if per_class:
                sel, nv = nms_padded_per_class_ref(raw, scores, classes, M, 0.5, t)
            else:
                sel, nv = TL.nms_padded_agnostic_ref(raw, scores, M, 0.5, t)
            rows = K.rows_from(raw, scores, classes, sel, nv, M)
            results.append(TL.merge_tile_detections_ref(rows, nv, windows, geoms, frame_hw, F, T, canvas, 0.45, t, per_class=per_class))
        low = results[0]
        assert (low[1] == M).any() and low[1].min() > 0
        for t, got in zip(thresholds, results):
            want = TL.merged_rows_above(*low, t)
            assert np.array_equal(got[1], want[1]), t
            assert np.array_equal(got[0], want[0]), t
        assert not results[-1][1].any()


# ------------------------------------------------------------------------------------------------ argument checks, no device
def _lib_and_tile():
    from yolo_v3_tf2_amd import _lib, input_stage as I
    d = np.zeros(3, I.TILE_DESC_DTYPE)
    d[:] = (0, 10, 12, 3, 1 | K.LETTERBOX, 2, 3, 4, 5)
    return _lib, _lib.load(), d


def test_tile_geometry_and_preprocess_checks_name_the_tile():
    _lib, lib, d = _lib_and_tile()
    out = np.full((3, 4), -7, np.int32)
    optr, dptr = out.ctypes.data_as(C.POINTER(C.c_int32)), lambda a: a.ctypes.data_as(C.POINTER(_lib.TileDesc))
    bad = [("y0", -1, b"window"), ("x0", 8, b"window"), ("y0", 7, b"window"), ("ch", 0, b"ch and cw"), ("cw", 0, b"ch and cw"),
           ("cw", 13, b"window"), ("ch", 2**31 - 1, b"window"), ("height", 0, b"height and width"), ("mode", 3, b"mode"), ("mode", 0x200, b"mode")]
    for field, value, word in bad:
        e = d.copy()
        e[field][1] = value
        assert lib.y3_tile_letterbox_geometry_hw(dptr(e), 3, 64, 64, optr) == _lib.Y3_ERR_INVALID, (field, value)
        msg = lib.y3_last_error()
        assert b"y3_tile_letterbox_geometry_hw: tile 1" in msg and word in msg, msg
        # the preprocess call refuses the same before it looks for a device: the pointers are never followed
        assert lib.y3_preprocess_tiles_hw(C.c_void_p(4096), 10 * 12 * 3, dptr(e), 3, C.c_void_p(4096), 0, 64, 64, None) == _lib.Y3_ERR_INVALID
        msg = lib.y3_last_error()
        assert b"y3_preprocess_tiles_hw: tile 1" in msg and word in msg, msg
    assert (out == -7).all()
    for kw in (dict(n=0), dict(Hc=0), dict(Wc=-1), dict(descs=None), dict(out=None)):
        a = dict(dict(descs=dptr(d), n=3, Hc=64, Wc=64, out=optr), **kw)
        assert lib.y3_tile_letterbox_geometry_hw(a["descs"], a["n"], a["Hc"], a["Wc"], a["out"]) == _lib.Y3_ERR_INVALID
    # y3_preprocess_tiles_hw only: channels, the blob's size, float alignment, the plain arguments
    only = [("channels", 2, 360, b"channels"), ("channels", 5, 360, b"channels"), ("offset", 1, 360, b"runs past"), ("height", 11, 360, b"runs past")]
    for field, value, nbytes, word in only:
        e = d.copy()
        e[field][2] = value
        assert lib.y3_preprocess_tiles_hw(C.c_void_p(4096), nbytes, dptr(e), 3, C.c_void_p(4096), 0, 64, 64, None) == _lib.Y3_ERR_INVALID
        msg = lib.y3_last_error()
        assert b"y3_preprocess_tiles_hw: tile 2" in msg and word in msg, msg
    f = d.copy()
    f["mode"] = 0
    f["offset"][0] = 2
    assert lib.y3_preprocess_tiles_hw(C.c_void_p(4096), 10 * 12 * 12 + 2, dptr(f), 3, C.c_void_p(4096), 0, 64, 64, None) == _lib.Y3_ERR_INVALID
    assert b"tile 0: float32 pixels must be 4-byte aligned" in lib.y3_last_error()
    for kw in (dict(pix=None), dict(descs=None), dict(batch=None), dict(n=0), dict(slot=-1), dict(Hc=0), dict(Wc=0)):
        a = dict(dict(pix=C.c_void_p(4096), descs=dptr(d), batch=C.c_void_p(4096), n=3, slot=0, Hc=64, Wc=64), **kw)
        assert lib.y3_preprocess_tiles_hw(a["pix"], 360, a["descs"], a["n"], a["batch"], a["slot"], a["Hc"], a["Wc"], None) == _lib.Y3_ERR_INVALID
        assert b"y3_preprocess_tiles_hw: bad argument" in lib.y3_last_error()


def test_merge_checks_that_need_no_device():
    from yolo_v3_tf2_amd import _lib
    lib = _lib.load()
    case = K.merge_case(2, 3, 4, seed=1, canvas=(64, 64))
    i32 = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    need = lib.y3_merge_tiles_workspace_bytes(2, 3, 4)
    N = 3 * 4
    parts = [2 * N * 16, 2 * N * 8, 2 * N * 4, 2 * 4 * 4]
    assert need == sum(-(-p // 16) * 16 for p in parts) + lib.y3_nms_per_class_workspace_bytes(2, N)
    for args in ((0, 3, 4), (2, 0, 4), (2, 65, 4), (2, 3, 0), (2, 3, 1025), (2**20, 64, 1024)):
        assert lib.y3_merge_tiles_workspace_bytes(*args) == 0, args
    assert lib.y3_merge_tiles_workspace_bytes(1, 64, 1024) > 0
    dev = C.c_void_p(4096)      # never followed: every call below is refused on the host
    good = dict(packed=dev, nv=dev, windows=case["windows"], geoms=case["geoms"], hw=case["frame_hw"], F=2, T=3, M=4, Hc=64, Wc=64, mode=0,
                iou=0.5, score=0.05, out=dev, nv_out=dev, ws=dev, bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        tab = lambda v: None if v is None else i32(v)
        return lib.y3_merge_tile_detections(a["packed"], a["nv"], tab(a["windows"]), tab(a["geoms"]), tab(a["hw"]), a["F"], a["T"], a["M"],
                                            a["Hc"], a["Wc"], a["mode"], a["iou"], a["score"], a["out"], a["nv_out"], a["ws"], a["bytes"], None)

    def edited(name, row, col, value):
        t = np.array(case[name], np.int32)
        t[row, col] = value
        return t

    bad = [(dict([(k, None)]), b"null pointer") for k in ("packed", "nv", "windows", "geoms", "hw", "out", "nv_out")]
    bad += [(dict(F=0), b"frames must be at least 1"), (dict(T=0), b"tiles must be in [1,64]"), (dict(T=65), b"tiles must be in [1,64]"),
            (dict(M=0), b"max_boxes must be in [1,1024]"), (dict(M=1025), b"max_boxes must be in [1,1024]"),
            (dict(Hc=0), b"canvas"), (dict(Wc=0), b"canvas"), (dict(mode=2), b"nms_mode"), (dict(mode=-1), b"nms_mode"),
            (dict(mode=1, iou=0.0), b"iou_threshold must be > 0"), (dict(mode=1, iou=float("nan")), b"iou_threshold must be > 0"),
            (dict(iou=0.0, score=-1.0), b"not supported"),
            (dict(hw=edited("frame_hw", 1, 0, 0)), b"frame 1: height and width"),
            (dict(windows=edited("windows", 4, 0, -1)), b"frame 1, tile 1: window"),
            (dict(windows=edited("windows", 5, 3, 0)), b"frame 1, tile 2: window"),
            (dict(windows=edited("windows", 0, 2, 98)), b"frame 0, tile 0: window"),
            (dict(windows=edited("windows", 2, 1, 1)), b"frame 0, tile 2: window"),
            (dict(geoms=edited("geoms", 3, 0, 0)), b"frame 1, tile 0: geometry"),
            (dict(geoms=edited("geoms", 1, 2, 63)), b"frame 0, tile 1: geometry"),
            (dict(geoms=edited("geoms", 1, 3, -1)), b"frame 0, tile 1: geometry"),
            (dict(ws=None), b"workspace too small"), (dict(bytes=need - 1), b"workspace too small"),
            (dict(ws=C.c_void_p(4104)), b"aligned"), (dict(packed=C.c_void_p(4098)), b"aligned"), (dict(out=C.c_void_p(4097)), b"aligned")]
    for kw, word in bad:
        assert call(**kw) == _lib.Y3_ERR_INVALID, kw
        msg = lib.y3_last_error()
        assert b"y3_merge_tile_detections" in msg and word in msg, (kw, msg)


# ------------------------------------------------------------------------------------------------ model switch, YAML keys, command line
def test_set_tiles_yaml_keys_and_command_line(program):
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev
    from yolo_v3_tf2_amd.core.parse_model import YoloModel
    from yolo_v3_tf2_amd.inference import Inference
    model = YoloModel(program)
    assert model.tiles is None
    model.set_tiles(2, 3, 64, True)
    assert model.tiles == (2, 3, 64, True) and model._net is None
    model.set_tiles(1, 1)
    assert model.tiles == (1, 1, 0, False)
    for bad in ((0, 3), (2, 9), (2, 3, -1), (8, 8, 0, True)):
        with pytest.raises(ValueError):
            model.set_tiles(*bad)
    assert model.tiles == (1, 1, 0, False)
    model.set_tiles(None)
    assert model.tiles is None
    cfg = {"tiles": [2, 3], "tile_overlap": 64, "tile_overview": True, "image_size": 416}
    assert Inference.tiles_from_config(cfg) == (2, 3, 64, True) and "tiles" in cfg
    assert Inference.tiles_from_config(cfg, pop=True) == (2, 3, 64, True) and cfg == {"image_size": 416}
    assert Inference.tiles_from_config({"tiles": [1, 2]}) == (1, 2, 0, False) and Inference.tiles_from_config({}) is None
    for bad in ({"tile_overlap": 3}, {"tile_overview": True}, {"tiles": [2]}, {"tiles": [1, 2, 3]}):
        with pytest.raises(ValueError):
            Inference.tiles_from_config(bad)
    a = ev._arg_parser().parse_args(["--on-device", "--ap", "--tiles", "2", "3", "--tile-overlap", "64", "--tile-overview"])
    assert a.tiles == [2, 3] and a.tile_overlap == 64 and a.tile_overview is True
    a = ev._arg_parser().parse_args([])
    assert a.tiles is None and a.tile_overlap == 0 and a.tile_overview is False
    for argv in (["--tiles", "2", "3"], ["--on-device", "--tile-overlap", "4"], ["--on-device", "--loss", "--tiles", "2", "2"]):
        with pytest.raises(SystemExit):
            ev.main(argv)
    with pytest.raises(ValueError, match="on_device"):
        ev.evaluate({"anchors_file": "-", "classes_name_file": "-"}, [0.1], tiles=(2, 2, 0, False))
    with pytest.raises(ValueError, match="on_device"):
        ev.evaluate({"anchors_file": "-", "classes_name_file": "-", "tiles": [2, 2]}, [0.1])
