"""Rectangular network input, host side (no GPU): the letterbox geometry of an H x W canvas (y3_letterbox_geometry_hw) against
its NumPy restatement and against the square entry point, runtime.rect_canvas / rect_anchors, the NumPy decode restatement
(core/yolo_decode_layer.yolo_decode_hw_host) against the oracle, and the argument checks of the new entry points."""
import ctypes as C

import numpy as np
import pytest

CANVASES = [(64, 96), (96, 64), (320, 416), (256, 416)]


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    return runtime


@pytest.fixture(scope="module")
def lib():
    from yolo_v3_tf2_amd import _lib
    return _lib.load()


def _descs(rt, hs, ws, flag=True):
    from yolo_v3_tf2_amd import _lib
    d = np.zeros(len(hs), rt.IMAGE_DESC_DTYPE)
    d["height"], d["width"], d["channels"], d["mode"] = hs, ws, 3, 1 | (_lib.Y3_IMAGE_LETTERBOX if flag else 0)
    return d


def _all_sizes():
    h, w = np.meshgrid(np.arange(1, 201), np.arange(1, 201), indexing="ij")
    return h.reshape(-1), w.reshape(-1)


@pytest.mark.parametrize("canvas", CANVASES)
def test_letterbox_geometry_hw_equals_the_numpy_restatement(rt, canvas):
    """Every h, w in 1..200 onto the canvas: the library's fp32 geometry == core/utils.letterbox_geometry, all four numbers."""
    from yolo_v3_tf2_amd.core.utils import letterbox_geometry
    h, w = _all_sizes()
    got = rt.letterbox_geometries(_descs(rt, h, w), canvas)
    assert got.dtype == np.int32 and np.array_equal(got, letterbox_geometry(h, w, *canvas))
    # without the flag: the whole canvas (the image is stretched to Hc x Wc)
    plain = rt.letterbox_geometries(_descs(rt, h[:50], w[:50], flag=False), canvas)
    assert np.array_equal(plain, np.tile(np.array([canvas[0], canvas[1], 0, 0], np.int32), (50, 1)))


@pytest.mark.parametrize("S", [64, 96, 416])
def test_square_canvas_is_the_square_entry_point(rt, lib, S):
    """Hc == Wc: y3_letterbox_geometry_hw == y3_letterbox_geometry over the same 1..200 range (one code path)."""
    from yolo_v3_tf2_amd import _lib
    h, w = _all_sizes()
    d = np.ascontiguousarray(_descs(rt, h, w))
    old = np.empty((len(d), 4), np.int32)
    _lib.check(lib.y3_letterbox_geometry(d.ctypes.data_as(C.POINTER(_lib.ImageDesc)), len(d), S, old.ctypes.data_as(C.POINTER(C.c_int32))))
    assert np.array_equal(rt.letterbox_geometries(d, (S, S)), old) and np.array_equal(rt.letterbox_geometries(d, S), old)


def test_rect_canvas_known_answers_and_fit(rt):
    """The issue's frames, their transposes, a square frame; then for every h, w in 1..200 with the long side brought to 96:
    both sides are multiples of the stride, the frame's own letterbox geometry fits the canvas, and no side could be one
    stride shorter (the smallest such canvas)."""
    from yolo_v3_tf2_amd.core.utils import letterbox_geometry
    assert rt.rect_canvas(480, 640, 416) == (320, 416)
    assert rt.rect_canvas(1080, 1920, 416) == (256, 416)
    assert rt.rect_canvas(640, 480, 416) == (416, 320)
    assert rt.rect_canvas(1920, 1080, 416) == (416, 256)
    assert rt.rect_canvas(500, 500, 416) == (416, 416)
    assert rt.rect_canvas(480, 640, 416, stride=64) == (320, 448)
    h, w = _all_sizes()
    for hh, ww in zip(h.tolist(), w.tolist()):
        H, W = rt.rect_canvas(hh, ww, 96)
        assert H % 32 == 0 and W % 32 == 0 and 32 <= H <= 96 and 32 <= W <= 96 and max(H, W) == 96
        sh, sw, top, left = (int(v) for v in letterbox_geometry(hh, ww, H, W))
        assert 1 <= sh and 1 <= sw and top >= 0 and left >= 0 and top + sh <= H and left + sw <= W, (hh, ww, H, W)
        full = letterbox_geometry(hh, ww, 96, 96)
        assert H - 32 < int(full[0]) and W - 32 < int(full[1]), (hh, ww, H, W)     # a stride less would not hold the resize


def test_rect_anchors(rt, anchors):
    """aw * S / W and ah * S / H in fp32; an axis whose side equals S is copied, never computed (x * S / S is not x in fp32:
    0.1 * 49 / 49 is one such value), so the long side of a rect_canvas and the square canvas give the file's values back."""
    a = rt.rect_anchors(anchors, 416, (320, 416))
    assert a.dtype == np.float32 and a.shape == (3, 3, 2)
    assert np.array_equal(a[..., 0], anchors[..., 0])
    assert np.array_equal(a[..., 1], anchors[..., 1] * np.float32(416) / np.float32(320))
    assert np.allclose(a[..., 1] * 320, anchors[..., 1] * 416, rtol=1e-6)          # the same pixels
    t = rt.rect_anchors(anchors, 416, (416, 256))
    assert np.array_equal(t[..., 1], anchors[..., 1]) and np.array_equal(t[..., 0], anchors[..., 0] * np.float32(416) / np.float32(256))
    # values for which the computed form would move: the copy keeps them
    x = np.float32(np.arange(1, 2001)) / np.float32(2001)
    assert (x * np.float32(49) / np.float32(49) != x).any()
    probe = np.stack([x, x], -1)
    assert np.array_equal(rt.rect_anchors(probe, 49, (49, 49)), probe) and np.array_equal(rt.rect_anchors(probe, 49, 49), probe)
    assert np.array_equal(rt.rect_anchors(probe, 49, (32, 49))[..., 0], x)


def test_inference_config_takes_an_h_w_pair(anchors):
    """inference.py's `image_size: [H, W]`: the canvas is the pair, and the anchors file -- normalised by the long side of the
    canvas, by convention -- is rescaled on the short axis only; an int and a square pair leave it as it is."""
    from yolo_v3_tf2_amd.inference import Inference
    hw, a = Inference.canvas_and_anchors([320, 416], anchors)
    assert hw == (320, 416) and a.dtype == np.float32
    assert np.array_equal(a[..., 0], anchors[..., 0]) and np.array_equal(a[..., 1], anchors[..., 1] * np.float32(416) / np.float32(320))
    hw, a = Inference.canvas_and_anchors([416, 256], anchors)
    assert hw == (416, 256)
    assert np.array_equal(a[..., 1], anchors[..., 1]) and np.array_equal(a[..., 0], anchors[..., 0] * np.float32(416) / np.float32(256))
    for size in (416, [416, 416]):
        hw, a = Inference.canvas_and_anchors(size, anchors)
        assert hw == (416, 416) and np.array_equal(a, anchors)
    with pytest.raises(Exception):
        Inference.canvas_and_anchors([416, 320, 3], anchors)


def test_grid_sizes_take_a_pair(program):
    assert program.grid_sizes(96) == [3, 6, 12]
    assert program.grid_sizes((64, 96)) == [(2, 3), (4, 6), (8, 12)]
    assert program.grid_sizes((96, 96)) == [(3, 3), (6, 6), (12, 12)]
    assert program.flops_per_image((416, 416)) == program.flops_per_image(416)
    assert abs(program.flops_per_image((320, 416)) / program.flops_per_image(416) - 320 / 416) < 1e-12


# Two host libm paths: NumPy's float32 exp (documented maximum error 2.52 ulp) and the C library's expf behind the oracle
# (< 1 ulp), so exp(t) differs by at most ~3.6 ulp.  A width w = exp(t) * anchor carries that as 3.6 ulp of w, and the scale the
# bound is relative to is the largest |corner| ~ w / 2: 3.6 x 2 x 2^-24 = 4.3e-7, plus the roundings of the product, the halving
# and the add (~3 ulp of the corner, 1.8e-7): 6.1e-7; conf and probs (sigmoid' <= 1/4) stay far below that.  Bound 8e-7 x scale,
# 2.5 times tighter than the 2e-6 x scale of tests/test_gpu_parity.py::test_decode_matches_oracle.  Observed on the machine this
# was written on: 1.7e-7 x scale for the boxes, 1.2e-7 for conf and probs.
HOST_BOUND = 8e-7


def _random_grids(gs, B, nc, seed):
    rng = np.random.default_rng(seed)
    return [rng.normal(0, 1.5, (B, gh, gw, 3, 5 + nc)).astype(np.float32) for gh, gw in gs]


@pytest.mark.parametrize("gs,B,nc", [((2, 4, 8), 3, 7), ((3, 6, 12), 2, 80), ((13, 26, 52), 1, 80)])
def test_host_decode_equals_the_oracle_on_square_grids(anchors, gs, B, nc):
    from oracle import oracle as O
    from yolo_v3_tf2_amd.core.yolo_decode_layer import yolo_decode_hw_host
    grids = _random_grids([(g, g) for g in gs], B, nc, 11)
    rb, rc, rp = O.yolo_decode(grids, anchors, nc)
    hb, hc, hp = yolo_decode_hw_host(grids, anchors, nc)
    assert hb.shape == rb.shape and hc.shape == rc.shape and hp.shape == rp.shape
    assert hb.dtype == hc.dtype == hp.dtype == np.float32
    scale = max(1.0, float(np.abs(rb).max()))
    print("square", gs, float(np.abs(hb - rb).max()) / scale, float(np.abs(hc - rc).max()), float(np.abs(hp - rp).max()))
    assert np.abs(hb - rb).max() <= HOST_BOUND * scale
    assert np.abs(hc - rc).max() <= HOST_BOUND and np.abs(hp - rp).max() <= HOST_BOUND


@pytest.mark.parametrize("gs", [((2, 3), (4, 6), (8, 12)), ((3, 2), (6, 4), (12, 8))])
def test_host_decode_against_the_oracle_on_rectangular_grids(anchors, gs):
    """The oracle divides x by gh and y by gw (the reference's cast(shape[1:3])); the restatement divides each axis by its own
    extent.  Widths, heights, conf and probs do not see the divisor and agree to the host bound; the centres satisfy
    cx * gw == cx_oracle * gh and cy * gh == cy_oracle * gw: both sides are sigmoid + col (sigmoid + row) up to the two
    divisions' and the multiplications' roundings and the min / max / mid-point arithmetic -- 8 ulp of the product (< grid
    side) is the bound.  This ties the restatement's row order and meshgrid to the oracle's without touching oracle/."""
    from oracle import oracle as O
    from yolo_v3_tf2_amd.core.yolo_decode_layer import yolo_decode_hw_host
    B, nc = 3, 7
    grids = _random_grids(gs, B, nc, 12)
    rb, rc, rp = O.yolo_decode(grids, anchors, nc)
    hb, hc, hp = yolo_decode_hw_host(grids, anchors, nc)
    N = 3 * sum(gh * gw for gh, gw in gs)
    assert hb.shape == rb.shape == (B, N, 4) and hc.shape == (B, N, 1) and hp.shape == (B, N, nc)
    assert np.abs(hc - rc).max() <= HOST_BOUND and np.abs(hp - rp).max() <= HOST_BOUND
    off = 0
    for gh, gw in gs:
        n = 3 * gh * gw
        h_, r_ = hb[:, off:off + n].astype(np.float64), rb[:, off:off + n].astype(np.float64)
        off += n
        scale = max(1.0, float(np.abs(r_).max()))
        # widths and heights: differences of the two corners; the centre's magnitude sets the rounding of the corners
        assert np.abs((h_[..., 2] - h_[..., 0]) - (r_[..., 2] - r_[..., 0])).max() <= 4 * HOST_BOUND * scale
        assert np.abs((h_[..., 3] - h_[..., 1]) - (r_[..., 3] - r_[..., 1])).max() <= 4 * HOST_BOUND * scale
        cx, cy = (h_[..., 0] + h_[..., 2]) / 2, (h_[..., 1] + h_[..., 3]) / 2
        ox, oy = (r_[..., 0] + r_[..., 2]) / 2, (r_[..., 1] + r_[..., 3]) / 2
        ulp = 8 * np.finfo(np.float32).eps * max(gh, gw) * scale
        assert np.abs(cx * gw - ox * gh).max() <= ulp and np.abs(cy * gh - oy * gw).max() <= ulp
        # and the centres are normalised: cell (row, col) lies in [col / gw, (col + 1) / gw] x [row / gh, (row + 1) / gh]
        col = np.tile(np.repeat(np.arange(gw), 3), gh)[None]
        row = np.repeat(np.arange(gh), 3 * gw)[None]
        assert (cx * gw >= col - 1e-5).all() and (cx * gw <= col + 1 + 1e-5).all()
        assert (cy * gh >= row - 1e-5).all() and (cy * gh <= row + 1 + 1e-5).all()


def test_unletterbox_boxes_takes_the_canvas_pair():
    from yolo_v3_tf2_amd.core.utils import unletterbox_boxes
    boxes = np.random.default_rng(3).random((5, 4), dtype=np.float32)
    g = (64, 85, 0, 5)
    want = np.stack([(boxes[:, 0] * np.float32(96) - np.float32(5)) / np.float32(85), (boxes[:, 1] * np.float32(64) - np.float32(0)) / np.float32(64),
                     (boxes[:, 2] * np.float32(96) - np.float32(5)) / np.float32(85), (boxes[:, 3] * np.float32(64) - np.float32(0)) / np.float32(64)], 1)
    assert np.array_equal(unletterbox_boxes(boxes, g, (64, 96)), want)
    assert np.array_equal(unletterbox_boxes(boxes, (64, 96, 0, 0), (64, 96)), boxes)          # the whole canvas: untouched
    assert np.array_equal(unletterbox_boxes(boxes, (32, 64, 16, 0), 64), unletterbox_boxes(boxes, (32, 64, 16, 0), (64, 64)))


# ------------------------------------------------------------------------------------------------------------ argument checks
def _err(lib):
    return lib.y3_last_error().decode()


def test_plan_hw_refuses_sides_that_are_no_multiple_of_32(lib, program):
    """Only the argument check that precedes everything ("bad argument": null net, a side <= 0) can be reached without a GPU:
    y3_net_create needs a device, so no host test holds a net.  The divisibility refusal and its message (sides that are no
    multiple of 32) are therefore NOT read here; tests/test_rect_gpu.py::test_plan_hw_refuses_bad_sides_by_name reads them."""
    from yolo_v3_tf2_amd import _lib
    assert lib.y3_net_plan_hw(None, 1, 64, 96, 0) == _lib.Y3_ERR_INVALID and "y3_net_plan" in _err(lib)
    assert lib.y3_net_plan_hw(None, 1, 0, 96, 0) == _lib.Y3_ERR_INVALID


def test_new_image_calls_refuse_null_pointers_and_zero_sizes(rt, lib):
    from yolo_v3_tf2_amd import _lib
    INV = _lib.Y3_ERR_INVALID
    d = np.ascontiguousarray(_descs(rt, [10, 20], [30, 40]))
    dp = d.ctypes.data_as(C.POINTER(_lib.ImageDesc))
    geoms = np.empty((2, 4), np.int32)
    gp = geoms.ctypes.data_as(C.POINTER(C.c_int32))
    fake = C.c_void_p(4096)      # never dereferenced: every check precedes the first launch
    assert lib.y3_letterbox_geometry_hw(None, 2, 64, 96, gp) == INV
    assert lib.y3_letterbox_geometry_hw(dp, 2, 64, 96, None) == INV
    assert lib.y3_letterbox_geometry_hw(dp, 0, 64, 96, gp) == INV
    assert lib.y3_letterbox_geometry_hw(dp, 2, 0, 96, gp) == INV and lib.y3_letterbox_geometry_hw(dp, 2, 64, 0, gp) == INV
    bad = d.copy()
    bad["height"][1] = 0
    assert lib.y3_letterbox_geometry_hw(bad.ctypes.data_as(C.POINTER(_lib.ImageDesc)), 2, 64, 96, gp) == INV
    assert "image 1" in _err(lib) and "y3_letterbox_geometry_hw" in _err(lib)
    # preprocess_image_hw
    assert lib.y3_preprocess_image_hw(None, 1, 10, 10, 3, fake, 0, 64, 96, None) == INV
    assert lib.y3_preprocess_image_hw(fake, 1, 10, 10, 3, None, 0, 64, 96, None) == INV
    assert lib.y3_preprocess_image_hw(fake, 1, 0, 10, 3, fake, 0, 64, 96, None) == INV
    assert lib.y3_preprocess_image_hw(fake, 1, 10, 10, 3, fake, 0, 0, 96, None) == INV
    assert lib.y3_preprocess_image_hw(fake, 1, 10, 10, 3, fake, 0, 64, 0, None) == INV
    assert lib.y3_preprocess_image_hw(fake, 1, 10, 10, 5, fake, 0, 64, 96, None) == INV and "y3_preprocess_image_hw" in _err(lib)
    # preprocess_batch_hw
    assert lib.y3_preprocess_batch_hw(None, 4096, dp, 2, fake, 0, 64, 96, None) == INV
    assert lib.y3_preprocess_batch_hw(fake, 4096, None, 2, fake, 0, 64, 96, None) == INV
    assert lib.y3_preprocess_batch_hw(fake, 4096, dp, 2, None, 0, 64, 96, None) == INV
    assert lib.y3_preprocess_batch_hw(fake, 4096, dp, 0, fake, 0, 64, 96, None) == INV
    assert lib.y3_preprocess_batch_hw(fake, 4096, dp, 2, fake, 0, 0, 96, None) == INV
    assert lib.y3_preprocess_batch_hw(fake, 4096, dp, 2, fake, 0, 64, 0, None) == INV
    d2 = d.copy()
    d2["offset"] = [0, 4000]     # image 1 (20 x 40 x 3 = 2400 bytes) runs past the 4096-byte blob
    assert lib.y3_preprocess_batch_hw(fake, 4096, d2.ctypes.data_as(C.POINTER(_lib.ImageDesc)), 2, fake, 0, 64, 96, None) == INV
    assert "image 1" in _err(lib) and "y3_preprocess_batch_hw" in _err(lib)
    # unletterbox_detections_hw
    geoms[:] = [[64, 85, 0, 5], [36, 96, 14, 0]]
    assert lib.y3_unletterbox_detections_hw(None, fake, gp, 2, 10, 64, 96, None) == INV
    assert lib.y3_unletterbox_detections_hw(fake, None, gp, 2, 10, 64, 96, None) == INV
    assert lib.y3_unletterbox_detections_hw(fake, fake, None, 2, 10, 64, 96, None) == INV
    assert lib.y3_unletterbox_detections_hw(fake, fake, gp, 0, 10, 64, 96, None) == INV
    assert lib.y3_unletterbox_detections_hw(fake, fake, gp, 2, 10, 0, 96, None) == INV
    assert lib.y3_unletterbox_detections_hw(fake, fake, gp, 2, 10, 64, 0, None) == INV
    assert lib.y3_unletterbox_detections_hw(fake, fake, gp, 2, 0, 64, 96, None) == INV
    # the (96, 64) canvas cannot hold the second geometry (36 x 96 at (14, 0)): refused by name, nothing enqueued
    assert lib.y3_unletterbox_detections_hw(fake, fake, gp, 2, 10, 96, 64, None) == INV and "image 0" in _err(lib)
    # decode_hw: null grids / outputs, an empty side
    hw = (C.c_int32 * 6)(2, 3, 4, 6, 8, 12)
    a = np.zeros(18, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    ptrs = (C.c_void_p * 3)(4096, 4096, 4096)
    assert lib.y3_yolo_decode_hw(ptrs, hw, 1, 7, a, fake, None, fake, None) == INV
    assert lib.y3_yolo_decode_scores_hw(ptrs, hw, 1, 7, a, fake, fake, None, None) == INV
    assert lib.y3_yolo_decode_hw(ptrs, (C.c_int32 * 6)(2, 0, 4, 6, 8, 12), 1, 7, a, fake, fake, fake, None) == INV
    assert lib.y3_yolo_decode_hw((C.c_void_p * 3)(4096, None, 4096), hw, 1, 7, a, fake, fake, fake, None) == INV
