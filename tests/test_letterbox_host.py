"""Letterboxed input, host tier (no GPU): the ABI of y3_letterbox_geometry / y3_unletterbox_detections / Y3_IMAGE_LETTERBOX, the
fp32 geometry against its NumPy definition and against where resize_image puts the pixels, the argument checks of the new and
the extended calls, pack_images(letterbox=...), and unletterbox_boxes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (h, w, S) -> (sh, sw, top, left)
CASES = [
    ((50, 100, 64), (32, 64, 16, 0)),         # wide image, even pad
    ((90, 30, 60), (60, 20, 0, 20)),          # tall image
    ((5, 128, 64), (2, 64, 31, 0)),           # 2.5 -> 2, half to even
    ((63, 128, 64), (32, 64, 16, 0)),         # 31.5 -> 32, half to even
    ((1, 200, 64), (1, 64, 31, 0)),           # the max(1, .) clamp
    ((33, 64, 64), (33, 64, 15, 0)),          # odd pad, floor
    ((23, 1, 64), (64, 3, 0, 30)),            # one-pixel-wide source
    ((1080, 1920, 416), (234, 416, 91, 0)),   # video frame
    ((128, 128, 64), (64, 64, 0, 0)),         # square source, no pad
]
SWEEP_SIZES = [27, 32, 51, 64, 96, 416, 608]


@pytest.fixture(scope="module")
def lib():
    from yolo_v3_tf2_amd import _lib
    return _lib.load()


def _descs(*rows):
    from yolo_v3_tf2_amd._lib import ImageDesc
    return (ImageDesc * len(rows))(*[ImageDesc(*r) for r in rows])


def _geometry(lib, hw_mode, S):
    """y3_letterbox_geometry over (h, w, mode) rows -> int32 [n,4]"""
    from yolo_v3_tf2_amd import _lib, runtime
    d = np.zeros(len(hw_mode), runtime.IMAGE_DESC_DTYPE)
    d["height"], d["width"], d["mode"] = [np.asarray(c) for c in zip(*hw_mode)]
    d["channels"] = 3
    out = np.full((len(d), 4), -7, np.int32)
    st = lib.y3_letterbox_geometry(d.ctypes.data_as(C.POINTER(_lib.ImageDesc)), len(d), S, out.ctypes.data_as(C.POINTER(C.c_int32)))
    assert st == 0, lib.y3_last_error()
    return out


def test_symbols_and_macro_declared_bound_and_exported(lib):
    from yolo_v3_tf2_amd import _lib
    raw = open(os.path.join(ROOT, "include", "y3.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ("y3_letterbox_geometry", "y3_unletterbox_detections"):
        assert re.search(r"\by3_status\s+%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"^#define Y3_IMAGE_LETTERBOX 0x100\s*$", header, flags=re.M)
    assert _lib.Y3_IMAGE_LETTERBOX == 0x100
    # the descriptor did not grow, and its typedef is the line it was
    assert re.search(r"typedef struct y3_image_desc \{ uint64_t offset; int32_t height, width, channels, mode; \}", header)
    assert C.sizeof(_lib.ImageDesc) == 24


@pytest.mark.parametrize("S", SWEEP_SIZES)
def test_geometry_sweep_equals_the_numpy_definition(lib, S):
    """Every h, w in 1..400 in one call: the library's fp32 geometry == core/utils.letterbox_geometry, it fits the canvas, and
    the longer side comes out as S.  (A double-precision implementation differs in 34 of these cases at S = 64, 416, 608.)"""
    from yolo_v3_tf2_amd import _lib
    from yolo_v3_tf2_amd.core.utils import letterbox_geometry
    h, w = [a.ravel() for a in np.meshgrid(np.arange(1, 401), np.arange(1, 401), indexing="ij")]
    got = _geometry(lib, list(zip(h.tolist(), w.tolist(), [1 | _lib.Y3_IMAGE_LETTERBOX] * h.size)), S)
    want = letterbox_geometry(h, w, S, S)
    assert want.dtype == np.int32 and want.shape == (h.size, 4)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (S, bad.size, [(int(h[i]), int(w[i]), got[i].tolist(), want[i].tolist()) for i in bad[:5]])
    sh, sw, top, left = got.T
    assert (sh >= 1).all() and (sw >= 1).all() and (top >= 0).all() and (left >= 0).all()
    assert (top + sh <= S).all() and (left + sw <= S).all()
    assert (np.where(h >= w, sh, sw) == S).all()


def test_double_precision_would_differ_somewhere():
    """The reason the precision is part of the contract: the float64 form of the formula disagrees inside the sweep."""
    from yolo_v3_tf2_amd.core.utils import letterbox_geometry
    h, w = [a.ravel() for a in np.meshgrid(np.arange(1, 401), np.arange(1, 401), indexing="ij")]
    differ = 0
    for S in (64, 416, 608):
        scale = np.minimum(S / h.astype(np.float64), S / w.astype(np.float64))
        d = np.stack([np.maximum(1, np.rint(scale * h)), np.maximum(1, np.rint(scale * w))], axis=-1).astype(np.int32)
        differ += int((d != letterbox_geometry(h, w, S, S)[:, :2]).any(axis=1).sum())
    assert differ == 34


@pytest.mark.parametrize("case,want", CASES)
def test_geometry_is_where_resize_image_puts_the_block(lib, case, want):
    from yolo_v3_tf2_amd import _lib
    from yolo_v3_tf2_amd.core.utils import letterbox_geometry, resize_image
    h, w, S = case
    flagged = _geometry(lib, [(h, w, _lib.Y3_IMAGE_LETTERBOX), (h, w, 1 | _lib.Y3_IMAGE_LETTERBOX), (h, w, 2 | _lib.Y3_IMAGE_LETTERBOX)], S)
    assert flagged.tolist() == [list(want)] * 3
    assert letterbox_geometry(h, w, S, S).tolist() == list(want)
    assert _geometry(lib, [(h, w, 0), (h, w, 1), (h, w, 2)], S).tolist() == [[S, S, 0, 0]] * 3, "unflagged images take the whole canvas"
    out = resize_image(np.ones((h, w, 3), np.float32), S, S)          # all-ones source: the block is exactly the non-zero part
    rows, cols = np.flatnonzero(out.any(axis=(1, 2))), np.flatnonzero(out.any(axis=(0, 2)))
    sh, sw, top, left = want
    assert (rows[0], rows[-1] + 1, cols[0], cols[-1] + 1) == (top, top + sh, left, left + sw)
    assert np.array_equal(out[top:top + sh, left:left + sw], np.ones((sh, sw, 3), np.float32)) and out.sum() == sh * sw * 3


# a pointer that is never dereferenced: every check below fails on the host before any HIP call
_FAKE = 0x10000
_LB = 0x100


@pytest.mark.parametrize("mode", [3 | _LB, 0x200, 0x101 | 0x400, -1, 3])
def test_bad_modes_are_refused_on_the_host(lib, mode):
    from yolo_v3_tf2_amd import _lib
    out = (C.c_int32 * 8)()
    rows = [(0, 8, 8, 3, 1 | _LB), (256, 8, 8, 3, mode)]
    st = lib.y3_preprocess_batch(_FAKE, 1 << 20, _descs(*rows), 2, _FAKE, 0, 64, None)
    assert st == _lib.Y3_ERR_INVALID and b"y3_preprocess_batch: image 1" in lib.y3_last_error(), lib.y3_last_error()
    st = lib.y3_letterbox_geometry(_descs(*rows), 2, 64, out)
    assert st == _lib.Y3_ERR_INVALID and b"y3_letterbox_geometry: image 1" in lib.y3_last_error(), lib.y3_last_error()
    st = lib.y3_preprocess_image(_FAKE, mode, 8, 8, 3, _FAKE, 0, 64, None)
    assert st == _lib.Y3_ERR_INVALID and b"y3_preprocess_image" in lib.y3_last_error()


def test_geometry_call_refuses_bad_arguments(lib):
    from yolo_v3_tf2_amd import _lib
    out = (C.c_int32 * 4)()
    d = _descs((0, 8, 8, 3, 1 | _LB))
    for args in ((None, 1, 64, out), (d, 1, 64, None), (d, 0, 64, out), (d, 1, 0, out), (_descs((0, 0, 8, 3, _LB)), 1, 64, out),
                 (_descs((0, 8, -2, 3, _LB)), 1, 64, out)):
        assert lib.y3_letterbox_geometry(*args) == _lib.Y3_ERR_INVALID, args
        assert b"y3_letterbox_geometry" in lib.y3_last_error()
    assert lib.y3_letterbox_geometry(d, 1, 64, out) == 0 and list(out) == [64, 64, 0, 0]


def _geoms(*rows):
    return (C.c_int32 * (4 * len(rows)))(*[v for r in rows for v in r])


@pytest.mark.parametrize("name,bad", [
    ("sh = 0", (0, 64, 0, 0)), ("sw = 0", (64, 0, 0, 0)), ("top < 0", (32, 64, -1, 0)), ("left < 0", (64, 32, 0, -1)),
    ("top + sh > S", (40, 64, 25, 0)), ("left + sw > S", (64, 40, 0, 25)), ("sh > S", (65, 64, 0, 0)),
    ("overflowing sum", (2**31 - 1, 64, 2**31 - 1, 0)),
])
def test_unletterbox_refuses_bad_geometries_and_names_the_image(lib, name, bad):
    from yolo_v3_tf2_amd import _lib
    good = (32, 64, 16, 0)
    st = lib.y3_unletterbox_detections(_FAKE, _FAKE, _geoms(good, good, bad), 3, 5, 64, None)
    assert st == _lib.Y3_ERR_INVALID, name
    assert b"y3_unletterbox_detections: image 2" in lib.y3_last_error(), lib.y3_last_error()


def test_unletterbox_refuses_bad_arguments(lib):
    from yolo_v3_tf2_amd import _lib
    g = _geoms((32, 64, 16, 0))
    for args in ((None, _FAKE, g, 1, 5, 64), (_FAKE, None, g, 1, 5, 64), (_FAKE, _FAKE, None, 1, 5, 64), (_FAKE, _FAKE, g, 0, 5, 64),
                 (_FAKE, _FAKE, g, 1, 0, 64), (_FAKE, _FAKE, g, 1, 1025, 64), (_FAKE, _FAKE, g, 1, -3, 64), (_FAKE, _FAKE, g, 1, 5, 0)):
        assert lib.y3_unletterbox_detections(*args, None) == _lib.Y3_ERR_INVALID, args
        assert b"y3_unletterbox_detections" in lib.y3_last_error()
    assert lib.y3_unletterbox_detections(_FAKE, _FAKE, g, 1, 1025, 64, None) == -1 and b"max_boxes" in lib.y3_last_error()


def test_pack_images_letterbox_flag():
    from yolo_v3_tf2_amd import _lib, runtime
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, (5, 7, 3), dtype=np.uint8), rng.random((3, 2, 4), dtype=np.float32),
            rng.integers(0, 256, (1, 33, 3), dtype=np.uint8)]
    modes = [1, 0, 2]
    blob0, d0 = runtime.pack_images(imgs, modes)
    assert d0["mode"].tolist() == modes, "descriptors without the keyword are what they were"
    blob1, d1 = runtime.pack_images(imgs, modes, letterbox=False)
    def pixels(blob, descs):      # the bytes between two images are padding and hold nothing
        return [blob[int(d["offset"]):int(d["offset"]) + im.nbytes].tobytes() for d, im in zip(descs, imgs)]

    assert np.array_equal(d0, d1) and pixels(blob0, d0) == pixels(blob1, d1) == [im.tobytes() for im in imgs]
    _, d2 = runtime.pack_images(imgs, modes, letterbox=True)
    assert d2["mode"].tolist() == [m | _lib.Y3_IMAGE_LETTERBOX for m in modes]
    blob3, d3 = runtime.pack_images(imgs, modes, letterbox=[True, False, True])
    assert d3["mode"].tolist() == [1 | 0x100, 0, 2 | 0x100] and pixels(blob3, d3) == pixels(blob0, d0)
    for name in ("offset", "height", "width", "channels"):
        assert np.array_equal(d3[name], d0[name]), name
    with pytest.raises(runtime.Y3Error):
        runtime.pack_images(imgs, modes, letterbox=[True, False])
    # the geometry of the whole batch in one call, no GPU needed
    assert runtime.letterbox_geometries(d3, 64).tolist() == [[46, 64, 9, 0], [64, 64, 0, 0], [2, 64, 31, 0]]
    assert runtime.letterbox_geometries(d0, 64).tolist() == [[64, 64, 0, 0]] * 3
    with pytest.raises(runtime.Y3Error):
        runtime.letterbox_geometries(np.zeros(2, np.int32), 64)


@pytest.mark.parametrize("case,geom", CASES)
def test_unletterbox_boxes_maps_the_block_to_the_unit_square(case, geom):
    """The block's corners on the padded canvas, normalised as the detector reports them, come back as (0, 0, 1, 1) within one
    ulp of 1 (four fp32 roundings; the zero corners are exact when left / S * S rounds back to left, one ulp of the divisor's
    quotient otherwise)."""
    from yolo_v3_tf2_amd.core.utils import unletterbox_boxes
    S = case[2]
    sh, sw, top, left = geom
    box = np.array([[left, top, left + sw, top + sh]], np.float32) / np.float32(S)
    out = unletterbox_boxes(box, geom, S)
    assert out.dtype == np.float32 and out.shape == (1, 4)
    ulp = np.spacing(np.float32(1.0))
    assert np.abs(out - np.array([0, 0, 1, 1], np.float32)).max() <= ulp, out
    # the restated arithmetic, operation by operation
    fs = np.float32(S)
    want = [(box[0, 0] * fs - np.float32(left)) / np.float32(sw), (box[0, 1] * fs - np.float32(top)) / np.float32(sh),
            (box[0, 2] * fs - np.float32(left)) / np.float32(sw), (box[0, 3] * fs - np.float32(top)) / np.float32(sh)]
    assert out[0].tolist() == [float(v) for v in want]


def test_unletterbox_boxes_leaves_the_whole_canvas_alone():
    from yolo_v3_tf2_amd.core.utils import unletterbox_boxes
    S = 416
    boxes = np.random.default_rng(12).random((3, 50, 4), dtype=np.float32)
    assert not np.array_equal((boxes * np.float32(S)) / np.float32(S), boxes), "x * S / S is not x in fp32: the shortcut matters"
    keep = boxes.copy()
    out = unletterbox_boxes(boxes, (S, S, 0, 0), S)
    assert np.array_equal(out, keep) and np.array_equal(boxes, keep)
    moved = unletterbox_boxes(boxes, (234, 416, 91, 0), S)
    assert moved.shape == boxes.shape and np.array_equal(moved[..., 0], (boxes[..., 0] * np.float32(S) - np.float32(0)) / np.float32(416))
    assert np.array_equal(moved[..., 1], (boxes[..., 1] * np.float32(S) - np.float32(91)) / np.float32(234))
