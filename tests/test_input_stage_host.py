"""Batched input stage, host tier (no GPU): the y3_preprocess_batch ABI and its argument checks, pack_images, and the
absence of a CPU fallback."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from yolo_v3_tf2_amd import _lib
    return _lib.load()


def _descs(*rows):
    from yolo_v3_tf2_amd._lib import ImageDesc
    return (ImageDesc * len(rows))(*[ImageDesc(*r) for r in rows])


def test_symbol_declared_bound_and_exported(lib):
    from yolo_v3_tf2_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "y3.h")).read(), flags=re.S)
    assert re.search(r"\by3_preprocess_batch\s*\(", header)
    assert re.search(r"typedef struct y3_image_desc \{ uint64_t offset; int32_t height, width, channels, mode; \}", header)
    assert "y3_preprocess_batch" in _lib.SYMBOLS
    assert hasattr(lib, "y3_preprocess_batch")
    assert C.sizeof(_lib.ImageDesc) == 24


# a pointer that is never dereferenced: every check below fails on the host before any HIP call
_FAKE = 0x10000


@pytest.mark.parametrize("name,pixels,nbytes,rows,n,batch", [
    ("null pixels", None, 1 << 20, [(0, 8, 8, 3, 1)], 1, _FAKE),
    ("null descriptors", _FAKE, 1 << 20, None, 1, _FAKE),
    ("null batch", _FAKE, 1 << 20, [(0, 8, 8, 3, 1)], 1, None),
    ("n_images = 0", _FAKE, 1 << 20, [(0, 8, 8, 3, 1)], 0, _FAKE),
    ("channels = 2", _FAKE, 1 << 20, [(0, 8, 8, 3, 1), (256, 8, 8, 2, 1)], 2, _FAKE),
    ("mode = 3", _FAKE, 1 << 20, [(0, 8, 8, 3, 3)], 1, _FAKE),
    ("height = 0", _FAKE, 1 << 20, [(0, 0, 8, 3, 1)], 1, _FAKE),
    ("past the blob, uint8", _FAKE, 8 * 8 * 3 + 15, [(16, 8, 8, 3, 1)], 1, _FAKE),
    ("past the blob, float32", _FAKE, 8 * 8 * 3 * 4 - 1, [(0, 8, 8, 3, 0)], 1, _FAKE),
    ("past the blob, 64-bit sizes", _FAKE, 1 << 20, [(0, 2**31 - 1, 2**31 - 1, 4, 0)], 1, _FAKE),
    ("offset wraps", _FAKE, 1 << 20, [(2**64 - 16, 8, 8, 3, 1)], 1, _FAKE),
    ("misaligned float offset", _FAKE, 1 << 20, [(0, 8, 8, 3, 0), (770, 8, 8, 3, 0)], 2, _FAKE),
])
def test_bad_arguments_are_refused_on_the_host(lib, name, pixels, nbytes, rows, n, batch):
    from yolo_v3_tf2_amd import _lib
    descs = _descs(*rows) if rows is not None else None
    st = lib.y3_preprocess_batch(pixels, nbytes, descs, n, batch, 0, 64, None)
    assert st == _lib.Y3_ERR_INVALID, name
    msg = lib.y3_last_error()
    assert b"y3_preprocess_batch" in msg, msg


def test_message_names_the_bad_image(lib):
    st = lib.y3_preprocess_batch(_FAKE, 1 << 20, _descs((0, 8, 8, 3, 1), (256, 8, 8, 3, 1), (512, 8, 8, 5, 1)), 3, _FAKE, 0, 64, None)
    assert st == -1 and b"image 2" in lib.y3_last_error()
    st = lib.y3_preprocess_batch(_FAKE, 1 << 20, _descs((0, 8, 8, 3, 1)), 1, _FAKE, -1, 64, None)
    assert st == -1 and b"y3_preprocess_batch" in lib.y3_last_error()


def _images(rng):
    return [rng.integers(0, 256, (5, 7, 3), dtype=np.uint8), rng.random((3, 2, 4), dtype=np.float32),
            rng.integers(0, 256, (1, 1, 4), dtype=np.uint8), rng.integers(0, 256, (1, 33, 3), dtype=np.uint8),
            rng.random((9, 4, 3), dtype=np.float32)[:, ::2]]          # the last one is not contiguous


def test_pack_images_layout():
    from yolo_v3_tf2_amd import _lib, runtime
    imgs = _images(np.random.default_rng(5))
    modes = [1, 0, 2, 1, 0]
    blob, descs = runtime.pack_images(imgs, modes)
    assert blob.dtype == np.uint8 and blob.ndim == 1 and blob.flags.c_contiguous
    assert descs.dtype == runtime.IMAGE_DESC_DTYPE and descs.dtype.itemsize == C.sizeof(_lib.ImageDesc) == 24
    for name, (ctype_name, ctype) in zip(descs.dtype.names, _lib.ImageDesc._fields_):
        assert name == ctype_name and descs.dtype.fields[name][1] == getattr(_lib.ImageDesc, name).offset
        assert descs.dtype.fields[name][0].itemsize == C.sizeof(ctype)
    end = 0
    for im, m, d in zip(imgs, modes, descs):
        off = int(d["offset"])
        assert off % 16 == 0 and off >= end            # aligned, and after the previous image
        end = off + im.nbytes
        assert (d["height"], d["width"], d["channels"], d["mode"]) == (*im.shape, m)
        assert np.array_equal(blob[off:end].view(im.dtype).reshape(im.shape), im)
    assert blob.size == end == runtime.packed_nbytes(imgs)
    # one mode for the whole list
    u8 = [im for im in imgs if im.dtype == np.uint8]
    _, d2 = runtime.pack_images(u8, 2)
    assert d2["mode"].tolist() == [2] * len(u8)


def test_pack_images_into_a_callers_buffer():
    from yolo_v3_tf2_amd import runtime
    imgs = [im for im in _images(np.random.default_rng(6)) if im.dtype == np.uint8]
    need = runtime.packed_nbytes(imgs)
    out = np.zeros(need + 100, np.uint8)
    blob, descs = runtime.pack_images(imgs, 1, out=out)
    assert blob.size == need and np.shares_memory(blob, out)
    with pytest.raises(runtime.Y3Error):
        runtime.pack_images(imgs, 1, out=np.zeros(need - 1, np.uint8))
    with pytest.raises(runtime.Y3Error):
        runtime.pack_images(imgs, 1, out=np.zeros(need, np.float32))


def test_pack_images_refuses_what_the_kernel_cannot_read():
    from yolo_v3_tf2_amd import runtime
    rng = np.random.default_rng(7)
    u8 = rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)
    for bad, mode in ((u8.astype(np.float64), 0), (u8.astype(np.int32), 1),     # wrong dtype
                      (u8, 0), (u8.astype(np.float32), 1), (u8.astype(np.float32), 2),  # dtype against the mode
                      (u8[..., 0], 1), (u8[None], 1),                            # wrong rank
                      (u8[..., :2], 1), (np.zeros((4, 4, 5), np.uint8), 1),      # wrong channel count
                      (np.zeros((0, 4, 3), np.uint8), 1),                        # empty
                      (u8, 3), (u8.tolist(), 1)):
        with pytest.raises(runtime.Y3Error):
            runtime.pack_images([bad], mode)
    with pytest.raises(runtime.Y3Error):
        runtime.pack_images([u8, u8], [1])


def test_no_cpu_fallback():
    """Host tensors are refused, and without a GPU the stage cannot be built: nothing is computed on the host instead."""
    import torch
    from yolo_v3_tf2_amd import runtime
    u8 = np.random.default_rng(8).integers(0, 256, (4, 4, 3), dtype=np.uint8)
    blob, descs = runtime.pack_images([u8], 1)
    batch = torch.zeros((1, 8, 8, 3))
    with pytest.raises(runtime.Y3Error):
        runtime.preprocess_batch(torch.from_numpy(blob), descs, batch)
    assert not batch.any()
    if not torch.cuda.is_available():
        with pytest.raises(runtime.Y3Error):
            runtime.InputStage(64, 4, 1 << 16)
