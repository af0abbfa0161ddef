"""The host-to-device input path: canvas geometry, the pixel blob of a batch (pack_images), the resize kernels' wrappers, the
letterbox geometry and its inverse on packed detections, and InputStage, the ring that overlaps all of it with the consumer."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._args import _dev, _need_cuda
from ._lib import Y3Error, check


def canvas_hw(image_size):
    """An image size as the (H, W) of the network canvas: an int S is the square (S, S), a pair is taken as (H, W)."""
    if isinstance(image_size, (int, np.integer)):
        return int(image_size), int(image_size)
    hw = tuple(int(v) for v in image_size)
    if len(hw) != 2:
        raise Y3Error(f"image_size must be an int or an (H, W) pair (got {image_size!r})")
    return hw


def _f32_geometry(h: int, w: int, Hc: int, Wc: int):
    """(sh, sw) of the letterbox geometry in the library's own fp32 arithmetic (include/y3.h, Y3_IMAGE_LETTERBOX;
    core/utils.letterbox_geometry is the same restatement with the offsets)."""
    scale = min(np.float32(Hc) / np.float32(h), np.float32(Wc) / np.float32(w))
    return max(1, int(np.rint(scale * np.float32(h)))), max(1, int(np.rint(scale * np.float32(w))))


def rect_canvas(height: int, width: int, image_size: int, stride: int = 32):
    """The smallest (H, W) canvas, both sides multiples of `stride`, that holds the aspect-preserving resize of a
    height x width frame whose long side becomes image_size -- the plan to letterbox such frames onto instead of the
    image_size^2 square, whose zero bars the conv stack would convolve.  (480, 640, 416) -> (320, 416).
    The resized extent is computed with the library's fp32 geometry; the canvas found is then checked with the same
    geometry (the frame letterboxed onto it must fit) and a side grows by one stride where rounding says otherwise."""
    h, w, S, st = int(height), int(width), int(image_size), int(stride)
    if h < 1 or w < 1 or S < 1 or st < 1:
        raise Y3Error("rect_canvas: height, width, image_size and stride must be at least 1")
    sh, sw = _f32_geometry(h, w, S, S)
    up = lambda v: -(-v // st) * st
    H, W = up(sh), up(sw)
    while True:
        gh, gw = _f32_geometry(h, w, H, W)
        if gh <= H and gw <= W:
            return H, W
        H, W = (H + st, W) if gh > H else (H, W + st)


def rect_anchors(anchors_table, image_size: int, canvas):
    """Anchors normalised by the square image_size (datasets/*/anchors.txt through core.utils.get_anchors) -> normalised
    by an (H, W) canvas: aw * S / W, ah * S / H, in fp32.  The anchor keeps its size in pixels.  An axis whose side equals
    image_size -- the long side of every rect_canvas -- is copied, not computed: x * S / S is not x in fp32."""
    H, W = canvas_hw(canvas)
    a = np.asarray(anchors_table, np.float32)
    out = a.copy()
    if W != int(image_size):
        out[..., 0] = a[..., 0] * np.float32(image_size) / np.float32(W)
    if H != int(image_size):
        out[..., 1] = a[..., 1] * np.float32(image_size) / np.float32(H)
    return out


def preprocess_image(image: torch.Tensor, batch: torch.Tensor, slot: int, divide_after: bool = False, letterbox: bool = False):
    """image [H,W,3|4] uint8 or float32 on the GPU -> batch[slot] ([Hc,Wc,3] fp32, the canvas the batch's shape names; values in [0,1] for uint8 input):
    decode_image's uint8->float conversion fused with tf.image.resize's bilinear resampling.  divide_after=True is
    the tfrecords source's order (reference: core/load_tfrecords.py:46-48): resize the 0..255 values, then / 255.
    letterbox=True keeps the aspect ratio and pads with zeros (reference: core/utils.py:17-28, resize_image); the whole
    slot is written."""
    _need_cuda(image, batch)
    if image.dim() != 3 or image.dtype not in (torch.uint8, torch.float32) or batch.dtype != torch.float32:
        raise Y3Error("image must be [H,W,C] uint8/float32 and batch float32 [B,Hc,Wc,3]")
    if batch.dim() != 4 or batch.shape[3] != 3 or not (0 <= slot < batch.shape[0]):
        raise Y3Error("batch must be [B,Hc,Wc,3] and slot inside it")
    H, W, C_ = image.shape
    mode = (2 if divide_after else 1) if image.dtype == torch.uint8 else 0
    if divide_after and mode == 0:
        raise Y3Error("divide_after applies to uint8 images")
    if letterbox:
        mode |= _lib.Y3_IMAGE_LETTERBOX
    check(_lib.load().y3_preprocess_image_hw(_dev(image), mode, H, W, C_, _dev(batch), slot,
                                             batch.shape[1], batch.shape[2], _lib.stream_ptr()), "y3_preprocess_image")
    return batch


# y3_image_desc (include/y3.h), as a NumPy structured dtype: what pack_images returns and preprocess_batch takes
IMAGE_DESC_DTYPE = np.dtype([("offset", "<u8"), ("height", "<i4"), ("width", "<i4"), ("channels", "<i4"), ("mode", "<i4")])
_BLOB_ALIGN = 16     # image starts inside a pixel blob


def _image_modes(images, mode):
    if np.ndim(mode) == 0:
        modes = [int(mode)] * len(images)
    else:
        modes = [int(m) for m in mode]
        if len(modes) != len(images):
            raise Y3Error(f"pack_images: {len(modes)} modes for {len(images)} images")
    for i, (im, m) in enumerate(zip(images, modes)):
        if not isinstance(im, np.ndarray) or im.ndim != 3 or im.shape[2] not in (3, 4) or 0 in im.shape:
            raise Y3Error(f"pack_images: image {i} must be a non-empty NumPy array [H,W,3|4]")
        want = {0: np.float32, 1: np.uint8, 2: np.uint8}.get(m)
        if want is None:
            raise Y3Error(f"pack_images: image {i}: mode must be 0, 1 or 2 (got {m})")
        if im.dtype != want:
            raise Y3Error(f"pack_images: image {i} is {im.dtype}, mode {m} takes {np.dtype(want)}")
    return modes


def _blob_offsets(images):
    offsets, end = [], 0
    for im in images:
        start = -(-end // _BLOB_ALIGN) * _BLOB_ALIGN
        offsets.append(start)
        end = start + im.nbytes
    return offsets, end


def packed_nbytes(images) -> int:
    """Bytes pack_images needs for this list (image starts 16-byte aligned)."""
    return _blob_offsets(images)[1]


def _image_flags(images, letterbox):
    if np.ndim(letterbox) == 0:
        return [_lib.Y3_IMAGE_LETTERBOX if letterbox else 0] * len(images)
    flags = [_lib.Y3_IMAGE_LETTERBOX if f else 0 for f in letterbox]
    if len(flags) != len(images):
        raise Y3Error(f"pack_images: {len(flags)} letterbox flags for {len(images)} images")
    return flags


def pack_images(images, mode, out: Optional[np.ndarray] = None, letterbox=False):
    """A list of [H,W,3|4] uint8 / float32 arrays -> (blob_u8, descs): one contiguous byte buffer with every image start
    16-byte aligned, and the y3_image_desc array (IMAGE_DESC_DTYPE) that names them.  Pure NumPy.
    mode: one value for the whole list or one per image -- 0 float32, 1 uint8 scaled by 1/255 before the resize (the
    image_file / images_dir sources), 2 uint8 divided by 255 after it (the tfrecords source).
    letterbox: one bool for the whole list or one per image -- True sets Y3_IMAGE_LETTERBOX in the descriptor's mode: the
    image keeps its aspect ratio and is padded with zeros (core/utils.resize_image) instead of being stretched.
    out: a 1-D uint8 array to pack into (e.g. a view of pinned memory); blob_u8 is then its used prefix."""
    images = list(images)
    modes = _image_modes(images, mode)
    flags = _image_flags(images, letterbox)
    offsets, total = _blob_offsets(images)
    if out is None:
        out = np.empty(total, np.uint8)
    elif not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.ndim != 1 or not out.flags.c_contiguous:
        raise Y3Error("pack_images: out must be a contiguous 1-D uint8 array")
    elif out.size < total:
        raise Y3Error(f"pack_images: out holds {out.size} bytes, the images need {total}")
    descs = np.zeros(len(images), IMAGE_DESC_DTYPE)
    for i, (im, m, f, off) in enumerate(zip(images, modes, flags, offsets)):
        np.copyto(out[off:off + im.nbytes].view(im.dtype).reshape(im.shape), im)
        descs[i] = (off, im.shape[0], im.shape[1], im.shape[2], m | f)
    return out[:total], descs


# The two kinds of descriptor array: (dtype, ctypes struct, what the array is called in messages)
_IMAGES = (IMAGE_DESC_DTYPE, _lib.ImageDesc, "the descriptor array of pack_images")


def _descs_ptr(descs, kind):
    dtype, ctype, what = kind
    if not isinstance(descs, np.ndarray) or descs.dtype != dtype or descs.ndim != 1:
        raise Y3Error(f"descs must be {what}")
    d = np.ascontiguousarray(descs)
    return d, d.ctypes.data_as(C.POINTER(ctype))


def _geometries(descs, image_size, kind, entry, name):
    d, d_ptr = _descs_ptr(descs, kind)
    geoms = np.empty((len(d), 4), np.int32)
    Hc, Wc = canvas_hw(image_size)
    check(getattr(_lib.load(), entry)(d_ptr, len(d), Hc, Wc, geoms.ctypes.data_as(C.POINTER(C.c_int32))), name)
    return geoms


def _preprocess(blob_dev, descs, batch, first_slot, kind, entry, name):
    _need_cuda(blob_dev, batch)
    if blob_dev.dtype != torch.uint8 or blob_dev.dim() != 1:
        raise Y3Error("blob_dev must be a 1-D uint8 tensor")
    d, d_ptr = _descs_ptr(descs, kind)
    if batch.dtype != torch.float32 or batch.dim() != 4 or batch.shape[3] != 3:
        raise Y3Error("batch must be float32 [B,Hc,Wc,3]")
    if not (0 <= first_slot and first_slot + len(descs) <= batch.shape[0]):
        raise Y3Error(f"slots {first_slot}..{first_slot + len(descs) - 1} are outside the batch of {batch.shape[0]}")
    check(getattr(_lib.load(), entry)(_dev(blob_dev), blob_dev.numel(), d_ptr, len(d), _dev(batch), int(first_slot),
                                      batch.shape[1], batch.shape[2], _lib.stream_ptr()), name)
    return batch


def letterbox_geometries(descs: np.ndarray, image_size) -> np.ndarray:
    """The descriptor array of pack_images -> int32 [n,4] (sh, sw, top, left): where each image lies on the
    canvas (image_size: an int S or an (H, W) pair), the whole canvas (H, W, 0, 0) for an image without the letterbox flag.  One host call for the whole batch
    (y3_letterbox_geometry; no GPU needed); the rows unletterbox_detections takes."""
    return _geometries(descs, image_size, _IMAGES, "y3_letterbox_geometry_hw", "y3_letterbox_geometry")


def unletterbox_detections(packed: torch.Tensor, num_valid: torch.Tensor, geoms, image_size):
    """packed [B,M,7] int32 words and num_valid [B] int32 on the GPU (Net.detect / pack_detections), geoms int32 [B,4]
    on the host (letterbox_geometries): the boxes of the valid rows are rewritten in place from the padded canvas to
    the coordinates of the source frames (y3_unletterbox_detections; host restatement: core/utils.unletterbox_boxes).
    Nothing else is touched.  image_size: the canvas, an int S or an (H, W) pair.  Enqueues on the current stream only."""
    _need_cuda(packed, num_valid)
    if packed.dtype != torch.int32 or packed.dim() != 3 or packed.shape[2] != 7 or not packed.is_contiguous():
        raise Y3Error("packed must be contiguous int32 [B,M,7]")
    if num_valid.dtype != torch.int32 or num_valid.shape != (packed.shape[0],) or not num_valid.is_contiguous():
        raise Y3Error("num_valid must be contiguous int32 [B]")
    g = np.ascontiguousarray(geoms, dtype=np.int32)
    if g.shape != (packed.shape[0], 4):
        raise Y3Error(f"geoms must be int32 [{packed.shape[0]},4]")
    Hc, Wc = canvas_hw(image_size)
    check(_lib.load().y3_unletterbox_detections_hw(_dev(packed), _dev(num_valid), g.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   packed.shape[0], packed.shape[1], Hc, Wc, _lib.stream_ptr()),
          "y3_unletterbox_detections")
    return packed


def preprocess_batch(blob_dev: torch.Tensor, descs: np.ndarray, batch: torch.Tensor, first_slot: int = 0):
    """The pixel blob of pack_images on the GPU (1-D uint8) -> batch[first_slot + i] for image i, one launch per 72
    images (y3_preprocess_batch); every slot has the bits preprocess_image gives for the same image."""
    return _preprocess(blob_dev, descs, batch, first_slot, _IMAGES, "y3_preprocess_batch_hw", "y3_preprocess_batch")


# y3_tile_desc (include/y3.h): a window (y0, x0, ch, cw) of an image of a pixel blob; what tile_descs returns and preprocess_tiles takes
TILE_DESC_DTYPE = np.dtype([("offset", "<u8"), ("height", "<i4"), ("width", "<i4"), ("channels", "<i4"), ("mode", "<i4"),
                            ("y0", "<i4"), ("x0", "<i4"), ("ch", "<i4"), ("cw", "<i4")])


def tile_grid(height, width, rows, cols, overlap_px=0, overview=False) -> np.ndarray:
    """y3_tile_grid: the windows of a height x width frame, int32 [T,4] = (y0, x0, ch, cw), row-major, the overview tile (the
    whole frame) last; Y3Error for what the library refuses.  One host call, no GPU.  NumPy restatement: tiles.tile_grid."""
    out = np.empty((_lib.MAX_TILES + 1, 4), np.int32)
    T = _lib.load().y3_tile_grid(int(height), int(width), int(rows), int(cols), int(overlap_px), int(bool(overview)),
                                 out.ctypes.data_as(C.POINTER(C.c_int32)))
    if T < 0:       # the status; the count otherwise
        check(T, "y3_tile_grid")
    return out[:T].copy()


def tile_descs(images, descs, rows, cols, overlap_px=0, overview=False):
    """The descriptor array of pack_images -> (tile descriptors [n*T] (TILE_DESC_DTYPE), windows int32 [n*T,4]): the grid of
    y3_tile_grid over every image, tile t of image i at index i * T + t.  A tile names its image's pixels in the blob, which
    therefore holds -- and uploads -- every frame once.  images: the list the descriptors were packed from (only its length is
    checked), or None."""
    d, _ = _descs_ptr(descs, _IMAGES)
    if images is not None and len(images) != len(d):
        raise Y3Error(f"tile_descs: {len(images)} images, {len(d)} descriptors")
    T = int(rows) * int(cols) + (1 if overview else 0)
    out = np.zeros(len(d) * T, TILE_DESC_DTYPE)
    windows = np.empty((len(d) * T, 4), np.int32)
    grids = {}      # one library call per distinct frame shape
    for i, im in enumerate(d):
        hw = (int(im["height"]), int(im["width"]))
        if hw not in grids:
            grids[hw] = tile_grid(*hw, rows, cols, overlap_px, overview)
        windows[i * T:(i + 1) * T] = grids[hw]
        for name in ("offset", "height", "width", "channels", "mode"):
            out[name][i * T:(i + 1) * T] = im[name]
    for k, name in enumerate(("y0", "x0", "ch", "cw")):
        out[name] = windows[:, k]
    return out, windows


_TILES = (TILE_DESC_DTYPE, _lib.TileDesc, "the tile descriptor array of tile_descs")


def tile_letterbox_geometries(descs: np.ndarray, image_size) -> np.ndarray:
    """letterbox_geometries for tile descriptors: int32 [n,4] (sh, sw, top, left) of each window taken as a ch x cw image
    (y3_tile_letterbox_geometry_hw); the rows merge_tile_detections takes."""
    return _geometries(descs, image_size, _TILES, "y3_tile_letterbox_geometry_hw", "y3_tile_letterbox_geometry")


def preprocess_tiles(blob_dev: torch.Tensor, descs: np.ndarray, batch: torch.Tensor, first_slot: int = 0):
    """preprocess_batch for windows: the pixel blob of pack_images on the GPU and the tile descriptors of tile_descs ->
    batch[first_slot + i] for tile i, one launch per 72 tiles (y3_preprocess_tiles_hw, the same kernel reading the frame with its own
    row pitch); every slot has the bits preprocess_batch gives for a contiguous copy of the window."""
    return _preprocess(blob_dev, descs, batch, first_slot, _TILES, "y3_preprocess_tiles_hw", "y3_preprocess_tiles")


class StagedBatch:
    """What InputStage.submit returns: `batch` ([n,S,S,3] fp32 on the GPU) holds the images once a stream has waited on
    the event `ready`; hand it back with InputStage.release when the consumer's work on it is enqueued.  `geometry`
    (int32 [n,4] on the host: sh, sw, top, left) says where each frame lies in its slot.  `frames`: how many frames were handed in, n."""

    def __init__(self, slot, batch, ready, geometry):
        self.slot, self.batch, self.ready, self.geometry = slot, batch, ready, geometry

    @property
    def frames(self) -> int:
        return self.batch.shape[0]


class StagedTiles(StagedBatch):
    """What TiledInputStage.submit returns: the batch holds frames * T tile images, tile t of frame f in slot f * T + t; `geometry` is
    per tile, `windows` (int32 [frames*T,4]: y0, x0, ch, cw) and `frame_hw` (int32 [frames,2]) are the other two tables
    merge_tile_detections takes, and `frames` counts the frames."""

    def __init__(self, slot, batch, ready, geometry, windows, frame_hw):
        super().__init__(slot, batch, ready, geometry)
        self.windows, self.frame_hw = windows, frame_hw

    @property
    def frames(self) -> int:
        return len(self.frame_hw)


class _StageSlot:
    def __init__(self, image_size, max_batch, max_blob_bytes, device):
        self.pinned = torch.empty(max_blob_bytes, dtype=torch.uint8, pin_memory=True)
        self.pinned_np = self.pinned.numpy()
        self.blob_dev = torch.empty(max_blob_bytes, dtype=torch.uint8, device=device)
        self.batch = torch.empty((max_batch, *canvas_hw(image_size), 3), dtype=torch.float32, device=device)
        self.ready = torch.cuda.Event()      # copy stream: pixels copied and resized into `batch`
        self.released = torch.cuda.Event()   # consumer stream: `batch` has been read
        self.state = "free"                  # free -> held (submit) -> released (release) -> held ...


class InputStage:
    """Host frames -> device batches, overlapped with the consumer: a ring of `depth` slots, each a pinned host blob, a
    device blob and a device batch [max_batch,S,S,3], fed by one copy stream.
    submit(images, mode, letterbox) packs the list into the next slot's pinned blob and enqueues, on the copy stream, one
    host-to-device copy and y3_preprocess_batch; release(handle) tells the stage that the consumer's reads are enqueued.
    Every wait is on an event: the host waits for `ready` of the slot's previous use before it overwrites the pinned
    blob, the copy stream waits for `released` before it overwrites the device buffers.  Nothing synchronises the device."""

    tiles_per_image = 1     # images a frame becomes in the device batch; TiledInputStage sets its T before the slots are made

    def __init__(self, image_size, max_batch: int, max_blob_bytes: int, depth: int = 2):
        _lib.require_gpu()      # image_size: an int S or an (H, W) canvas
        if min(canvas_hw(image_size)) < 1 or max_batch < 1 or max_blob_bytes < 1 or depth < 1:
            raise Y3Error("InputStage: image_size, max_batch, max_blob_bytes and depth must be at least 1")
        self.image_size = int(image_size) if isinstance(image_size, (int, np.integer)) else canvas_hw(image_size)
        self.max_batch, self.depth = int(max_batch), int(depth)
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.stream = torch.cuda.Stream(self.device)
        self.slots = [_StageSlot(self.image_size, self.max_batch * self.tiles_per_image, int(max_blob_bytes), self.device)
                      for _ in range(self.depth)]
        for s in self.slots:     # used on the copy stream for as long as the stage lives
            s.blob_dev.record_stream(self.stream)
            s.batch.record_stream(self.stream)
        self._next = 0

    def _resize(self, slot, images, descs):
        """The packed frames of a slot -> (launch, handle): `launch` enqueues their resize into slot.batch on the current stream, and
        `handle` is what submit returns, its geometry computed here with one host call per batch."""
        handle = StagedBatch(slot, slot.batch[:len(images)], slot.ready, letterbox_geometries(descs, self.image_size))
        return (lambda: preprocess_batch(slot.blob_dev, descs, slot.batch, 0)), handle

    def submit(self, images, mode, letterbox=False) -> StagedBatch:
        images = list(images)
        if not 1 <= len(images) <= self.max_batch:
            raise Y3Error(f"InputStage.submit: {len(images)} images, the stage holds 1..{self.max_batch}")
        slot = self.slots[self._next]
        if slot.state == "held":
            raise Y3Error(f"InputStage.submit: all {self.depth} slots are in use; release() the oldest batch first")
        if slot.state == "released":
            slot.ready.synchronize()     # the slot's earlier copy has left the pinned blob
        blob, descs = pack_images(images, mode, out=slot.pinned_np, letterbox=letterbox)
        launch, handle = self._resize(slot, images, descs)
        n = blob.size
        with torch.cuda.stream(self.stream):
            if slot.state == "released":
                self.stream.wait_event(slot.released)
            slot.blob_dev[:n].copy_(slot.pinned[:n], non_blocking=True)
            launch()
            slot.ready.record(self.stream)
        slot.state = "held"
        self._next = (self._next + 1) % self.depth
        return handle

    def release(self, handle: StagedBatch):
        """Call on the consumer's stream after its last use of handle.batch has been enqueued."""
        if handle.slot.state != "held" or handle.ready is not handle.slot.ready:
            raise Y3Error("InputStage.release: not a batch in flight")
        handle.slot.released.record(torch.cuda.current_stream())
        handle.slot.state = "released"


def tiles_arg(who, tiles):
    """(rows, cols, overlap_px, overview) as the streams and TiledInputStage take it -> the tuple in its types, and T, the tile images per
    frame; Y3Error for what no frame could be cut by (y3_tile_grid refuses the rest per frame: an overlap larger than the frame)."""
    try:
        rows, cols, overlap_px, overview = tiles
        t = (int(rows), int(cols), int(overlap_px), bool(overview))
    except (TypeError, ValueError):
        raise Y3Error(f"{who}: tiles must be (rows, cols, overlap_px, overview) (got {tiles!r})") from None
    T = t[0] * t[1] + (1 if t[3] else 0)
    if not (1 <= t[0] <= 8 and 1 <= t[1] <= 8 and t[2] >= 0 and T <= _lib.MAX_TILES):
        raise Y3Error(f"{who}: tiles: rows and cols in [1,8], overlap_px >= 0, at most {_lib.MAX_TILES} tiles per frame (got {t!r})")
    return t, T


class TiledInputStage(InputStage):
    """InputStage for sliced inference: tiles = (rows, cols, overlap_px, overview), T = rows * cols + overview tile images per frame.
    The device batches hold max_batch * T images; submit packs and uploads the frames ONCE, exactly as InputStage does, and
    y3_preprocess_tiles_hw cuts every frame's windows (y3_tile_grid) out of that one upload, each window stretched -- or with
    letterbox=True letterboxed -- onto the canvas as an image of its own.  The handle is a StagedTiles."""

    def __init__(self, image_size, max_batch: int, max_blob_bytes: int, tiles, depth: int = 2):
        self.tiles, self.tiles_per_image = tiles_arg("TiledInputStage", tiles)
        super().__init__(image_size, max_batch, max_blob_bytes, depth)

    def _resize(self, slot, images, descs):
        tdescs, windows = tile_descs(images, descs, *self.tiles)
        geometry = tile_letterbox_geometries(tdescs, self.image_size)
        frame_hw = np.stack([descs["height"], descs["width"]], axis=1).astype(np.int32)
        handle = StagedTiles(slot, slot.batch[:len(geometry)], slot.ready, geometry, windows, frame_hw)
        return (lambda: preprocess_tiles(slot.blob_dev, tdescs, slot.batch, 0)), handle
