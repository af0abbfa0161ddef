"""Host mirror of the helpers of reference core/utils.py that sit on the inference path."""
import os

import numpy as np


def get_anchors(anchors_file):
    """reference: core/utils.py:31-37 -- `loadtxt(delimiter=',')` then reshape(-1, 3, 2): row-major, so table[0] holds
    the first three lines of the file (the largest anchors in the COCO file, used by the coarsest grid)."""
    nanchors_per_scale = 3
    anchor_entry_size = 2
    anchors_table = np.loadtxt(anchors_file, dtype=float, delimiter=",")
    return anchors_table.reshape(-1, nanchors_per_scale, anchor_entry_size)


def dir_filelist(images_dir, ext_list=".*"):
    """reference: core/utils.py:46-53"""
    filenames = []
    for f in os.listdir(images_dir):
        ext = os.path.splitext(f)[1]
        if ext.lower() not in ext_list:
            continue
        filenames.append(f"{images_dir}/{f}")
    return filenames


def resize_bilinear(img, out_h, out_w):
    """tf.image.resize(img, (out_h, out_w)) default method (bilinear, antialias=False, half-pixel centres) for one
    HWC float32 image -- reference call site: inference.py:158.  fp32; host counterpart of y3_preprocess_image."""
    img = np.asarray(img, np.float32)
    in_h, in_w = img.shape[0], img.shape[1]

    def taps(n_in, n_out):
        scale = np.float32(n_in) / np.float32(n_out)
        src = (np.arange(n_out, dtype=np.float32) + np.float32(0.5)) * scale - np.float32(0.5)
        fl = np.floor(src)
        lo = np.maximum(fl, 0).astype(np.int64)
        hi = np.minimum(np.ceil(src), n_in - 1).astype(np.int64)
        return lo, hi, (src - fl).astype(np.float32)

    ylo, yhi, yfr = taps(in_h, out_h)
    xlo, xhi, xfr = taps(in_w, out_w)
    # TF's ResizeBilinear interpolates along x first (top and bottom rows), then along y
    top = img[ylo][:, xlo] + (img[ylo][:, xhi] - img[ylo][:, xlo]) * xfr[None, :, None]
    bot = img[yhi][:, xlo] + (img[yhi][:, xhi] - img[yhi][:, xlo]) * xfr[None, :, None]
    return (top + (bot - top) * yfr[:, None, None]).astype(np.float32)


def letterbox_geometry(h, w, target_height, target_width):
    """Where resize_image puts an h x w source on a (target_height, target_width) canvas: int32 [..., 4] =
    (sh, sw, top, left), the scaled size and its top-left corner.  Every operation in float32, as tf.image.resize(
    preserve_aspect_ratio=True) does it: scale = min(th / h, tw / w), sh = max(1, round-half-even(scale * h)), likewise
    sw; the padding is centred with the odd pixel after (floor).  The same formula in float64 gives another size for
    some sources, so the precision is part of the definition (the library: y3_letterbox_geometry).  h, w: scalars or
    arrays of one shape."""
    h, w = np.asarray(h), np.asarray(w)
    fh, fw = h.astype(np.float32), w.astype(np.float32)
    scale = np.minimum(np.float32(target_height) / fh, np.float32(target_width) / fw)
    sh = np.maximum(1, np.rint(scale * fh).astype(np.int64))
    sw = np.maximum(1, np.rint(scale * fw).astype(np.int64))
    top, left = (target_height - sh) // 2, (target_width - sw) // 2
    return np.stack([sh, sw, top, left], axis=-1).astype(np.int32)


def resize_image(img, target_height, target_width):
    """Aspect-preserving resize then centred zero padding to (target_height, target_width) -- reference
    core/utils.py:17-28 (tf.image.resize(preserve_aspect_ratio=True) + tf.image.pad_to_bounding_box).  `img` is one
    HWC image or an NHWC batch, float32.  Scaled size and position: letterbox_geometry."""
    img = np.asarray(img, np.float32)
    if img.ndim == 4:
        return np.stack([resize_image(i, target_height, target_width) for i in img])
    h, w = img.shape[0], img.shape[1]
    sh, sw, top, left = (int(v) for v in letterbox_geometry(h, w, target_height, target_width))
    scaled = img if (sh, sw) == (h, w) else resize_bilinear(img, sh, sw)   # same-size bilinear is the identity
    if top < 0 or left < 0 or top + sh > target_height or left + sw > target_width:
        raise ValueError("resize_image: scaled image does not fit the target")   # pad_to_bounding_box raises too
    out = np.zeros((target_height, target_width, img.shape[2]), np.float32)
    out[top:top + sh, left:left + sw] = scaled
    return out


def unletterbox_boxes(boxes, geometry, image_size):
    """Normalised (xmin, ymin, xmax, ymax) boxes on the padded canvas (image_size: an int S for S x S, or an (H, W)
    pair) -> normalised to the source frame that letterbox_geometry placed there; boxes [..., 4] float32, geometry
    (sh, sw, top, left).  float32, one rounding per operation: x' = (x * W - left) / sw, y' = (y * H - top) / sh; no
    clipping (the reference never clips boxes).  A geometry that is the whole canvas returns the values as they are
    (x * W / W is not x in float32).  Host restatement of y3_unletterbox_detections_hw."""
    boxes = np.asarray(boxes, np.float32)
    sh, sw, top, left = (int(v) for v in np.asarray(geometry).reshape(4))
    H, W = (int(image_size),) * 2 if np.ndim(image_size) == 0 else (int(v) for v in image_size)
    if (sh, sw, top, left) == (H, W, 0, 0):
        return boxes.copy()
    fs = np.array([W, H, W, H], np.float32)
    off = np.array([left, top, left, top], np.float32)
    div = np.array([sw, sh, sw, sh], np.float32)
    return ((boxes * fs - off) / div).astype(np.float32)


def load_image_rgb01(path):
    """tf.image.decode_image(bytes, channels=3, dtype=float32): RGB, alpha dropped, uint8/255 -> [0,1]
    (reference: inference.py:157)."""
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert("RGBA") if im.mode in ("RGBA", "LA", "P") else im.convert("RGB")
        a = np.asarray(im, np.uint8)[..., :3]
    return a.astype(np.float32) * np.float32(1.0 / 255.0)   # convert_image_dtype: cast * (1 / 255)


def load_image_u8(path):
    """RGB uint8 [H,W,3] (alpha dropped) for the GPU input stage (runtime.preprocess_image)."""
    from PIL import Image
    with Image.open(path) as im:
        im = im.convert("RGBA") if im.mode in ("RGBA", "LA", "P") else im.convert("RGB")
        return np.ascontiguousarray(np.asarray(im, np.uint8)[..., :3])
