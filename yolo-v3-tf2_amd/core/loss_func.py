"""Host restatement of reference core/loss_func.py:19-69 in NumPy, with the reference's names: `get_loss_func(anchors, nclasses)`
returns `yolo_loss(y_true, y_pred)` on the dense label grid of one scale; `loss_from_cells` is the sparse form the library
computes on the GPU (include/y3.h, y3_yolo_loss) with its per-image [B,3,4] layout.  TensorFlow is not a dependency: the Keras /
TF operators (TF 2.8.1, Keras 2.8.0) are written out -- binary_crossentropy and sparse_categorical_crossentropy on probabilities
clip to [epsilon, 1 - epsilon] and take logarithms; the latter hands log(p) to sparse_softmax_cross_entropy_with_logits.

Every term is computed in `dtype` (float32: the reference's and the kernel's precision) with each operation rounded on its own,
by the `_terms_*` helpers both forms share; the terms are then summed in float64.  This is the validation loss only: no gradient
exists here, and the regulariser the reference adds (model.losses, decay_factor) is not part of any number below."""
import numpy as np

EPSILON = np.float32(1e-7)                    # keras.backend.epsilon()
ONE_MINUS_EPSILON = np.float32(1.0) - EPSILON


def _sigmoid(x):
    one = x.dtype.type(1)
    with np.errstate(over="ignore"):
        return one / (one + np.exp(-x))


def _clip(p):
    return np.minimum(np.maximum(p, p.dtype.type(EPSILON)), p.dtype.type(ONE_MINUS_EPSILON))


def _terms_obj(logit, target):
    """binary_crossentropy(true_obj, sigmoid(logit)) over a last axis of one element: -(t log(p + eps) + (1 - t) log(1 - p + eps))
    with p clipped; target is 0 or 1, so one product is 0 * finite and the term is one of the two logarithms."""
    T = logit.dtype.type
    p = _clip(_sigmoid(logit))
    t = target.astype(logit.dtype)
    return -(t * np.log(p + T(EPSILON)) + (T(1) - t) * np.log((T(1) - p) + T(EPSILON)))


def _terms_box(logits, boxes, col, row, grid_size, anchor_wh):
    """-> (xy, wh) terms of rows with a label: logits [...,4+], boxes [...,4], col / row the cell, anchor_wh [...,2]."""
    T = logits.dtype.type
    tw, th = boxes[..., 2] - boxes[..., 0], boxes[..., 3] - boxes[..., 1]
    scale = T(2) - tw * th
    g = T(grid_size)
    tx = ((boxes[..., 0] + boxes[..., 2]) / T(2)) * g - col.astype(logits.dtype)
    ty = ((boxes[..., 1] + boxes[..., 3]) / T(2)) * g - row.astype(logits.dtype)
    dx, dy = tx - _sigmoid(logits[..., 0]), ty - _sigmoid(logits[..., 1])
    xy = scale * (dx * dx + dy * dy)
    with np.errstate(divide="ignore", invalid="ignore"):
        lw, lh = np.log(tw / anchor_wh[..., 0]), np.log(th / anchor_wh[..., 1])
    lw, lh = np.where(np.isinf(lw), T(0), lw), np.where(np.isinf(lh), T(0), lh)      # tf.where(is_inf): a NaN stays
    dw, dh = lw - logits[..., 2], lh - logits[..., 3]
    return xy, scale * (dw * dw + dh * dh)


def _terms_class(class_logits, classes):
    """sparse_categorical_crossentropy(classes, sigmoid(class_logits)): rows [R,nc], classes [R] -> [R]."""
    l = np.log(_clip(_sigmoid(class_logits)))
    m = l.max(axis=-1)
    lc = np.take_along_axis(l, classes.astype(np.int64)[:, None], axis=-1)[:, 0]
    return np.log(np.exp(l - m[:, None]).sum(axis=-1, dtype=l.dtype)) - (lc - m)


def get_loss_func(anchors, nclasses, eager_mode=True, dtype=np.float32):
    """anchors [3,2]: the anchors of the scale.  -> yolo_loss(y_true [B,g,g,3,6], y_pred [B,g,g,3,5+nclasses]): float64
    [xy, wh, obj, class] summed over the batch and the grid (eager_mode, reference line 65) or their sum.  The label grid is
    what PreprocessDataset._arrange_in_grid makes: (xmin, ymin, xmax, ymax, obj, class) per cell and anchor, zeros elsewhere."""
    anchors = np.asarray(anchors, dtype).reshape(3, 2)

    def yolo_loss(y_true, y_pred):
        y_true, y_pred = np.asarray(y_true, dtype), np.asarray(y_pred, dtype)
        B, g = y_true.shape[0], y_true.shape[1]
        col, row = np.meshgrid(np.arange(g), np.arange(g))                 # grid[..., 0] = col, grid[..., 1] = row
        col = np.broadcast_to(col[None, :, :, None], (B, g, g, 3))
        row = np.broadcast_to(row[None, :, :, None], (B, g, g, 3))
        obj_mask = y_true[..., 4]
        xy, wh = _terms_box(y_pred, y_true[..., 0:4], col, row, g, np.broadcast_to(anchors, (B, g, g, 3, 2)))
        with np.errstate(invalid="ignore"):
            xy_loss, wh_loss = obj_mask * xy, obj_mask * wh
        obj_loss = _terms_obj(y_pred[..., 4], y_true[..., 4])
        cls = _terms_class(y_pred[..., 5:].reshape(-1, nclasses), y_true[..., 5].reshape(-1)).reshape(B, g, g, 3)
        class_loss = obj_mask * cls
        result = np.array([t.sum(dtype=np.float64) for t in (xy_loss, wh_loss, obj_loss, class_loss)])
        return result if eager_mode else result.sum()

    return yolo_loss


def loss_from_cells(grids, gt_boxes, gt_classes, cells, anchors, nclasses, dtype=np.float32):
    """grids: three arrays [B,g,g,3,5+nclasses]; ground truth as runtime.pack_ground_truth lays it out; cells [B,G] from
    core/preprocess_dataset.assign_targets; anchors [3,3,2] -> float64 [B,3,4]: per image and scale the sums xy, wh, obj, class
    (what y3_yolo_loss writes).  An image with a -3 in its cells is an error image and gets twelve zeros.  For a data set,
    sum over the images / images is the reference's per-batch `loss_fn(label, output) / batch_size` (train.py:39-54): val_loss is
    the sum of its 12 entries, perGrid its row sums, perSource[xy,wh,obj,class] its column sums -- without the regulariser.
    dtype=np.float64 computes the same terms in double precision (the yardstick for what float32 rounding is worth)."""
    anchors = np.asarray(anchors, dtype).reshape(3, 3, 2)
    gt_boxes = np.asarray(gt_boxes, np.float32).astype(dtype)
    gt_classes, cells = np.asarray(gt_classes), np.asarray(cells)
    B = cells.shape[0]
    out = np.zeros((B, 3, 4), np.float64)
    off = 0
    for s, grid in enumerate(grids):
        grid = np.asarray(grid, np.float32).astype(dtype)
        g = grid.shape[1]
        rows = 3 * g * g
        flat = grid.reshape(B, rows, 5 + nclasses)
        for b in range(B):
            if (cells[b] == -3).any():
                continue
            r = np.nonzero((cells[b] >= off) & (cells[b] < off + rows))[0]
            n = cells[b, r] - off
            target = np.zeros(rows, dtype)
            target[n] = 1
            out[b, s, 2] = _terms_obj(flat[b, :, 4], target).sum(dtype=np.float64)
            if len(r):
                cell, a = n // 3, n % 3
                t = flat[b, n]
                xy, wh = _terms_box(t, gt_boxes[b, r], cell % g, cell // g, g, anchors[s][a])
                out[b, s, 0] = xy.sum(dtype=np.float64)
                out[b, s, 1] = wh.sum(dtype=np.float64)
                out[b, s, 3] = _terms_class(t[:, 5:], gt_classes[b, r]).sum(dtype=np.float64)
        off += rows
    return out


def summarize_loss(loss_sum, images):
    """float64 [3,4] summed over `images` images -> (val_loss, perGrid [3], perSource [4]) as train.py:45-52 forms them."""
    mean = np.asarray(loss_sum, np.float64) / max(int(images), 1)
    return float(mean.sum()), mean.sum(axis=1), mean.sum(axis=0)
