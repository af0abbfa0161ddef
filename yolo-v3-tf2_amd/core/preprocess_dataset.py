"""Host restatement of the label assignment of reference core/preprocess_dataset.py:19-92 in NumPy, with the reference's names:
`PreprocessDataset._arrange_in_grid` makes the dense label grid of one scale, `assign_targets` is the sparse form the library
computes on the GPU (include/y3.h, y3_yolo_assign_targets): one decode-row index per ground-truth row instead of a grid.
All arithmetic is float32 with every operation rounded on its own; both forms share `_best_anchors` and `_cells`."""
import numpy as np


def _best_anchors(boxes, anchors):
    """boxes [...,4] float32, anchors [3,3,2] -> the index 0..8 of the anchor with the first maximum width/height IoU (reference
    _find_max_iou_anchors, lines 35-48).  First maximum: anchor 0, then a later anchor only when strictly greater, so a NaN
    never wins -- the rule of the kernel, written out because np.argmax and tf.argmax treat a NaN differently."""
    boxes = np.asarray(boxes, np.float32)
    a = np.asarray(anchors, np.float32).reshape(-1, 2)
    w, h = boxes[..., 2] - boxes[..., 0], boxes[..., 3] - boxes[..., 1]
    best = np.zeros(w.shape, np.int32)
    best_iou = None
    with np.errstate(all="ignore"):
        for k in range(len(a)):
            inter = np.minimum(w, a[k, 0]) * np.minimum(h, a[k, 1])
            iou = inter / ((w * h + a[k, 0] * a[k, 1]) - inter)
            if best_iou is None:
                best_iou = iou
            else:
                take = iou > best_iou
                best = np.where(take, np.int32(k), best)
                best_iou = np.where(take, iou, best_iou)
    return best


def _cells(boxes, grid_size):
    """-> (row, col, inside): tf.cast(centre * grid, int32) of lines 21-26 (truncation toward zero), and whether the cell lies in
    [0, grid) -- exactly when -1 < centre * grid < grid, which is false for a NaN.  row / col are 0 where not inside."""
    boxes = np.asarray(boxes, np.float32)
    g = np.float32(grid_size)
    with np.errstate(all="ignore"):
        fx = ((boxes[..., 0] + boxes[..., 2]) / np.float32(2)) * g
        fy = ((boxes[..., 1] + boxes[..., 3]) / np.float32(2)) * g
        inside = (fx > -1) & (fx < g) & (fy > -1) & (fy < g)
    col = np.where(inside, np.trunc(np.where(inside, fx, 0)), 0).astype(np.int32)
    row = np.where(inside, np.trunc(np.where(inside, fy, 0)), 0).astype(np.int32)
    return row, col, inside


class PreprocessDataset:
    """reference: core/preprocess_dataset.py:17-92 (the tf.data plumbing of __call__ is not restated: the library reads its data
    set through core/load_tfrecords.py)."""

    def _find_max_iou_anchors(self, bboxes, anchors):
        return _best_anchors(np.asarray(bboxes, np.float32)[..., 0:4], anchors)

    def _arrange_in_grid(self, y_train, anchors, grid_index, output_shape, max_bboxes):
        """y_train [B,max_bboxes,6] = (xmin, ymin, xmax, ymax, obj, class), anchors [3,3,2], output_shape [B,g,g,3,6] -> the
        dense label grid of scale `grid_index`: the rows with obj != 0 whose best anchor belongs to this scale, scattered to
        (image, row, col, anchor) in order, so that a later row replaces an earlier one on the same cell
        (tensor_scatter_nd_update on the CPU).  A cell outside the grid raises IndexError, as the reference's scatter raises."""
        y_train = np.asarray(y_train, np.float32)
        anchors = np.asarray(anchors, np.float32)
        B, g = int(output_shape[0]), int(output_shape[1])
        assert y_train.shape[:2] == (B, max_bboxes) and anchors.shape[0] * anchors.shape[1] == 9
        best = self._find_max_iou_anchors(y_train, anchors)
        row, col, inside = _cells(y_train[..., 0:4], g)
        # histogram_fixed_width_bins over [0, 9) in 3 bins of the anchor index is best // 3
        mask = (y_train[..., 4] != 0) & (best // anchors.shape[1] == grid_index)
        out = np.zeros(tuple(int(v) for v in output_shape), np.float32)
        for b, r in zip(*np.nonzero(mask)):
            if not inside[b, r]:
                raise IndexError(f"_arrange_in_grid: image {b} row {r} falls outside the {g} x {g} grid")
            out[b, row[b, r], col[b, r], best[b, r] % anchors.shape[1]] = y_train[b, r]
        return out


def assign_targets(gt_boxes, gt_classes, gt_count, anchors, grid_sizes, nclasses):
    """Ground truth as runtime.pack_ground_truth lays it out (gt_boxes [B,G,4] float32, gt_classes [B,G] int32, gt_count [B]) ->
    cells [B,G] int32, what y3_yolo_assign_targets writes, bit for bit: per row r < count the row's index in decode's row order
    n = 3 sum_{t<s} g_t^2 + (row g_s + col) 3 + a; -1 for r >= count; -2 for a row whose cell a later row took; -3 for every
    row r < count of an error image (a non-finite coordinate, a class outside [0,nclasses), a cell outside its grid)."""
    gt_boxes = np.asarray(gt_boxes, np.float32)
    gt_classes = np.asarray(gt_classes)
    B, G = gt_classes.shape
    count = np.clip(np.asarray(gt_count).astype(np.int64), 0, G)
    live = np.arange(G)[None, :] < count[:, None]
    best = _best_anchors(gt_boxes, anchors)
    s, a = best // 3, best % 3
    offsets = np.concatenate([[0], np.cumsum([3 * int(g) * int(g) for g in grid_sizes])]).astype(np.int64)
    key = np.zeros((B, G), np.int64)
    ok = np.isfinite(gt_boxes).all(-1) & (gt_classes >= 0) & (gt_classes < nclasses)
    inside = np.zeros((B, G), bool)
    for k, g in enumerate(grid_sizes):
        row, col, ins = _cells(gt_boxes, g)
        pick = s == k
        key = np.where(pick, offsets[k] + (row.astype(np.int64) * int(g) + col) * 3 + a, key)
        inside = np.where(pick, ins, inside)
    ok &= inside
    cells = np.full((B, G), -1, np.int32)
    for b in range(B):
        n = int(count[b])
        if not ok[b, :n].all():
            cells[b, :n] = -3
            continue
        k = key[b, :n]
        last = {int(v): r for r, v in enumerate(k)}          # the highest row index on each cell
        cells[b, :n] = [int(v) if last[int(v)] == r else -2 for r, v in enumerate(k)]
    assert not (live & (cells == -1)).any()
    return cells
