"""The streaming pipelines of Net: frames in host memory -> detections (detect_stream) or evaluation results (evaluate_stream).
One loop (_detect_batches) stages batch i+1 while batch i is detected; what is done with a batch's packed rows is the caller's:
detect_stream copies them to a pinned ring, evaluate_stream hands them to its consumers (counters, loss, average precision),
which share one result buffer that is read back once.  Every function takes the net as its first argument; Net.detect_stream
and Net.evaluate_stream carry the documentation."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import ops
from ._args import _anchors, _dev, _fptr
from ._lib import Y3Error, check
from .input_stage import InputStage, TiledInputStage, packed_nbytes, tiles_arg, unletterbox_detections


def detect_stream(net, batches, anchors, max_boxes, iou_threshold, score_threshold, mode, depth, max_batch, max_blob_bytes, letterbox,
                  tiles=None, merge_iou_threshold=None):
    M = int(max_boxes)
    outs = {}       # ring slot -> pinned rows, pinned counts, event: made on the slot's first use
    pending = []
    truncated = _Truncated()

    def result(entry):
        k, n = entry
        packed_host, nv_host, done = outs[k]
        done.synchronize()      # an event wait: the next batch's detect is already queued behind this one
        return packed_host[:n].numpy().copy(), nv_host[:n].numpy().copy()

    for i, handle, packed_dev, nv_dev, cur, stage, _ in _detect_batches(
            net, "detect_stream", batches, anchors, M, iou_threshold, score_threshold, mode, depth, max_batch, max_blob_bytes, letterbox,
            tiles=tiles, merge_iou_threshold=merge_iou_threshold, truncated=truncated):
        k, n = i % stage.depth, handle.frames
        if k not in outs:
            outs[k] = (torch.empty((stage.max_batch, M, 7), dtype=torch.int32, pin_memory=True),
                       torch.empty((stage.max_batch,), dtype=torch.int32, pin_memory=True), torch.cuda.Event())
        packed_host, nv_host, done = outs[k]
        packed_host[:n].copy_(packed_dev[:n], non_blocking=True)
        nv_host[:n].copy_(nv_dev[:n], non_blocking=True)
        done.record(cur)
        pending.append((k, n))
        if len(pending) == stage.depth:     # its output buffers are the next to be reused
            yield result(pending.pop(0))
    while pending:
        yield result(pending.pop(0))
    if truncated.images():      # behind the last result: everything of the stream has run
        import warnings
        warnings.warn(f"detect_stream: {truncated.images()} image(s) had more multi-label candidates than the capacity "
                      f"{truncated.capacity} and were truncated (Net.multi_label_capacity; with tiles: tile images)", RuntimeWarning, stacklevel=2)


class _Truncated:
    """Multi-label streams: how many images had more candidates than the capacity.  One int64 on the device, added to behind every
    detect on the stream's own stream and read back once, when the stream is over."""

    def __init__(self):
        self.count, self.capacity, self._host = None, 0, None

    def enqueue(self, totals, capacity):
        if self.count is None:
            self.count, self.capacity = torch.zeros((), dtype=torch.int64, device=totals.device), int(capacity)
        self.count += (totals > int(capacity)).sum()

    def images(self):
        if self._host is None:
            self._host = 0 if self.count is None else int(self.count.item())
        return self._host


def _detect_batches(net, who, batches, anchors, M, iou_threshold, score_threshold, mode, depth, max_batch, max_blob_bytes,
                    letterbox, keep_grids=False, tiles=None, merge_iou_threshold=None, truncated=None):
    """The loop detect_stream and evaluate_stream share: a generator that stages batch i+1 on the InputStage's copy stream,
    enqueues y3_net_detect (and, with letterbox, y3_unletterbox_detections) of batch i on the current stream, and yields
    (i, handle, packed_dev, nv_dev, stream, stage, grids) for the consumer to enqueue its own work on `stream` behind them.
    The device buffers are slot i % depth of a ring: the consumer's reads are ordered before their reuse by the stream.
    keep_grids: the consumer wants the raw head grids as well (`grids`: three [n,g,g,3,5+nc] views, otherwise None), so
    each batch is one y3_net_detect_grids -- y3_net_detect that writes the grids, bit-identical detections -- into grid
    buffers made once here.
    tiles = (rows, cols, overlap_px, overview): sliced inference.  The stage cuts every frame into T windows from the one upload, the
    net is planned for max_batch * T tile images, y3_net_detect runs on the tile batch in the net's NMS mode into a ring of its own, and
    y3_merge_tile_detections (the same mode, merge_iou_threshold, by default iou_threshold) takes the place of
    y3_unletterbox_detections: what is yielded is per FRAME and in frame coordinates, with the shapes of the untiled route.
    tiles=None enqueues exactly what it did before the argument existed.
    net.multi_label (read here, when the stream starts): y3_net_detect[_grids] runs its multi-label route by itself -- with tiles on every
    tile image, the merge consuming the packed rows unchanged.  Behind every detect the totals are compared with the capacity on the
    device and counted into `truncated` (a _Truncated): no copy to the host, no synchronisation."""
    T = 1
    if tiles is not None:
        if keep_grids:
            raise Y3Error(f"{who}: loss=True cannot be combined with tiles (the ground truth is not mapped onto the windows)")
        tiles, T = tiles_arg(who, tiles)
        merge_iou = float(iou_threshold if merge_iou_threshold is None else merge_iou_threshold)
    elif merge_iou_threshold is not None:
        raise Y3Error(f"{who}: merge_iou_threshold needs tiles")
    if max_batch is None or max_blob_bytes is None:
        if not isinstance(batches, (list, tuple)):
            raise Y3Error(f"{who}: pass max_batch and max_blob_bytes when `batches` is not a list or tuple")
        if max_batch is None:
            max_batch = max((len(b) for b in batches), default=0)
        if max_blob_bytes is None:
            max_blob_bytes = max((packed_nbytes(b) for b in batches), default=0)
    S = net.image_size
    if net.canvas[0] <= 0:
        raise Y3Error(f"{who}: plan() the net first (the image size is the plan's)")
    if depth < 2:
        raise Y3Error(f"{who}: depth must be at least 2 (batch i+1 is staged while batch i is detected)")
    if max_batch < 1:
        return
    stage = (InputStage(S, max_batch, max(int(max_blob_bytes), 16), depth) if tiles is None else
             TiledInputStage(S, max_batch, max(int(max_blob_bytes), 16), tiles, depth))
    if max_batch * T > net.max_batch:
        net.plan(max_batch * T, S)
    a = _anchors(anchors, reshape=True, scales=net.heads)
    dev = stage.device
    ring = [(torch.empty((max_batch, M, 7), dtype=torch.int32, device=dev),
             torch.empty((max_batch,), dtype=torch.int32, device=dev)) for _ in range(stage.depth)]
    if tiles is not None:       # the tiles' rows, and the workspace of the merge: one of each, all of it runs on the one stream
        tile_packed = torch.empty((max_batch * T, M, 7), dtype=torch.int32, device=dev)
        tile_nv = torch.empty((max_batch * T,), dtype=torch.int32, device=dev)
        merge_ws = torch.empty(max(ops.merge_tiles_workspace_bytes(max_batch, T, M), 16), dtype=torch.uint8, device=dev)
    if keep_grids:
        nc, gs = net.program.nclasses, net._grid_hw()
        if nc <= 0:
            raise Y3Error(f"{who}: the program has no detection heads")
        grid_bufs = [torch.empty((max_batch, gh, gw, 3, 5 + nc), dtype=torch.float32, device=dev) for gh, gw in gs]
        grid_ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in grid_bufs])
    multi = bool(net.multi_label)
    if multi:       # a capacity above the boxes of the plan: the detect refuses it
        K = net.multi_label_capacity or sum(3 * gh * gw for gh, gw in net._grid_hw())
        totals_dev = torch.empty((max_batch * T,), dtype=torch.int32, device=dev)
    it = iter(batches)
    first = next(it, None)
    handle = stage.submit(first, mode, letterbox) if first is not None else None
    i = 0
    while handle is not None:
        nxt = next(it, None)
        following = stage.submit(nxt, mode, letterbox) if nxt is not None else None   # batch i+1 goes in before detect of batch i
        cur = torch.cuda.current_stream()
        cur.wait_event(handle.ready)
        n = handle.batch.shape[0]
        packed_dev, nv_dev = ring[i % stage.depth]
        sp, grids = C.c_void_p(cur.cuda_stream), None
        # the tiles' rows go to the merge, an untiled batch's straight into the ring
        out, out_nv = (tile_packed, tile_nv) if tiles is not None else (packed_dev, nv_dev)
        if keep_grids:      # the first n images of every buffer are a contiguous prefix
            grids = [t[:n] for t in grid_bufs]
            check(net.lib.y3_net_detect_grids(net._h, _dev(handle.batch), n, _fptr(a), M, float(iou_threshold), float(score_threshold),
                                              grid_ptrs, _dev(out), _dev(out_nv), sp), "y3_net_detect_grids")
        else:
            check(net.lib.y3_net_detect(net._h, _dev(handle.batch), n, _fptr(a), M, float(iou_threshold),
                                        float(score_threshold), _dev(out), _dev(out_nv), sp), "y3_net_detect")
        if multi:
            check(net.lib.y3_net_read_multi_label_totals(net._h, n, _dev(totals_dev), sp), "y3_net_read_multi_label_totals")
            if truncated is not None:
                truncated.enqueue(totals_dev[:n], K)
        stage.release(handle)
        if tiles is not None:
            f = handle.frames
            ops.merge_tile_detections(tile_packed[:n], tile_nv[:n], handle.windows, handle.geometry, handle.frame_hw, net.canvas,
                                      merge_iou, score_threshold, per_class=net.nms_per_class, out=(packed_dev[:f], nv_dev[:f]),
                                      ws=merge_ws, lib=net.lib)
        elif letterbox:
            unletterbox_detections(packed_dev[:n], nv_dev[:n], handle.geometry, net.canvas)
        yield i, handle, packed_dev, nv_dev, cur, stage, grids
        handle, i = following, i + 1


class _GroundTruthRing:
    """The ground truth of a batch, host lists -> device views: per ring slot the pinned words, their device copy and the
    "copied" event, made on the slot's first use and waited on before the slot's pinned words are written again."""

    def __init__(self, max_gt):
        self.G, self.slots = max_gt, {}

    def upload(self, k, gt, stage, stream):
        """-> (boxes [n,G,4] float32, classes [n,G] int32, count [n] int32) on the device, ordered on `stream`."""
        n, G = len(gt), self.G
        if k not in self.slots:
            words = stage.max_batch * (G * 5 + 1)
            self.slots[k] = [torch.empty(words, dtype=torch.int32, pin_memory=True),
                             torch.empty(words, dtype=torch.int32, device=stage.device), torch.cuda.Event(), False]
        pinned, gt_dev, copied, used = self.slots[k]
        if used:
            copied.synchronize()      # the slot's earlier copy (depth batches ago) has left the pinned words
        boxes_w, classes_w, count_w = ops._gt_views(pinned.numpy(), n, G)
        ops.pack_ground_truth(gt, G, out=(boxes_w.view(np.float32), classes_w, count_w))
        words = n * (G * 5 + 1)
        gt_dev[:words].copy_(pinned[:words], non_blocking=True)
        copied.record(stream)
        self.slots[k][3] = True
        boxes_d, classes_d, count_d = ops._gt_views(gt_dev, n, G)
        return boxes_d.view(torch.float32), classes_d, count_d


# The consumers of evaluate_stream.  Each owns `words` 64-bit words of the one result buffer; enqueue(out, ...) puts its work for
# one batch on the current stream, `out` being its words on the device; result(words) turns their final read-back into its part of
# the return value.

class _Counters:
    """The threshold counters of y3_evaluate_detections, one [T, 5*nc + 2] block per variant (plain / one-class)."""

    def __init__(self, nc, thresholds, iou_threshold, variants, both):
        self.nc, self.thr, self.iou, self.variants, self.both = nc, np.asarray(thresholds, np.float32), iou_threshold, variants, both
        self.shape = (len(variants), len(thresholds), 5 * nc + 2)
        self.words = int(np.prod(self.shape))

    def enqueue(self, out, packed, nv, gt, grids):
        for oc, counters in zip(self.variants, out.view(self.shape)):
            ops.evaluate_detections(packed, nv, *gt, self.nc, self.iou, self.thr, oc, counters=counters)

    def result(self, words):
        out = words.reshape(self.shape)
        return (out[0], out[1]) if self.both else out[0]


class _AveragePrecision:
    """The records of y3_match_detections, one tensor per batch kept on the device; its nc + 2 ground-truth totals are the words."""

    def __init__(self, net, nc, M, iou_thresholds, one_class):
        self.net, self.nc, self.M, self.thr, self.one_class, self.records = net, nc, M, iou_thresholds, one_class, []
        self.words = nc + 2

    def enqueue(self, out, packed, nv, gt, grids):
        self.records.append(torch.empty((packed.shape[0], self.M, 2), dtype=torch.int32, device=packed.device))
        ops._match(packed, nv, *gt, self.nc, self.thr, self.one_class, self.records[-1], out, lib=self.net.lib)

    def result(self, words):
        from .evaluate_detections import average_precision
        rec = torch.cat(self.records).cpu().numpy() if self.records else np.zeros((0, self.M, 2), np.int32)   # behind the one read-back
        return average_precision(rec.view(np.uint32), words, self.nc, len(self.thr))


class _Loss:
    """The validation loss: the [3,4] float64 sums of y3_yolo_loss over the images counted, then the images counted and the errors."""
    words = 14

    def __init__(self, net, anchors, nc):
        self.a, self.nc, self.gs = anchors, nc, [g for g, _ in net._grid_hw()]

    def allocate(self, max_batch, max_gt, device):
        """The scratch of the largest batch (cells of y3_yolo_assign_targets, per-image sums), made once with the result buffer."""
        self.cells = torch.empty((max_batch, max_gt), dtype=torch.int32, device=device)
        self.loss = torch.empty((max_batch, 3, 4), dtype=torch.float64, device=device)

    def enqueue(self, out, packed, nv, gt, grids):
        n = packed.shape[0]
        boxes, classes, count = gt
        cells, loss = self.cells[:n], self.loss[:n]
        ops.assign_targets(boxes, classes, count, self.a, self.gs, self.nc, cells=cells)
        ops.yolo_loss(grids, self.a, self.nc, boxes, classes, cells, loss=loss)
        loss_sum, loss_images = out[:12].view(torch.float64).view(3, 4), out[12:]
        loss_sum += loss.sum(dim=0)
        bad = (cells[:, 0] == -3).sum()
        loss_images += torch.stack([n - bad, bad])

    def result(self, words):
        return {"sum": words[:12].view(np.float64).reshape(3, 4).copy(), "images": int(words[12]), "errors": int(words[13])}


def evaluate_stream(net, batches, gts, anchors, max_boxes, iou_threshold, score_thresholds, nclasses, evaluate_iou_threshold,
                    one_class, mode, depth, max_batch, max_blob_bytes, letterbox, max_gt, loss, ap, tiles=None, merge_iou_threshold=None):
    thresholds = [float(t) for t in score_thresholds]
    ap_thr = None if ap is None or ap is False else ops.ap_iou_thresholds(ap)
    if loss and net.heads != 3:
        raise Y3Error(f"evaluate_stream: loss=True needs a three-head net (this one has {net.heads}; "
                      "y3_yolo_assign_targets / y3_yolo_loss are three-scale)")
    if loss and letterbox:
        raise Y3Error("evaluate_stream: loss=True cannot be combined with letterbox=True (the ground truth is not mapped onto the canvas)")
    if loss and tiles is not None:
        raise Y3Error("evaluate_stream: loss=True cannot be combined with tiles (the ground truth is not mapped onto the windows)")
    if loss and net.canvas[0] != net.canvas[1]:
        raise ValueError(f"evaluate_stream: loss=True needs a square plan (the net is planned for {net.canvas[0]} x {net.canvas[1]}; "
                         "the loss kernels take one grid size per scale)")
    if loss and int(nclasses) != net.program.nclasses:
        raise Y3Error(f"evaluate_stream: loss=True needs nclasses = {net.program.nclasses}, the program's (got {int(nclasses)})")
    both = isinstance(one_class, str)
    if both and one_class != "both":
        raise Y3Error('evaluate_stream: one_class must be False, True or "both"')
    if not 1 <= len(thresholds) <= 16:
        raise Y3Error("evaluate_stream: 1 to 16 score thresholds")
    if max_gt is None:
        if not isinstance(gts, (list, tuple)):
            raise Y3Error("evaluate_stream: pass max_gt when `gts` is not a list or tuple")
        G = max((len(np.asarray(c).reshape(-1)) for g in gts for _, c in g), default=0) or 1
    else:
        G = int(max_gt)
    gt_iter, missing = iter(gts), object()
    nc, M = int(nclasses), int(max_boxes)
    variants = (0, 1) if both else (int(bool(one_class)),)
    a = _anchors(anchors, reshape=True) if loss else None      # the loss's own copy (three scales); the detect takes the net's head count
    counted = _Counters(nc, thresholds, evaluate_iou_threshold, variants, both)
    matched = _AveragePrecision(net, nc, M, ap_thr, variants[0]) if ap_thr is not None else None
    summed = _Loss(net, a, nc) if loss else None
    consumers = [c for c in (counted, matched, summed) if c is not None]     # in the order their launches go out per batch
    part, total = {}, 0       # the layout of the one result buffer: each consumer's words, back to back
    for c in consumers:
        part[c], total = slice(total, total + c.words), total + c.words
    gt_ring, result, truncated = _GroundTruthRing(G), None, _Truncated()
    for i, handle, packed_dev, nv_dev, cur, stage, grids in _detect_batches(
            net, "evaluate_stream", batches, anchors, M, iou_threshold, min(thresholds), mode, depth, max_batch, max_blob_bytes, letterbox,
            keep_grids=bool(loss), tiles=tiles, merge_iou_threshold=merge_iou_threshold, truncated=truncated):
        n = handle.frames
        gt = next(gt_iter, missing)
        if gt is missing:
            raise Y3Error(f"evaluate_stream: `gts` ends before batch {i}")
        gt = list(gt)
        if len(gt) != n:
            raise Y3Error(f"evaluate_stream: batch {i} has {n} frames, its ground truth {len(gt)} entries")
        if result is None:      # 64-bit words, zeroed once and read back once
            result = torch.zeros(total, dtype=torch.int64, device=stage.device)
            if summed is not None:
                summed.allocate(stage.max_batch, G, stage.device)
        gt_dev = gt_ring.upload(i % stage.depth, gt, stage, cur)
        packed, nv = packed_dev[:n], nv_dev[:n]
        for c in consumers:
            c.enqueue(result[part[c]], packed, nv, gt_dev, grids)
    if next(gt_iter, missing) is not missing:
        raise Y3Error("evaluate_stream: `gts` has more entries than there are batches")
    words = np.zeros(total, np.int64) if result is None else result.cpu().numpy()      # the one read-back: waits for the stream
    if truncated.images():      # the one-pass argument (every threshold from the detect at the lowest) does not hold for a truncated image
        raise Y3Error(f"evaluate_stream: {truncated.images()} image(s) had more multi-label candidates than the capacity {truncated.capacity} "
                      "at the lowest score threshold; raise Net.multi_label_capacity (0: every box of the plan) or the lowest threshold")
    ret = [c.result(words[part[c]]) for c in (counted, summed, matched) if c is not None]      # the order of the return value
    return ret[0] if len(ret) == 1 else tuple(ret)
