"""The stand-alone ops behind the network: decode, class scores, NMS and the packed rows, the evaluation counters and the AP
matching, target assignment and the validation loss, the plane-split helpers.  Torch tensors in, torch tensors out; each C entry
point named here is called from this one place.  The private forms with an `out` argument are what the streaming loops (stream.py)
write into their preallocated buffers with."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._args import _anchors, _dev, _fptr, _need_cuda
from ._lib import Y3Error, check


def _grids_args(grids, square=True):
    """square: the three-scale entry points' (ptrs, grid_sizes[3]); otherwise (ptrs, grid_hw[n][2]) of the n = 2 or 3 grids handed in,
    for the _n entry points."""
    _need_cuda(*grids)
    if len(grids) != 3 and (square or len(grids) != 2):
        raise Y3Error("expected three grids" if square else "expected two or three grids")
    for g in grids:
        if g.dtype != torch.float32 or g.dim() != 5 or g.shape[3] != 3 or (square and g.shape[1] != g.shape[2]):
            raise Y3Error("each grid must be float32 [B,g,g,3,5+nc]" if square else "each grid must be float32 [B,gh,gw,3,5+nc]")
    ptrs = (C.c_void_p * len(grids))(*[g.data_ptr() for g in grids])
    if square:
        gs = (C.c_int32 * 3)(*[g.shape[1] for g in grids])
    else:       # grid_hw[n][2] = {gh, gw}
        gs = (C.c_int32 * (2 * len(grids)))(*[v for g in grids for v in (g.shape[1], g.shape[2])])
    B = grids[0].shape[0]
    N = sum(3 * g.shape[1] * g.shape[2] for g in grids)
    return ptrs, gs, B, N


def yolo_decode(grids, anchors_table, nclasses):
    """-> (bboxes [B,N,4], confidence [B,N,1], class_probs [B,N,nc]).  Three grids [B,gh,gw,3,5+nc], or two (YOLOv3-tiny) with an
    anchors_table [2,3,2]: each centre is normalised by its own axis (include/y3.h, y3_yolo_decode_hw), which for gh == gw is the
    reference's arithmetic bit for bit."""
    ptrs, gs, B, N = _grids_args(grids, square=False)
    a = _anchors(anchors_table, scales=len(grids))
    dev = grids[0].device
    bboxes = torch.empty((B, N, 4), dtype=torch.float32, device=dev)
    conf = torch.empty((B, N, 1), dtype=torch.float32, device=dev)
    probs = torch.empty((B, N, nclasses), dtype=torch.float32, device=dev)
    check(_lib.load().y3_yolo_decode_hw_n(ptrs, gs, len(grids), B, nclasses, _fptr(a), _dev(bboxes), _dev(conf), _dev(probs),
                                     _lib.stream_ptr()), "y3_yolo_decode")
    return bboxes, conf, probs


def yolo_decode_scores(grids, anchors_table, nclasses):
    """fused decode + class arg-max/score -> (bboxes [B,N,4], class_indices [B,N] i64, scores [B,N])"""
    return _decode_scores(grids, anchors_table, nclasses)


def _decode_scores(grids, anchors_table, nclasses, out=None):
    ptrs, gs, B, N = _grids_args(grids, square=False)
    a = _anchors(anchors_table, scales=len(grids))
    dev = grids[0].device
    bboxes, cls, scores = out or (torch.empty((B, N, 4), dtype=torch.float32, device=dev),
                                  torch.empty((B, N), dtype=torch.int64, device=dev),
                                  torch.empty((B, N), dtype=torch.float32, device=dev))
    check(_lib.load().y3_yolo_decode_scores_hw_n(ptrs, gs, len(grids), B, nclasses, _fptr(a), _dev(bboxes), _dev(cls), _dev(scores),
                                            _lib.stream_ptr()), "y3_yolo_decode_scores")
    return bboxes, cls, scores


def maxpool2x2(x: torch.Tensor, stride: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MaxPooling2D(2, strides=stride, 'same') of x [B,H,W,C] (float32, bfloat16, float16 or int8, on the GPU) -> [B,H/stride,W/stride,C]
    (y3_maxpool2x2; maxpool.maxpool2x2_ref restates the rule).  stride 1 or 2, stride 2 on even H and W; C * element size a multiple
    of 16 bytes (int8: C % 16 == 0; every byte value is legal).  Enqueues on the current stream only."""
    _need_cuda(x, out)
    dt = {torch.float32: _lib.Y3_DTYPE_F32, torch.bfloat16: _lib.Y3_DTYPE_BF16, torch.float16: _lib.Y3_DTYPE_F16,
          torch.int8: _lib.Y3_DTYPE_I8}.get(x.dtype)
    if dt is None or x.dim() != 4:
        raise Y3Error("maxpool2x2: x must be float32, bfloat16, float16 or int8 [B,H,W,C]")
    if stride not in (1, 2):
        raise Y3Error(f"maxpool2x2: stride must be 1 or 2 (got {stride!r})")
    B, H, W, Cc = (int(v) for v in x.shape)
    if stride == 2 and (H % 2 or W % 2):
        raise Y3Error(f"maxpool2x2: a stride-2 pool needs even extents (got {H} x {W})")
    shape = (B, H // stride, W // stride, Cc)
    if out is None:
        out = torch.empty(shape, dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != x.dtype:
        raise Y3Error(f"maxpool2x2: out must be {x.dtype} {list(shape)}")
    check(_lib.load().y3_maxpool2x2(_dev(x), _dev(out), B, H, W, Cc, int(stride), dt, _lib.stream_ptr()), "y3_maxpool2x2")
    return out


def decode_candidates_workspace_bytes(grid_hw, batch: int, nclasses: int) -> int:
    """y3_decode_candidates_workspace_bytes_n: grid_hw = two or three (gh, gw) pairs; 0 for sizes decode_candidates refuses."""
    grid_hw = [tuple(hw) for hw in grid_hw]
    gs = (C.c_int32 * (2 * len(grid_hw)))(*[int(v) for hw in grid_hw for v in hw])
    return int(_lib.load().y3_decode_candidates_workspace_bytes_n(gs, len(grid_hw), int(batch), int(nclasses)))


def decode_candidates(grids, anchors_table, nclasses, score_threshold, capacity, out=None, ws=None):
    """Multi-label candidates (y3_yolo_decode_candidates_hw; host restatement: multilabel.candidates_ref over yolo_decode's arrays):
    every pair (box n, class c) with conf[n] * prob[n,c] > score_threshold, numbered per image in the order (n, c) ascending, the
    first `capacity` of them stored -> (cand_boxes [B,K,4] f32, cand_cls [B,K] i64, cand_scores [B,K] f32, cand_src [B,K] i32 = n,
    totals [B] i32, uncapped).  Rows behind min(total, K) are zero.  Grids [B,gh,gw,3,5+nc], square or rectangular.  out: the five
    tensors to write; ws: a uint8 workspace of decode_candidates_workspace_bytes (one is made otherwise).  Enqueues on the current
    stream only."""
    ptrs, gs, B, N = _grids_args(grids, square=False)
    a = _anchors(anchors_table, scales=len(grids))
    dev = grids[0].device
    K = int(capacity)
    if K < 1:
        raise Y3Error(f"decode_candidates: capacity must be at least 1 (got {K})")
    if out is None:
        out = (torch.empty((B, K, 4), dtype=torch.float32, device=dev), torch.empty((B, K), dtype=torch.int64, device=dev),
               torch.empty((B, K), dtype=torch.float32, device=dev), torch.empty((B, K), dtype=torch.int32, device=dev),
               torch.empty((B,), dtype=torch.int32, device=dev))
    boxes, cls, scores, src, totals = out
    _need_cuda(boxes, cls, scores, src, totals, ws)
    want = ((B, K, 4), torch.float32), ((B, K), torch.int64), ((B, K), torch.float32), ((B, K), torch.int32), ((B,), torch.int32)
    if any(tuple(t.shape) != s or t.dtype != d or not t.is_contiguous() for t, (s, d) in zip(out, want)):
        raise Y3Error(f"decode_candidates: out must be contiguous f32 [{B},{K},4], i64 [{B},{K}], f32 [{B},{K}], i32 [{B},{K}], i32 [{B}]")
    lib = _lib.load()
    if ws is None:
        ws = torch.empty(max(lib.y3_decode_candidates_workspace_bytes_n(gs, len(grids), B, int(nclasses)), 16), dtype=torch.uint8, device=dev)
    elif ws.dtype != torch.uint8 or ws.dim() != 1:
        raise Y3Error("ws must be a 1-D uint8 tensor")
    check(lib.y3_yolo_decode_candidates_hw_n(ptrs, gs, len(grids), B, int(nclasses), _fptr(a), float(score_threshold), K, _dev(boxes), _dev(cls),
                                           _dev(scores), _dev(src), _dev(totals), _dev(ws), ws.numel(), _lib.stream_ptr()),
          "y3_yolo_decode_candidates_hw")
    return boxes, cls, scores, src, totals


def class_candidates(bboxes, conf, probs, score_threshold, capacity):
    """decode_candidates for callers that hold the decoded tensors (y3_class_candidates), as class_scores is to yolo_decode_scores:
    bboxes [B,N,4], conf [B,N,1] or [B,N], probs [B,N,nc] as yolo_decode gives them -> the same five tensors, bit for bit those of
    decode_candidates on the grids they were decoded from."""
    _need_cuda(bboxes, conf, probs)
    if bboxes.dtype != torch.float32 or conf.dtype != torch.float32 or probs.dtype != torch.float32 or probs.dim() != 3:
        raise Y3Error("class_candidates: float32 bboxes [B,N,4], conf [B,N,1], probs [B,N,nc]")
    B, N, nc = probs.shape
    if bboxes.numel() != B * N * 4 or conf.numel() != B * N:
        raise Y3Error(f"class_candidates: bboxes must hold [{B},{N},4] and conf [{B},{N}] values")
    K, dev = int(capacity), probs.device
    if K < 1:
        raise Y3Error(f"class_candidates: capacity must be at least 1 (got {K})")
    out = (torch.empty((B, K, 4), dtype=torch.float32, device=dev), torch.empty((B, K), dtype=torch.int64, device=dev),
           torch.empty((B, K), dtype=torch.float32, device=dev), torch.empty((B, K), dtype=torch.int32, device=dev),
           torch.empty((B,), dtype=torch.int32, device=dev))
    ws = torch.empty(max(B * N * 4, 16), dtype=torch.uint8, device=dev)
    check(_lib.load().y3_class_candidates(_dev(bboxes), _dev(conf), _dev(probs), B, N, nc, float(score_threshold), K, *[_dev(t) for t in out],
                                          _dev(ws), ws.numel(), _lib.stream_ptr()), "y3_class_candidates")
    return out


def candidate_sources(packed: torch.Tensor, num_valid: torch.Tensor, cand_src: torch.Tensor):
    """The index word (word 6) of every valid packed row, in place: candidate k -> cand_src[b,k], the box it came from
    (y3_candidate_sources).  packed [B,M,7] int32 as pack_detections wrote it over the [B,K] candidates.  -> packed."""
    _need_cuda(packed, num_valid, cand_src)
    if packed.dtype != torch.int32 or packed.dim() != 3 or packed.shape[2] != 7 or not packed.is_contiguous():
        raise Y3Error("packed must be contiguous int32 [B,M,7]")
    B, M = packed.shape[0], packed.shape[1]
    if num_valid.dtype != torch.int32 or num_valid.shape != (B,) or cand_src.dtype != torch.int32 or cand_src.dim() != 2 or \
            cand_src.shape[0] != B or not cand_src.is_contiguous():
        raise Y3Error(f"num_valid must be int32 [{B}] and cand_src contiguous int32 [{B},K]")
    check(_lib.load().y3_candidate_sources(_dev(packed), _dev(num_valid), _dev(cand_src), B, cand_src.shape[1], M, _lib.stream_ptr()),
          "y3_candidate_sources")
    return packed


def class_scores(conf, probs):
    _need_cuda(conf, probs)
    B, N, nc = probs.shape
    cls = torch.empty((B, N), dtype=torch.int64, device=probs.device)
    scores = torch.empty((B, N), dtype=torch.float32, device=probs.device)
    check(_lib.load().y3_class_scores(_dev(conf), _dev(probs), B, N, nc, _dev(cls), _dev(scores), _lib.stream_ptr()),
          "y3_class_scores")
    return cls, scores


def split3_planes(x: torch.Tensor) -> torch.Tensor:
    """fp32 [...,C] -> bf16 [...,3,C] with hi + mid + lo == x exactly (the activation format of Y3_DTYPE_F32X3)."""
    hi = x.to(torch.bfloat16)
    r1 = x - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    return torch.stack([hi, mid, lo], dim=-2).contiguous()


def split2_planes(x: torch.Tensor) -> torch.Tensor:
    """fp32 [...,C] -> fp16 [...,2,C]: h = fp16(x), l' = fp16((x - h) * 2^11), x == h + l' * 2^-11 up to 2^-22 |x|
    (the activation format of Y3_DTYPE_F32X2)."""
    h = x.to(torch.float16)
    lo = ((x - h.float()) * 2048.0).to(torch.float16)
    return torch.stack([h, lo], dim=-2).contiguous()


def pack_ground_truth(gts, max_gt: Optional[int] = None, out=None):
    """A list of per-image (boxes [g,4], classes [g]) -> padded (boxes [B,G,4] float32, classes [B,G] int32, count [B] int32),
    the ground-truth form of evaluate_detections.  Pure NumPy.  G = max_gt, by default the largest g of the list (at least 1);
    an image with more rows than max_gt raises.  out: the three arrays to fill (e.g. views of pinned memory); rows behind
    an image's count are zeroed."""
    gts = [(np.asarray(b, np.float32).reshape(-1, 4), np.asarray(c).reshape(-1)) for b, c in gts]
    for i, (b, c) in enumerate(gts):
        if len(b) != len(c):
            raise Y3Error(f"pack_ground_truth: image {i} has {len(b)} boxes and {len(c)} classes")
    most = max((len(c) for _, c in gts), default=0)
    G = max(most, 1) if max_gt is None else int(max_gt)
    if G < 1 or most > G:
        raise Y3Error(f"pack_ground_truth: max_gt = {G}, the images hold up to {most} boxes")
    B = len(gts)
    if out is None:
        out = (np.empty((B, G, 4), np.float32), np.empty((B, G), np.int32), np.empty((B,), np.int32))
    boxes, classes, count = out
    if (boxes.shape, classes.shape, count.shape) != ((B, G, 4), (B, G), (B,)) or \
            (boxes.dtype, classes.dtype, count.dtype) != (np.float32, np.int32, np.int32):
        raise Y3Error(f"pack_ground_truth: out must be float32 [{B},{G},4], int32 [{B},{G}], int32 [{B}]")
    boxes[...] = 0
    classes[...] = 0
    for i, (b, c) in enumerate(gts):
        boxes[i, :len(b)] = b
        classes[i, :len(c)] = c
        count[i] = len(c)
    return boxes, classes, count


def _gt_views(words, n: int, G: int):
    """A 1-D int32 buffer (NumPy or torch) -> its (boxes [n,G,4], classes [n,G], count [n]) parts, boxes still as words."""
    nb, ncl = n * G * 4, n * G
    return words[:nb].reshape(n, G, 4), words[nb:nb + ncl].reshape(n, G), words[nb + ncl:nb + ncl + n]


def _scored_args(packed, num_valid, gt_boxes, gt_classes, gt_count):
    """The checks evaluate_detections and match_detections share -> (B, M, G)."""
    if packed.dtype != torch.int32 or packed.dim() != 3 or packed.shape[2] != 7:
        raise Y3Error("packed must be contiguous int32 [B,M,7]")
    B, M = packed.shape[0], packed.shape[1]
    if num_valid.dtype != torch.int32 or num_valid.shape != (B,):
        raise Y3Error(f"num_valid must be int32 [{B}]")
    if gt_boxes.dtype != torch.float32 or gt_boxes.dim() != 3 or gt_boxes.shape[0] != B or gt_boxes.shape[2] != 4:
        raise Y3Error(f"gt_boxes must be float32 [{B},G,4]")
    G = gt_boxes.shape[1]
    if gt_classes.dtype != torch.int32 or gt_classes.shape != (B, G):
        raise Y3Error(f"gt_classes must be int32 [{B},{G}]")
    if gt_count.dtype != torch.int32 or gt_count.shape != (B,):
        raise Y3Error(f"gt_count must be int32 [{B}]")
    return B, M, G


def evaluate_detections(packed: torch.Tensor, num_valid: torch.Tensor, gt_boxes: torch.Tensor, gt_classes: torch.Tensor,
                        gt_count: torch.Tensor, nclasses: int, iou_threshold: float, score_thresholds, one_class=False,
                        counters: Optional[torch.Tensor] = None):
    """packed [B,M,7] int32 words and num_valid [B] int32 on the GPU (Net.detect at the LOWEST threshold of the sweep,
    pack_detections, unletterbox_detections), ground truth on the GPU as pack_ground_truth lays it out (gt_boxes [B,G,4]
    float32, gt_classes [B,G] int32, gt_count [B] int32) -> the counters of every score threshold, int64
    [T, 5*nclasses + 2] on the GPU: preds, gts, tp, fp, fn (each [nclasses]), errors, examples per threshold
    (y3_evaluate_detections; host restatement: evaluate_detections.sweep_counters).  counters=None: a zeroed tensor is
    made; otherwise the call ADDS to the one given.  Enqueues on the current stream only."""
    _need_cuda(packed, num_valid, gt_boxes, gt_classes, gt_count, counters)
    B, M, G = _scored_args(packed, num_valid, gt_boxes, gt_classes, gt_count)
    thr = np.ascontiguousarray(np.asarray(score_thresholds, np.float32).reshape(-1))
    nc = int(nclasses)
    if counters is None:
        counters = torch.zeros((len(thr), 5 * nc + 2), dtype=torch.int64, device=packed.device)
    elif counters.dtype != torch.int64 or counters.shape != (len(thr), 5 * nc + 2):
        raise Y3Error(f"counters must be int64 [{len(thr)},{5 * nc + 2}]")
    check(_lib.load().y3_evaluate_detections(_dev(packed), _dev(num_valid), B, M, _dev(gt_boxes), _dev(gt_classes), _dev(gt_count),
                                             G, nc, float(iou_threshold), _fptr(thr), len(thr), int(bool(one_class)),
                                             _dev(counters), _lib.stream_ptr()), "y3_evaluate_detections")
    return counters


def ap_iou_thresholds(ap):
    """The `ap` argument of evaluate_stream / evaluate -> its IoU thresholds, float32 [K]: True means the ten thresholds 0.5, 0.55,
    ..., 0.95 of mAP@[.5:.95] (evaluate_detections.AP_IOU_THRESHOLDS), a sequence means those thresholds."""
    from .evaluate_detections import AP_IOU_THRESHOLDS
    thr = AP_IOU_THRESHOLDS if ap is True else np.ascontiguousarray(np.asarray(ap, np.float32).reshape(-1))
    if not 1 <= len(thr) <= 16 or not np.isfinite(thr).all():
        raise Y3Error("ap: 1 to 16 finite IoU thresholds (or True for 0.5, 0.55, ..., 0.95)")
    return thr


def match_detections(packed: torch.Tensor, num_valid: torch.Tensor, gt_boxes: torch.Tensor, gt_classes: torch.Tensor,
                     gt_count: torch.Tensor, nclasses: int, iou_thresholds, one_class=False,
                     records: Optional[torch.Tensor] = None, gt_totals: Optional[torch.Tensor] = None):
    """The inputs of evaluate_detections -> (records int32 [B,M,2], gt_totals int64 [nclasses + 2]) on the GPU: per image the
    greedy matching behind COCO-style average precision, at every IoU threshold of iou_thresholds [K <= 16] (y3_match_detections;
    host restatement: evaluate_detections.match_detections, which also names the words; evaluate_detections.average_precision
    integrates the records of a data set).  The rows are matched in ROW order -- Net.detect writes them in descending score --
    and nothing is sorted.  records: the tensor to write (every row of it is written; torch has no arithmetic on uint32, so the
    words travel as int32 like the packed rows: .view(np.uint32) on the host); gt_totals=None: a zeroed tensor is made, otherwise
    the call ADDS to the one given.  Enqueues on the current stream only."""
    return _match(packed, num_valid, gt_boxes, gt_classes, gt_count, nclasses, iou_thresholds, one_class, records, gt_totals)


def _match(packed, num_valid, gt_boxes, gt_classes, gt_count, nclasses, iou_thresholds, one_class, records, gt_totals, lib=None):
    """match_detections; lib: the library handle to call through (a Net's own `lib`) instead of the module's."""
    _need_cuda(packed, num_valid, gt_boxes, gt_classes, gt_count, records, gt_totals)
    B, M, G = _scored_args(packed, num_valid, gt_boxes, gt_classes, gt_count)
    thr = np.ascontiguousarray(np.asarray(iou_thresholds, np.float32).reshape(-1))
    nc = int(nclasses)
    if records is None:
        records = torch.empty((B, M, 2), dtype=torch.int32, device=packed.device)
    elif records.dtype != torch.int32 or records.shape != (B, M, 2):
        raise Y3Error(f"records must be int32 [{B},{M},2]")
    if gt_totals is None:
        gt_totals = torch.zeros((max(nc, 0) + 2,), dtype=torch.int64, device=packed.device)
    elif gt_totals.dtype != torch.int64 or gt_totals.shape != (nc + 2,):
        raise Y3Error(f"gt_totals must be int64 [{nc + 2}]")
    check((lib or _lib.load()).y3_match_detections(_dev(packed), _dev(num_valid), B, M, _dev(gt_boxes), _dev(gt_classes), _dev(gt_count),
                                          G, nc, _fptr(thr), len(thr), int(bool(one_class)), _dev(records), _dev(gt_totals),
                                          _lib.stream_ptr()), "y3_match_detections")
    return records, gt_totals


def _gt_args(who, gt_boxes, gt_classes):
    if gt_boxes.dtype != torch.float32 or gt_boxes.dim() != 3 or gt_boxes.shape[2] != 4:
        raise Y3Error(f"{who}: gt_boxes must be float32 [B,G,4]")
    B, G = gt_boxes.shape[0], gt_boxes.shape[1]
    if gt_classes.dtype != torch.int32 or gt_classes.shape != (B, G):
        raise Y3Error(f"{who}: gt_classes must be int32 [{B},{G}]")
    return B, G


def assign_targets(gt_boxes: torch.Tensor, gt_classes: torch.Tensor, gt_count: torch.Tensor, anchors_table, grid_sizes,
                   nclasses: int, cells: Optional[torch.Tensor] = None):
    """Ground truth on the GPU as pack_ground_truth lays it out (gt_boxes [B,G,4] float32, gt_classes [B,G] int32, gt_count [B]
    int32) -> cells [B,G] int32 on the GPU: per ground-truth row the index of its label's row in decode's row order (best
    anchor by width/height IoU, the cell of its centre, the later row winning a shared cell), -1 behind the count, -2 for a row
    that lost its cell, -3 for the rows of an error image (y3_yolo_assign_targets; reference
    core/preprocess_dataset.py::_arrange_in_grid in sparse form; host restatement: core.preprocess_dataset.assign_targets).
    cells: the tensor to write.  Enqueues on the current stream only."""
    _need_cuda(gt_boxes, gt_classes, gt_count, cells)
    B, G = _gt_args("assign_targets", gt_boxes, gt_classes)
    if gt_count.dtype != torch.int32 or gt_count.shape != (B,):
        raise Y3Error(f"assign_targets: gt_count must be int32 [{B}]")
    gs = [int(g) for g in grid_sizes]
    if len(gs) != 3:
        raise Y3Error("assign_targets: three grid sizes")
    a = _anchors(anchors_table)
    if cells is None:
        cells = torch.empty((B, G), dtype=torch.int32, device=gt_boxes.device)
    elif cells.dtype != torch.int32 or cells.shape != (B, G):
        raise Y3Error(f"assign_targets: cells must be int32 [{B},{G}]")
    check(_lib.load().y3_yolo_assign_targets(_dev(gt_boxes), _dev(gt_classes), _dev(gt_count), B, G, int(nclasses),
                                             (C.c_int32 * 3)(*gs), _fptr(a), _dev(cells), _lib.stream_ptr()),
          "y3_yolo_assign_targets")
    return cells


def yolo_loss(grids, anchors_table, nclasses: int, gt_boxes: torch.Tensor, gt_classes: torch.Tensor, cells: torch.Tensor,
              loss: Optional[torch.Tensor] = None):
    """The raw head grids of Net.forward ([B,g,g,3,5+nc] each) + ground truth + the cells of assign_targets -> float64 [B,3,4] on
    the GPU: per image and scale the sums xy, wh, obj, class of reference core/loss_func.py (y3_yolo_loss; host restatement:
    core.loss_func.loss_from_cells).  An error image (cells -3) gets twelve zeros.  Each image's numbers are bit-identical
    whatever batch it is in.  This is the validation loss: no gradient, and the regulariser the reference's training loop adds
    (model.losses) is not part of it.  loss: the tensor to write (overwritten, not added to).  Enqueues on the current stream only."""
    ptrs, gs, B, _ = _grids_args(grids)
    _need_cuda(gt_boxes, gt_classes, cells, loss)
    nc = int(nclasses)
    if any(g.shape[4] != 5 + nc for g in grids):
        raise Y3Error(f"yolo_loss: each grid must be float32 [B,g,g,3,{5 + nc}]")
    if any(g.shape[0] != B for g in grids):
        raise Y3Error("yolo_loss: the grids hold unlike batches")
    Bg, G = _gt_args("yolo_loss", gt_boxes, gt_classes)
    if Bg != B:
        raise Y3Error(f"yolo_loss: {B} images in the grids, {Bg} in the ground truth")
    if cells.dtype != torch.int32 or cells.shape != (B, G):
        raise Y3Error(f"yolo_loss: cells must be int32 [{B},{G}]")
    a = _anchors(anchors_table)
    if loss is None:
        loss = torch.empty((B, 3, 4), dtype=torch.float64, device=gt_boxes.device)
    elif loss.dtype != torch.float64 or loss.shape != (B, 3, 4):
        raise Y3Error(f"yolo_loss: loss must be float64 [{B},3,4]")
    check(_lib.load().y3_yolo_loss(ptrs, gs, B, nc, _fptr(a), _dev(gt_boxes), _dev(gt_classes), _dev(cells), G, _dev(loss),
                                   _lib.stream_ptr()), "y3_yolo_loss")
    return loss


# the last NMS workspace per rule (per class or not): ((device, bytes), tensor).  One per rule, so that a call under the other rule
# does not free the workspace a captured graph of this one replays on
_ws_cache: Dict[bool, tuple] = {}


def _nms_workspace_bytes(B, N, per_class=False):
    lib = _lib.load()
    return lib.y3_nms_per_class_workspace_bytes(B, N) if per_class else lib.y3_nms_workspace_bytes(B, N)


def nms_padded(bboxes, scores, max_output_size, iou_threshold, score_threshold):
    """-> (selected_indices_padded [B,M] i32, num_valid [B] i32)"""
    return _nms(bboxes, scores, max_output_size, iou_threshold, score_threshold)


def nms_padded_per_class(bboxes, scores, classes, max_output_size, iou_threshold, score_threshold):
    """nms_padded with one predicate changed (y3_nms_padded_per_class): a box is suppressed by an earlier kept box iff their class
    ids are equal and IoU >= iou_threshold; the first max_output_size selected boxes over all classes together are returned.
    classes: int64 [B,N] as class_scores / yolo_decode_scores give them, ids in [0, 2^31).  iou_threshold must be > 0.
    -> (selected_indices_padded [B,M] i32, num_valid [B] i32).  Host restatement: nms_per_class.nms_padded_per_class_ref."""
    return _nms(bboxes, scores, max_output_size, iou_threshold, score_threshold, classes=classes)


def _nms(bboxes, scores, max_output_size, iou_threshold, score_threshold, out=None, ws=None, classes=None):
    """nms_padded, with `classes` nms_padded_per_class; out: the (sel, nv) tensors to write; ws: the caller's own workspace instead
    of the process-wide _ws_cache."""
    _need_cuda(bboxes, scores, classes)
    if bboxes.dtype != torch.float32 or scores.dtype != torch.float32:
        raise Y3Error("boxes and scores must be float32")
    B, N = scores.shape
    if classes is not None and (classes.dtype != torch.int64 or classes.shape != (B, N) or not classes.is_contiguous()):
        raise Y3Error(f"nms_padded_per_class: classes must be contiguous int64 [{B},{N}]")
    lib = _lib.load()
    if ws is None:
        need = _nms_workspace_bytes(B, N, classes is not None)
        key = (bboxes.device.index, need)
        held = _ws_cache.get(classes is not None)
        if held is None or held[0] != key:
            held = _ws_cache[classes is not None] = (key, torch.empty(need, dtype=torch.uint8, device=bboxes.device))
        ws = held[1]
    sel, nv = out or (torch.empty((B, int(max_output_size)), dtype=torch.int32, device=bboxes.device),
                      torch.empty((B,), dtype=torch.int32, device=bboxes.device))
    if classes is None:
        check(lib.y3_nms_padded(_dev(bboxes), _dev(scores), B, N, int(max_output_size), float(iou_threshold),
                                float(score_threshold), _dev(sel), _dev(nv), _dev(ws), ws.numel(), _lib.stream_ptr()),
              "y3_nms_padded")
    else:
        check(lib.y3_nms_padded_per_class(_dev(bboxes), _dev(scores), _dev(classes), B, N, int(max_output_size), float(iou_threshold),
                                          float(score_threshold), _dev(sel), _dev(nv), _dev(ws), ws.numel(), _lib.stream_ptr()),
              "y3_nms_padded_per_class")
    return sel, nv


def pack_detections(bboxes, cls, scores, sel, nv):
    """-> [B,M,7] int32 words: box (4 x f32 bits), score (f32 bits), class, index; rows >= num_valid zero"""
    return _pack(bboxes, cls, scores, sel, nv)


def _pack(bboxes, cls, scores, sel, nv):
    _need_cuda(bboxes, cls, scores, sel, nv)
    B, N = scores.shape
    M = sel.shape[1]
    out = torch.empty((B, M, 7), dtype=torch.int32, device=bboxes.device)
    check(_lib.load().y3_pack_detections(_dev(bboxes), _dev(cls), _dev(scores), _dev(sel), _dev(nv), B, N, M, _dev(out),
                                         _lib.stream_ptr()), "y3_pack_detections")
    return out


def merge_tiles_workspace_bytes(frames: int, tiles: int, max_boxes: int) -> int:
    """y3_merge_tiles_workspace_bytes: the workspace merge_tile_detections needs (either NMS rule); 0 for sizes it refuses."""
    return int(_lib.load().y3_merge_tiles_workspace_bytes(int(frames), int(tiles), int(max_boxes)))


def merge_tile_detections(packed: torch.Tensor, num_valid: torch.Tensor, windows, geoms, frame_hw, image_size,
                          iou_threshold: float, score_threshold: float, per_class: bool = False, out=None,
                          ws: Optional[torch.Tensor] = None, lib=None):
    """Sliced inference, the merge (y3_merge_tile_detections; host restatement: tiles.merge_tile_detections_ref).  packed
    [F*T,M,7] int32 words and num_valid [F*T] int32 on the GPU as Net.detect leaves them on the tile batch (tile t of frame f is
    image f * T + t; the boxes normalised to the canvas, NOT un-letterboxed); on the host windows int32 [F*T,4] = (y0, x0, ch,
    cw) (tile_descs), geoms int32 [F*T,4] (tile_letterbox_geometries) and frame_hw int32 [F,2] -> (packed [F,M,7], num_valid
    [F]) per FRAME, in frame coordinates: the tiles' rows mapped to the frame (merge_tiles_kernel), then the existing padded NMS
    over their union (per class with per_class=True) at iou_threshold / score_threshold with max_output_size M, then the
    existing pack.  The index word of a merged row is t * M + r.  image_size: the canvas, an int S or an (H, W) pair.
    out: the (packed, num_valid) tensors to write; ws: a uint8 workspace of merge_tiles_workspace_bytes(F, T, M) (one is made
    otherwise); lib: the library handle to call through.  Enqueues on the current stream only."""
    _need_cuda(packed, num_valid, ws)
    if packed.dtype != torch.int32 or packed.dim() != 3 or packed.shape[2] != 7:
        raise Y3Error("packed must be contiguous int32 [F*T,M,7]")
    fh = np.ascontiguousarray(frame_hw, dtype=np.int32)
    if fh.ndim != 2 or fh.shape[1] != 2 or len(fh) < 1 or packed.shape[0] % len(fh):
        raise Y3Error(f"frame_hw must be int32 [F,2] with F dividing the {packed.shape[0]} tile images")
    F, M = len(fh), packed.shape[1]
    T = packed.shape[0] // F
    if num_valid.dtype != torch.int32 or num_valid.shape != (F * T,):
        raise Y3Error(f"num_valid must be int32 [{F * T}]")
    w, g = np.ascontiguousarray(windows, dtype=np.int32), np.ascontiguousarray(geoms, dtype=np.int32)
    if w.shape != (F * T, 4) or g.shape != (F * T, 4):
        raise Y3Error(f"windows and geoms must be int32 [{F * T},4]")
    lib = lib or _lib.load()
    if ws is None:
        ws = torch.empty(max(lib.y3_merge_tiles_workspace_bytes(F, T, M), 16), dtype=torch.uint8, device=packed.device)
    elif ws.dtype != torch.uint8 or ws.dim() != 1:
        raise Y3Error("ws must be a 1-D uint8 tensor")
    merged, nv = out or (torch.empty((F, M, 7), dtype=torch.int32, device=packed.device),
                         torch.empty((F,), dtype=torch.int32, device=packed.device))
    _need_cuda(merged, nv)
    if merged.dtype != torch.int32 or merged.shape != (F, M, 7) or nv.dtype != torch.int32 or nv.shape != (F,):
        raise Y3Error(f"out must be int32 [{F},{M},7] and int32 [{F}]")
    from .input_stage import canvas_hw
    Hc, Wc = canvas_hw(image_size)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    check(lib.y3_merge_tile_detections(_dev(packed), _dev(num_valid), i32(w), i32(g), i32(fh), F, T, M, Hc, Wc,
                                       _lib.Y3_NMS_PER_CLASS if per_class else _lib.Y3_NMS_AGNOSTIC, float(iou_threshold),
                                       float(score_threshold), _dev(merged), _dev(nv), _dev(ws), ws.numel(), _lib.stream_ptr()),
          "y3_merge_tile_detections")
    return merged, nv


def unpack_detections(packed: torch.Tensor):
    """[.., M, 7] int32 words -> (boxes f32 [..,M,4], scores f32 [..,M], classes i32, indices i32)"""
    f = packed[..., :5].contiguous().view(torch.float32)
    return f[..., :4], f[..., 4], packed[..., 5], packed[..., 6]
