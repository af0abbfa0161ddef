"""Inputs of per-class NMS shared by tests/test_nms_per_class_host.py (the NumPy restatement against brute force and the C oracle)
and tests/test_nms_per_class_gpu.py (nms_kernel<PER_CLASS> against the restatement, bit for bit).

A case is (boxes [B,N,4] f32, scores [B,N] f32, classes [B,N] i64, M, T, S); boxes are (y1, x1, y2, x2)."""
import numpy as np

from tests import nms_edge_cases as C

T, S = C.T_DEFAULT, C.S_DEFAULT
KEPT_CAP = 2048      # csrc/nms.hip: kept boxes beyond this many live in the global workspace, their class ids with them

# candidate counts on the kernel's switches: the balanced pair loop takes over at 128, the chunk is 256 (513: a third, short chunk),
# 4097 leaves the LDS sort
RANDOM_COUNTS = (127, 128, 129, 255, 256, 257, 513, 4097)
RANDOM_CLASSES = (2, 7, 80)
BIG_IDS = np.array([0, 1, 2**30, 2**31 - 2, 2**31 - 1], np.int64)


def random_ids(seed, shape, ncls):
    return np.random.default_rng(seed).integers(0, ncls, shape).astype(np.int64)


def random_case(nc, ncls, M):
    """Exactly nc candidates among the 6000 stress-set boxes of nms_edge_cases.count_case, class ids uniform over ncls classes."""
    boxes, scores, _, t, s = C.count_case(nc)
    return boxes, scores, random_ids(7000 + 13 * nc + ncls, scores.shape, ncls), M, t, s


def merge_of_agnostic_runs(nms_padded, boxes, scores, classes, M, T, S):
    """The second consequence of the rule: per class the AGNOSTIC result (`nms_padded`, the oracle's) with every other class's
    score replaced by the finite filler S - 1, the per-class results merged by (score descending, index ascending) and cut at M."""
    B = scores.shape[0]
    sel, nv = np.zeros((B, M), np.int32), np.zeros(B, np.int32)
    rows = [[] for _ in range(B)]
    for c in np.unique(classes):
        masked = np.where(classes == c, scores, np.float32(S) - np.float32(1.0)).astype(np.float32)
        sc, nc = nms_padded(boxes, masked, M, T, S)
        for b in range(B):
            rows[b] += [(-(float(scores[b, i]) + 0.0), int(i)) for i in sc[b, :nc[b]]]
    for b in range(B):
        picked = [i for _, i in sorted(rows[b])][:M]
        sel[b, :len(picked)], nv[b] = picked, len(picked)
    return sel, nv


def _lattice(n, origin=0.0):
    """n pairwise-disjoint boxes on a 64-wide lattice of 1/64 cells starting at `origin`"""
    ii = np.arange(n)
    x0, y0 = origin + (ii % 64) / 64.0, origin + (ii // 64) / 64.0
    return np.stack([y0 + 0.001, x0 + 0.001, y0 + 0.014, x0 + 0.014], -1).astype(np.float32)


def _descending(n, hi=0.95, lo=0.2):
    """n strictly decreasing scores: sorted position == index"""
    s = np.linspace(hi, lo, n).astype(np.float32)
    assert (np.diff(s) < 0).all()
    return s


def distinct_ids_case(M):
    """Heavily overlapping stress-set boxes, every box a class of its own: nothing is suppressed."""
    boxes, scores, _, t, s = C.count_case(513)
    classes = np.arange(scores.size, dtype=np.int64).reshape(scores.shape)
    return boxes, scores, classes, M, t, s


def duplicates_case():
    """600 disjoint boxes in descending score order (sorted position == index) with four exact duplicates: positions 10 and 11
    repeat 3 and 4 (the same chunk: the suppression rows), 300 and 301 repeat 5 and 6 (an earlier chunk: the kept list in LDS);
    10 and 300 have their original's class, 11 and 301 another.  -> case, the indices that must be missing"""
    n = 600
    boxes, scores, classes = _lattice(n), _descending(n), np.zeros(n, np.int64)
    for dup, orig, other in ((10, 3, False), (11, 4, True), (300, 5, False), (301, 6, True)):
        boxes[dup] = boxes[orig]
        classes[dup] = 1 if other else 0
    boxes, scores, classes = (np.stack([a, a]) for a in (boxes, scores, classes))
    classes[1] += 5      # image 1: the same pattern on other ids
    return (boxes, scores, classes, 1024, T, S), (10, 300)


CHUNK = 256          # csrc/nms.hip: sorted candidates are resolved 256 at a time; an earlier chunk's survivors are met in the kept-list pass


def spill_case():
    """The kept list past KEPT_CAP, so that a suppressor and its class id are read back from the workspace.  max_output_size <= 1024
    bounds the SELECTED boxes, so the list is filled with kept boxes that are never selected: pairwise-disjoint boxes of class 0 with
    no positive coordinate (y in [-0.5, -0.001], x < 0), in descending score order, so that sorted position == kept slot == index
    for them.  Boxes 0..2815 are eleven whole chunks; those from slot 2048 on (chunk 8 and later) live in the workspace.  A probe
    meets an original only in the kept-list pass when it lies in a LATER chunk, so every probe sits at least one chunk behind the
    box it rests on (`origin`; the in-chunk pair loop never sees the pair):
      chunk 11 (positions 2816..3071)
        D1  an exact duplicate of box 2100 (chunk 8, spilled), class 0      dropped by the spilled box of its class
        D2  an exact duplicate of box 2200 (chunk 8, spilled), class 1      kept (2200 is class 0): itself spilled, with class 1
        P1  box 2150 (chunk 8, spilled) with y2 raised to +1e-4 (IoU ~ 1 with 2150), class 0
                                                                            suppressed by spilled box 2150: NOT selected
        P2  box 2250 (chunk 8, spilled) likewise, class 2                   only an other-class spilled box overlaps it: selected
        P4  box 100 (chunk 0, in LDS) likewise, class 0                     suppressed from the kept list in LDS: NOT selected
        P5  box 101 (chunk 0, in LDS) likewise, class 2                     selected
        then 250 more disjoint boxes without a positive coordinate, class 0, which fill the chunk
      chunk 12 (positions 3072..)
        P3  box 2200 raised likewise, class 1                               suppressed only by D2 (chunk 11, spilled, class 1; the
                                                                            spilled box 2200 itself is class 0): NOT selected
        then 40 disjoint positive boxes of classes 0 and 1, all selected.
    A kernel that takes every spilled class id as equal drops P2, one that takes none as equal selects P1 and P3, one that loses D2's
    id selects P3.  Image 1 is the same with classes 0 and 1 swapped.
    -> case, {name: index}, {name: index of the box it rests on}, the indices that must be selected, in order"""
    nneg, nfill = 11 * CHUNK, CHUNK - 6
    k = np.arange(nneg + nfill)
    neg = np.stack([np.full(len(k), -0.5), -(k + 1) * 0.01, np.full(len(k), -0.001), -(k + 1) * 0.01 + 0.008], -1).astype(np.float32)
    assert (neg <= 0).all() and (neg[:, 3] > neg[:, 1]).all() and (neg[1:, 3] < neg[:-1, 1]).all()      # no positive coordinate, disjoint

    def raised(i):
        b = neg[i].copy()
        b[2] = np.float32(1e-4)
        return b

    probes = [("D1", neg[2100], 0, 2100), ("D2", neg[2200], 1, 2200), ("P1", raised(2150), 0, 2150), ("P2", raised(2250), 2, 2250),
              ("P4", raised(100), 0, 100), ("P5", raised(101), 2, 101)]
    later = [("P3", raised(2200), 1, 2200)]
    pos = _lattice(40, origin=0.01)
    boxes = np.concatenate([neg[:nneg], np.stack([b for _, b, _, _ in probes]), neg[nneg:], np.stack([b for _, b, _, _ in later]),
                            pos]).astype(np.float32)
    classes = np.concatenate([np.zeros(nneg, np.int64), [c for _, _, c, _ in probes], np.zeros(nfill, np.int64), [c for _, _, c, _ in later],
                              np.arange(40) % 2]).astype(np.int64)
    n = len(boxes)
    scores = _descending(n)
    at = {name: nneg + j for j, (name, _, _, _) in enumerate(probes)}
    at["P3"] = nneg + CHUNK
    origin = {name: o for name, _, _, o in probes + later}
    selected = [at["P2"], at["P5"]] + list(range(at["P3"] + 1, n))
    swapped = np.where(classes < 2, 1 - classes, classes)
    case = (np.stack([boxes, boxes]), np.stack([scores, scores]), np.stack([classes, swapped]), 1024, T, S)
    return case, at, origin, selected
