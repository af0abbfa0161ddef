"""Inputs the average-precision tests of both tiers share (tests/test_ap_host.py, tests/test_ap_gpu.py): the hand-made unit
cases of the matching, one per path, the seeded recipe of overlapping boxes, the IoU threshold sets, and an independent
brute-force matcher in plain Python loops."""
import numpy as np

from tests.evaluate_cases import batch_of, pack_rows

TEN = np.linspace(0.5, 0.95, 10).astype(np.float32)
THRESHOLDS = {1: np.array([0.5], np.float32), 10: TEN, 16: np.linspace(0.3, 0.975, 16).astype(np.float32)}
INVALID = 0xFFFFFFFF


def unit_cases():
    """[(name, nclasses, iou thresholds, data = (packed, num_valid, gt_boxes, gt_classes, gt_count), expected)]; expected: per
    image the masks of its first num_valid rows, or "error" for an error image (with one_class=False)."""
    cases = []

    def add(name, nc, thresholds, images, expected, M=None, G=None, num_valid=None, gt_count=None):
        packed, nv, gb, gc, cnt = batch_of(images, M, G)
        if num_valid is not None:
            nv = np.asarray(num_valid, np.int32)
        if gt_count is not None:
            cnt = np.asarray(gt_count, np.int32)
        cases.append((name, nc, np.asarray(thresholds, np.float32), (packed, nv, gb, gc, cnt), expected))

    box = [.125, .125, .5, .5]
    # two rows on one box: the second is FP at every threshold
    add("two rows on one box", 1, TEN, [([box, box], [0.9, 0.8], [0, 0], [box], [0])], [[0x3FF, 0]])
    # boxes A and B of one class overlap.  Row 0 is A itself; row 1 prefers A too (IoU 0.88 against 0.68 with B): A is taken, it
    # gets its second-best B up to 0.65 and nothing above
    A, B = [0, 0, .5, .5], [.125, 0, .625, .5]
    add("second best", 1, TEN, [([A, [.03125, 0, .53125, .5]], [0.9, 0.8], [0, 0], [A, B], [0, 0])], [[0x3FF, 0xF]])
    # row 0 lies midway between two boxes (IoU 0.6 with both, every operation exact in binary): it takes the HIGHER row, which is
    # the only one row 1 (IoU 1 with it, 1/3 with the other) could take at 0.5.  At 0.75 row 0 fails and row 1 matches
    add("equal IoU: the higher row wins", 1, [0.5, 0.75],
        [([[.25, .25, .75, .75], [.375, .25, .875, .75]], [0.9, 0.8], [0, 0], [[.125, .25, .625, .75], [.375, .25, .875, .75]], [0, 0])],
        [[0b01, 0b10]])
    add("class mismatch with IoU 1", 3, TEN, [([box], [0.9], [2], [box], [1])], [[0]])
    # IoU exactly 0.5 and exactly 0.75 (binary fractions: the division is exact); >= includes the threshold itself
    up = np.nextafter(np.float32(0.75), np.float32(1))
    add("IoU equal to a threshold", 2, [0.5, 0.75, up],
        [([[0, 0, .5, .5], [0, 0, .5, .5]], [0.9, 0.8], [0, 1], [[0, 0, .5, .25], [0, 0, .5, .375]], [0, 1])], [[0b001, 0b011]])
    # a zero-area row against a zero-area box elsewhere: 0/0.  The NaN never qualifies, not even at a negative threshold; the
    # box around the row (IoU 0) does, at -1 and at 0
    add("two zero-area boxes", 1, [-1.0, 0.0, 0.5], [([[.2, .2, .2, .2]], [0.9], [0], [[.1, .1, .3, .3], [.6, .6, .6, .6]], [0, 0])],
        [[0b011]])
    add("num_valid 0", 2, TEN, [([], [], [], [box, A], [0, 1])], [[]])
    add("gt_count 0", 2, TEN, [([box, A], [0.9, 0.8], [0, 1], [], [])], [[0, 0]])
    # counts beyond the buffers (and below zero) are clamped: image 0 holds 2 rows and 1 box, image 1 counts nothing
    add("counts outside their range", 1, TEN, [([box, box], [0.9, 0.8], [0, 0], [box], [0]), ([box, box], [0.9, 0.8], [0, 0], [box], [0])],
        [[0x3FF, 0], []], num_valid=[7, -3], gt_count=[5, -1])
    # error images: a ground-truth class of -1 and of nclasses, a row class of nclasses and of 2**30; image 0 is clean
    img = ([box, A], [0.9, 0.8], [1, 2])
    add("bad classes", 3, TEN, [img + ([box, A], [1, 0]), img + ([box, A], [1, -1]), img + ([box, A], [3, 1]),
                                ([box, A], [0.9, 0.8], [1, 3], [box, A], [1, 2]), ([box, A], [0.9, 0.8], [2**30, 1], [box, A], [1, 2])],
        [[0x3FF, 0], "error", "error", "error", "error"])
    # a bad class behind num_valid is never read
    add("bad class behind num_valid", 3, TEN, [([box, A], [0.9, 0.8], [1, 7], [box], [1])], [[0x3FF]], num_valid=[1])
    # row 0 (IoU 0.6) takes the box at 0.5 and fails at 0.75, where row 1 (IoU 0.9) finds it free
    add("matched at 0.75 and not at 0.5", 1, [0.5, 0.75], [([[0, 0, .5, .3], [0, 0, .5, .45]], [0.9, 0.8], [0, 0], [A], [0])],
        [[0b01, 0b10]])
    return cases


def expected_records(case):
    """The hand-written expectation of a unit case as (records uint32 [B,M,2], gt_totals int64 [nc + 2]), one_class=False."""
    _, nc, _, (packed, nv, gb, gc, cnt), expected = case
    B, M = packed.shape[:2]
    rec = np.zeros((B, M, 2), np.uint32)
    rec[..., 1] = INVALID
    totals = np.zeros(nc + 2, np.int64)
    for b, masks in enumerate(expected):
        if isinstance(masks, str):
            totals[nc] += 1
            continue
        n = len(masks)
        assert n == min(max(int(nv[b]), 0), M)
        rec[b, :n, 0] = packed[b, :n, 4].view(np.uint32)
        rec[b, :n, 1] = packed[b, :n, 5].astype(np.uint32) | (np.asarray(masks, np.uint32) << np.uint32(16))
        totals[:nc] += np.bincount(gc[b, :min(max(int(cnt[b]), 0), gc.shape[1])], minlength=nc)
        totals[nc + 1] += 1
    return rec, totals


SIGMAS = (0.001, 0.004, 0.01, 0.02, 0.04)
RECIPE_SEED = 11
RECIPE_NC = 3
MAIN_SHAPE = (5, 100, 65)       # B, M, G of the recipe the non-triviality conditions are asserted on


def recipe(seed, B, M, G, nc=RECIPE_NC):
    """Overlapping boxes with jittered detections in shuffled order.  Per image g ground-truth boxes (image 0: G, otherwise 1 ..
    G), centres U(0.25,0.75), sides U(0.1,0.4), classes U{0 .. nc-1}: crowded, so boxes of one class overlap.  Each box gets 0 to
    3 + M // g detections: the box plus N(0, sigma) on every coordinate, sigma cycling through SIGMAS, its class (one in eight:
    the next class).  The detections are shuffled and cut to M rows; the scores are sorted descending from U(0,1), so the row
    order is unrelated to the IoU."""
    rng = np.random.default_rng(seed)
    packed = np.zeros((B, M, 7), np.int32)
    nv = np.zeros(B, np.int32)
    gb = np.zeros((B, G, 4), np.float32)
    gc = np.zeros((B, G), np.int32)
    cnt = np.zeros(B, np.int32)
    for b in range(B):
        g = G if b == 0 else int(rng.integers(1, G + 1))
        c, s = rng.uniform(0.25, 0.75, (g, 2)), rng.uniform(0.1, 0.4, (g, 2))
        gb[b, :g] = np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32)
        gc[b, :g] = rng.integers(0, nc, g)
        cnt[b] = g
        boxes, classes = [], []
        for j in range(g):
            for d in range(int(rng.integers(0, 4 + M // g))):
                boxes.append(gb[b, j] + rng.normal(0, SIGMAS[d % len(SIGMAS)], 4).astype(np.float32))
                classes.append((gc[b, j] + 1) % nc if rng.integers(0, 8) == 0 else gc[b, j])
        order = rng.permutation(len(boxes))[:M]
        n = len(order)
        nv[b] = n
        scores = np.sort(rng.uniform(0, 1, n).astype(np.float32))[::-1]
        packed[b] = pack_rows(np.asarray(boxes, np.float32).reshape(-1, 4)[order], scores, np.asarray(classes, np.int32)[order], M)
    return packed, nv, gb, gc, cnt


def brute_force(packed, nv, gb, gc, cnt, nc, thresholds, one_class=False):
    """The matching in plain Python loops over scalars, written from the rule and not from the restatement: per image a list of
    masks, or None for an error image."""
    B, M = packed.shape[:2]
    G = gc.shape[1]
    boxes = packed[..., :4].copy().view(np.float32)
    f = np.float32

    def iou(p, q):
        with np.errstate(invalid="ignore", divide="ignore"):
            ow = max(f(min(p[2], q[2]) - max(p[0], q[0])), f(0))
            oh = max(f(min(p[3], q[3]) - max(p[1], q[1])), f(0))
            inter = f(ow * oh)
            a1, a2 = f(f(p[2] - p[0]) * f(p[3] - p[1])), f(f(q[2] - q[0]) * f(q[3] - q[1]))
            return f(inter / f(f(a1 + a2) - inter))

    out = []
    for b in range(B):
        n, g = min(max(int(nv[b]), 0), M), min(max(int(cnt[b]), 0), G)
        pc = [0 if one_class else int(packed[b, r, 5]) for r in range(n)]
        tc = [0 if one_class else int(gc[b, j]) for j in range(g)]
        if any(c < 0 or c >= nc for c in pc + tc):
            out.append(None)
            continue
        table = [[iou(boxes[b, r], gb[b, j]) for j in range(g)] for r in range(n)]
        masks = [0] * n
        for k, t in enumerate(np.asarray(thresholds, np.float32)):
            taken = [False] * g
            for r in range(n):
                best = -1
                for j in range(g):
                    v = table[r][j]
                    if taken[j] or tc[j] != pc[r] or not v >= t:
                        continue
                    if best < 0 or v >= table[r][best]:
                        best = j
                if best >= 0:
                    taken[best] = True
                    masks[r] |= 1 << k
        out.append(masks)
    return out
