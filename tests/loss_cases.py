"""Inputs the validation-loss tests of both tiers share (tests/test_loss_host.py, tests/test_loss_gpu.py): the random recipe, the
larger shapes, the hand-made assignment cases, and the bar the device's loss is held to."""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The device and NumPy compute the same fp32 terms and differ by the last bits of expf / logf.  The float32 restatement and the
# same restatement in float64 differ by that kind of error, so the bar is 4 x the largest relative gap between those two over
# every case below (the factor: two libms disagreeing in opposite directions on top of the fp32 rounding).  The gap is taken per
# entry of the [B,3,4] result, relative to that entry, so it is set by the entries with the fewest terms: the xy sum of a scale
# that holds one box is scale * (dx^2 + dy^2) with dx = tx - sigmoid(t) a difference of two numbers of like size.
# Measured, largest entry of loss_from_cells(float32) against loss_from_cells(float64): recipe nc = 1 / 7 / 80 with max_gt 40:
# 5.63e-07 / 1.03e-06 / 2.85e-07; with max_gt 1: 1.87e-06 / 1.85e-07 / 3.87e-07; (13,26,52): 1.35e-06; (19,38,76): 1.07e-06.
# tests/test_loss_host.py::test_float32_rounding_stays_under_a_quarter_of_the_bar holds the bar to this basis.
LARGEST_GAP = 1.88e-06
LOSS_RTOL = 4 * LARGEST_GAP


def anchors():
    from yolo_v3_tf2_amd.core.utils import get_anchors
    return get_anchors(os.path.join(ROOT, "datasets/coco2012/anchors.txt")).astype(np.float32)


def random_boxes(rng, n):
    """Centres U[0,1), sides exp(U(log 0.015, log 0.95) + N(0, 0.3)) clipped to [0.01, 0.95], corners clipped to [0, 0.999]."""
    c = rng.random((n, 2))
    side = np.clip(np.exp(rng.uniform(np.log(0.015), np.log(0.95), (n, 1)) + rng.normal(0, 0.3, (n, 2))), 0.01, 0.95)
    return np.clip(np.concatenate([c - side / 2, c + side / 2], 1), 0, 0.999).astype(np.float32)


def random_grids(rng, B, grid_sizes, nc):
    """Logits N(0, 1.5), with -2 on the objectness logit."""
    grids = []
    for g in grid_sizes:
        t = rng.normal(0, 1.5, (B, g, g, 3, 5 + nc)).astype(np.float32)
        t[..., 4] -= 2
        grids.append(t)
    return grids


def make_case(seed, grid_sizes, counts, nc, max_gt):
    """-> dict(grids, gt_boxes [B,G,4], gt_classes [B,G], gt_count [B], grid_sizes, nc): one image per entry of `counts`."""
    from yolo_v3_tf2_amd.runtime import pack_ground_truth
    rng = np.random.default_rng(seed)
    gts = [(random_boxes(rng, n), rng.integers(0, nc, n).astype(np.int32)) for n in counts]
    gb, gc, cnt = pack_ground_truth(gts, max_gt)
    return dict(grids=random_grids(rng, len(counts), grid_sizes, nc), gt_boxes=gb, gt_classes=gc, gt_count=cnt,
                grid_sizes=tuple(grid_sizes), nc=nc)


RECIPE_GRIDS = (2, 4, 8)
RECIPE_COUNTS = {40: (1, 3, 8, 40, 0), 1: (1, 1, 1, 1, 0)}


def collisions(cells):
    return int((np.asarray(cells) == -2).sum())


@functools.lru_cache(maxsize=None)
def recipe(nc, max_gt=40):
    """Five images of 1, 3, 8, 40 and 0 boxes (max_gt = 1: the one-box variant, 1, 1, 1, 1 and 0) on grids (2,4,8).  Made once per
    (nc, max_gt) and shared: treat it as read-only.  The max_gt = 40 recipe must reach every (scale, anchor) pair and hold
    cell collisions, or the tests built on it stop seeing what they are meant to see."""
    from yolo_v3_tf2_amd.core.preprocess_dataset import assign_targets
    case = make_case(1030 + nc, RECIPE_GRIDS, RECIPE_COUNTS[max_gt], nc, max_gt)
    if max_gt == 40:
        cells = assign_targets(case["gt_boxes"], case["gt_classes"], case["gt_count"], anchors(), RECIPE_GRIDS, nc)
        offs = np.array([0, 12, 60, 252])
        pairs = set()
        for n in cells[cells >= 0]:
            s = int(np.searchsorted(offs, n, side="right")) - 1
            pairs.add((s, int(n - offs[s]) % 3))
        assert len(pairs) == 9, f"the recipe reaches only {sorted(pairs)}"
        assert collisions(cells) >= 8, f"the recipe holds only {collisions(cells)} cell collisions"
        assert not (cells == -3).any()
    return case


@functools.lru_cache(maxsize=None)
def large_case(grid_sizes):
    """(13,26,52): three images of 100, 10 and 55 boxes, max_gt 100; (19,38,76): two images of 60 and 5 boxes (the larger bitmap)."""
    counts, max_gt = {(13, 26, 52): ((100, 10, 55), 100), (19, 38, 76): ((60, 5), 60)}[tuple(grid_sizes)]
    return make_case(sum(grid_sizes), grid_sizes, counts, 80, max_gt)


def all_loss_cases():
    """(name, case) of every shape the device's loss is compared on."""
    for max_gt in (40, 1):
        for nc in (1, 7, 80):
            yield f"recipe-nc{nc}-g{max_gt}", recipe(nc, max_gt)
    for gs in ((13, 26, 52), (19, 38, 76)):
        yield "grids-%d-%d-%d" % gs, large_case(gs)


def relative_gap(got, want):
    """The largest |got - want| / |want| over the entries where want != 0; entries where want == 0 must be equal."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    zero = want == 0
    assert np.array_equal(got[zero], want[zero]), "an entry that is exactly 0 on one side is not on the other"
    if zero.all():
        return 0.0
    return float((np.abs(got - want)[~zero] / np.abs(want[~zero])).max())


# ---------------------------------------------------------------------------------------------------------------------------
# Assignment unit cases on grids (2,4,8): (name, nclasses, anchors [3,3,2], [(boxes, classes) per image], cells wanted per image)
def _centred(cx, cy, w, h):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]


def unit_cases():
    a = anchors()
    tied = a.copy()
    tied[1, 1] = tied[1, 0]                       # anchors 3 and 4 are the same: an exact IoU tie
    w4, h4 = float(a[1, 1, 0]), float(a[1, 1, 1])  # anchor 4 -> scale 1 (g = 4), a = 1
    w3, h3 = float(a[1, 0, 0]), float(a[1, 0, 1])
    at = lambda s_off, g, row, col, k: s_off + (row * g + col) * 3 + k
    return [
        # two boxes of anchor 4's size around (0.3, 0.3): cell (1,1) of the 4 x 4 grid, twice; the third row elsewhere
        ("a collision keeps the later row", 3, a,
         [([_centred(0.3, 0.3, w4, h4), _centred(0.31, 0.29, w4, h4), _centred(0.8, 0.55, w4, h4)], [0, 1, 2])],
         [[-2, at(12, 4, 1, 1, 1), at(12, 4, 2, 3, 1)]]),
        # (0.75 + 1.25) / 2 is exactly 1.0: col = g; both rows of that image are marked, its neighbour is not
        ("a centre of exactly 1.0 is an error image", 3, a,
         [([_centred(0.3, 0.3, w4, h4), [0.75, 0.2, 1.25, 0.4]], [0, 1]), ([_centred(0.3, 0.3, w4, h4)], [2])],
         [[-3, -3], [at(12, 4, 1, 1, 1), -1]]),
        ("a class equal to nclasses is an error image", 3, a,
         [([_centred(0.3, 0.3, w4, h4)], [2]), ([_centred(0.3, 0.3, w4, h4), _centred(0.6, 0.6, w4, h4)], [1, 3])],
         [[at(12, 4, 1, 1, 1), -1], [-3, -3]]),
        ("a negative class is an error image", 3, a, [([_centred(0.3, 0.3, w4, h4)], [-1])], [[-3]]),
        ("a non-finite coordinate is an error image", 3, a,
         [([_centred(0.3, 0.3, w4, h4), [0.1, np.inf, 0.2, 0.3]], [0, 1]), ([[np.nan, 0.1, 0.2, 0.3]], [0])],
         [[-3, -3], [-3, -1]]),
        ("an exact IoU tie takes the first anchor", 3, tied, [([_centred(0.3, 0.3, w3, h3)], [0])], [[at(12, 4, 1, 1, 0)]]),
        # w = h = 0: every IoU is 0 / (anchor area) = 0, the first anchor (scale 0, g = 2) takes it; (0.5, 0.5) is cell (1,1)
        ("a zero-area box is assigned", 3, a, [([[0.5, 0.5, 0.5, 0.5]], [1])], [[at(0, 2, 1, 1, 0)]]),
        ("no ground truth", 3, a, [([], []), ([], [])], [[-1], [-1]]),
        # -0.2 * 8 = -1.6 truncates to -1: outside; -0.1 * 2 = -0.2 truncates to 0: inside, as tf.cast has it
        ("a centre left of the image", 3, a,
         [([_centred(-0.2, 0.5, 0.03, 0.03)], [0]), ([_centred(-0.1, 0.5, 0.9, 0.8)], [0])],
         [[-3], [at(0, 2, 1, 0, 2)]]),
    ]


def unit_batch(images, max_gt=None):
    from yolo_v3_tf2_amd.runtime import pack_ground_truth
    return pack_ground_truth([(np.asarray(b, np.float32).reshape(-1, 4), np.asarray(c, np.int32)) for b, c in images], max_gt)


def unit_want(want, G):
    out = np.full((len(want), G), -1, np.int32)
    for b, row in enumerate(want):
        out[b, :len(row)] = row
    return out
