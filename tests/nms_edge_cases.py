"""NMS inputs the random stress sets never produce, shared by tests/test_nms_edges_host.py (the two CPU references against each other)
and tests/test_nms_edges_gpu.py (nms_kernel against the oracle, bit for bit): flipped boxes (the canonicalisation the kernel takes from
box [0,0] of the batch), negative and signed-zero scores, candidate counts placed on the kernel's own switches, and max_output_size
reached on a word, chunk and API boundary.

A case is (boxes [B,N,4] f32, scores [B,N] f32, M, T, S); boxes are (y1, x1, y2, x2) as TF reads them."""
import numpy as np

from tests.helpers import nms_stress_set

T_DEFAULT, S_DEFAULT = 0.5, 0.1


# ---------------------------------------------------------------------------------------------- 1. canonicalisation
CANONICAL = ("swap_y_all", "swap_x_all", "swap_both_all", "flip_box00_above_S", "flip_box00_below_S")


def canonical_base():
    """The unflipped batch the canonicalisation cases start from; box [0,0] scores above S."""
    boxes, scores = nms_stress_set(np.random.default_rng(71), 2, 1000)
    scores[0, 0] = 0.9
    return boxes, scores


def canonical_case(name):
    boxes, scores = canonical_base()
    if name in ("swap_y_all", "swap_both_all"):
        boxes[..., [0, 2]] = boxes[..., [2, 0]]
    if name in ("swap_x_all", "swap_both_all"):
        boxes[..., [1, 3]] = boxes[..., [3, 1]]
    if name == "flip_box00_above_S":      # swap_y for the whole batch, decided by one box: every other box turns upside down
        boxes[0, 0, [0, 2]] = boxes[0, 0, [2, 0]]
    if name == "flip_box00_below_S":      # the masked box is all zero: m00 = 0, no swap, and the flipped box itself is gone
        boxes[0, 0] = boxes[0, 0, [2, 3, 0, 1]]
        scores[0, 0] = 0.05
    assert name in CANONICAL
    return boxes, scores, 100, T_DEFAULT, S_DEFAULT


# ---------------------------------------------------------------------------------------------- 2. scores
SCORES = ("all_pass_S_minus_1", "negative_and_signed_zero")


def score_case(name):
    boxes, scores = nms_stress_set(np.random.default_rng(2), 3, 3000)
    if name == "all_pass_S_minus_1":      # the corner tests/test_oracle.py has and the device list stopped before
        return boxes, scores, 300, T_DEFAULT, -1.0
    assert name == "negative_and_signed_zero"
    scores = (scores - np.float32(0.2)).astype(np.float32)
    scores[:, 0::7] = np.float32(0.0)
    scores[:, 3::7] = np.float32(-0.0)
    assert np.signbit(scores[:, 3::7]).all() and not np.signbit(scores[:, 0::7]).any()
    return boxes, scores, 1024, T_DEFAULT, -0.1      # M above the survivor count: the selection runs through the zeros into the negatives


# ---------------------------------------------------------------------------------------------- 3. candidate counts
# 128: the balanced pair loop takes over from the triangular one; 256: the chunk; 512: the cap when T <= 0; 4096: the LDS sort's capacity
CANDIDATE_COUNTS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097)
DEGENERATE_COUNTS = (511, 512, 513)      # again at T = 0.0
N_COUNT = 6000
_count_boxes = {}


def count_case(nc, T=T_DEFAULT):
    """Exactly nc scores above S among 6000 stress-set boxes (both images, other places), the rest at 0.05; scores from a coarse grid,
    so most are duplicates; M = 1024, so the whole sorted order reaches the output."""
    if "b" not in _count_boxes:
        _count_boxes["b"] = nms_stress_set(np.random.default_rng(72), 2, N_COUNT)[0]
    boxes = _count_boxes["b"].copy()
    rng = np.random.default_rng(1000 + nc)
    scores = np.full((2, N_COUNT), 0.05, np.float32)
    for b in range(2):
        grid = rng.integers(0, max(nc // 3, 2), nc)
        scores[b, rng.permutation(N_COUNT)[:nc]] = (0.2 + 0.7 * grid / max(nc // 3, 2)).astype(np.float32)
    assert ((scores > S_DEFAULT).sum(1) == nc).all()
    return boxes, scores, 1024, T, S_DEFAULT


# ---------------------------------------------------------------------------------------------- 4. where M is reached
# every survivor is selected, in sorted order: the M-th selection is sorted position M - 1 -- bit 63 of a word (64, 128, ...), the last
# candidate of a chunk (256, 512, 1024), the first of the next (257); 1024 is the API's bound
M_VALUES = (63, 64, 65, 128, 255, 256, 257, 512, 1024)
N_LATTICE = 4096


def lattice_case(M, k):
    """k survivors on the disjoint 64 x 64 lattice of test_nms_survivor_counts (nothing suppresses anything), max_output_size M."""
    ii = np.arange(N_LATTICE)
    x0, y0 = (ii % 64) / 64.0, (ii // 64) / 64.0
    boxes = np.stack([x0 + 0.001, y0 + 0.001, x0 + 0.014, y0 + 0.014], -1).astype(np.float32)[None].repeat(2, 0)
    rng = np.random.default_rng(5000 + 3 * M + k)
    scores = np.full((2, N_LATTICE), 0.05, np.float32)
    for b in range(2):
        scores[b, rng.permutation(N_LATTICE)[:k]] = rng.uniform(0.2, 0.9, k).astype(np.float32)
    return boxes, scores, M, T_DEFAULT, S_DEFAULT
