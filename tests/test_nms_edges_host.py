"""The NMS edge cases of tests/nms_edge_cases.py on the host: the C oracle and the NumPy restatement of TF's tiled NMS (run to its fixed
point) must agree on every case the device is then held to (tests/test_nms_edges_gpu.py), and each case must do what it is for."""
import numpy as np
import pytest

from oracle import nms_tiled_ref as T
from oracle import oracle as O
from tests import nms_edge_cases as C


def _both(boxes, scores, M, Tt, S):
    """-> (sel, num_valid) of the oracle, after the tiled restatement gave the same."""
    a = O.nms_padded(boxes, scores, M, Tt, S)
    b = T.non_max_suppression_padded(boxes, scores, M, Tt, S, converge=True)
    assert np.array_equal(a[1], b[1]), (a[1], b[1])
    assert np.array_equal(a[0], b[0])
    assert all(not a[0][i, n:].any() for i, n in enumerate(a[1]))      # rows past num_valid are zero
    return a


@pytest.mark.parametrize("name", C.CANONICAL)
def test_canonicalisation_cases(name):
    boxes, scores, M, Tt, S = C.canonical_case(name)
    sel, nv = _both(boxes, scores, M, Tt, S)
    assert nv.min() > 10
    base_boxes, base_scores = C.canonical_base()
    base = O.nms_padded(base_boxes, base_scores, M, Tt, S)
    if name in ("swap_y_all", "swap_x_all", "swap_both_all"):
        # box [0,0] decides for the batch, and every box is flipped the same way: the unflipped batch's answer
        assert np.array_equal(sel, base[0]) and np.array_equal(nv, base[1])
    if name == "flip_box00_above_S":
        # one flipped box turns the whole batch: both images differ from the unflipped batch's, image 1 although none of ITS boxes
        # changed -- a kernel that read each image's own box 0 would leave image 1 as it was
        assert boxes[0, 0, 0] > boxes[0, 0, 2] and scores[0, 0] > S and np.array_equal(boxes[1], base_boxes[1])
        for b in range(2):
            assert not np.array_equal(sel[b], base[0][b]), b
    if name == "flip_box00_below_S":
        # m00 = 0: no swap.  The batch without its box [0,0] (score below S there too) gives the same answer
        assert boxes[0, 0, 0] > boxes[0, 0, 2] and boxes[0, 0, 1] > boxes[0, 0, 3] and scores[0, 0] <= S
        base_scores[0, 0] = 0.05
        gone = O.nms_padded(base_boxes, base_scores, M, Tt, S)
        assert np.array_equal(sel, gone[0]) and np.array_equal(nv, gone[1])


@pytest.mark.parametrize("name", C.SCORES)
def test_score_cases(name):
    boxes, scores, M, Tt, S = C.score_case(name)
    sel, nv = _both(boxes, scores, M, Tt, S)
    if name == "all_pass_S_minus_1":
        assert (scores > S).all() and (nv == M).all()
    else:
        picked = np.take_along_axis(scores, sel.astype(np.int64), axis=1)
        for b in range(len(nv)):
            p = picked[b, :nv[b]]
            assert (p > S).all()
            # the selection reaches the signed zeros and the negative scores behind them, in score order (-0.0 == +0.0: by index)
            assert (p == 0).sum() >= 2 and np.signbit(p[p == 0]).any() and not np.signbit(p[p == 0]).all(), b
            assert (p < 0).any() and (np.diff(p) <= 0).all(), b
            z = sel[b, :nv[b]][p == 0]
            assert (np.diff(z) > 0).all(), b
            # ... the two signs interleaved: a sort key taken from the bits of -0.0 would put one sign in front of the other
            assert np.abs(np.diff(np.signbit(p[p == 0]).astype(int))).sum() >= 3, b


@pytest.mark.parametrize("nc", C.CANDIDATE_COUNTS)
def test_candidate_count_cases(nc):
    boxes, scores, M, Tt, S = C.count_case(nc)
    sel, nv = _both(boxes, scores, M, Tt, S)
    assert (nv >= 1).all() and (nv <= nc).all()
    if nc >= 512:
        assert (nv > 100).all(), nv
    vals = scores[scores > S]
    assert nc < 8 or len(np.unique(vals)) < len(vals) / 2      # duplicates: the sort's tie rule is in play


@pytest.mark.parametrize("nc", C.DEGENERATE_COUNTS)
def test_candidate_count_cases_at_T_zero(nc):
    """T = 0: nothing is suppressed inside the first 512 sorted positions and everything behind them is wiped."""
    boxes, scores, M, Tt, S = C.count_case(nc, T=0.0)
    sel, nv = _both(boxes, scores, M, Tt, S)
    assert (nv == min(nc, 512)).all(), nv      # every stress-set box has a positive coordinate


@pytest.mark.parametrize("M", C.M_VALUES)
def test_where_M_is_reached(M):
    for k in (M - 1, M, M + 1):
        boxes, scores, M_, Tt, S = C.lattice_case(M, k)
        sel, nv = _both(boxes, scores, M_, Tt, S)
        assert (nv == min(k, M)).all(), (k, nv)
        for b in range(2):      # the first min(k, M) of the k scored boxes, by score
            order = np.argsort(-scores[b], kind="stable")[:min(k, M)]
            assert np.array_equal(sel[b, :nv[b]], order), (k, b)
