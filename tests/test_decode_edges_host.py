"""The cases of tests/decode_edge_cases.py on the CPU reference (oracle.yolo_decode / the NumPy restatement on gh != gw grids,
y3o_scores): every expected class index, every entry claimed to be exactly 1.0f / 0.0f / inf really is, no constructed logit lies in
the range the module refuses to assert on, and the class-count cases really end every scale on a partial workgroup and leave a scalar
tail where the module says they do.  This keeps the cases from going soft; tests/test_decode_edges_gpu.py runs them on the device."""
import numpy as np
import pytest

from tests import decode_edge_cases as C


@pytest.fixture(scope="module", params=list(C.GRID_SETS))
def gs(request):
    return C.GRID_SETS[request.param]


@pytest.mark.parametrize("index", range(len(C.case_ids())), ids=C.case_ids())
def test_case_claims_hold_on_the_cpu_reference(anchors, gs, index):
    case = C.all_cases(gs)[index]
    assert not C.in_avoided_range(case["grids"])
    N = C.n_boxes(gs)
    for g, (gh, gw) in zip(case["grids"], gs):
        assert g.dtype == np.float32 and g.shape[1:] == (gh, gw, 3, 5 + case["nc"]) and g.flags.c_contiguous
    rb, rc, rp, cls, scores = C.reference(case, anchors)
    assert rb.shape == (case["grids"][0].shape[0], N, 4)
    C.check_claims(case, rb, rc, rp, cls, scores)
    assert np.array_equal(cls, rp.argmax(-1))      # y3o_scores is the first maximum, as NumPy's argmax is


def test_the_two_cpu_references_agree_on_square_grids(anchors):
    """The NumPy restatement used on gh != gw grids against the C oracle where both apply: within 2 ulp of expf, inf where inf."""
    from yolo_v3_tf2_amd.core.yolo_decode_layer import yolo_decode_hw_host
    for case in (C.saturated_fields(C.SQUARE), C.pair_ties(C.SQUARE)):
        rb, rc, rp, _, _ = C.reference(case, anchors)
        with np.errstate(over="ignore", invalid="ignore"):
            hb, hc, hp = yolo_decode_hw_host(case["grids"], anchors, case["nc"])
        fin = np.isfinite(rb)
        assert np.array_equal(fin, np.isfinite(hb)) and np.array_equal(rb[~fin], hb[~fin])
        assert np.abs(hb[fin] - rb[fin]).max() <= 2e-6 * np.abs(rb[fin]).max()
        assert np.abs(hc.reshape(rc.shape) - rc).max() <= 2e-6 and np.abs(hp - rp).max() <= 2e-6


def test_pair_ties_cover_every_lane_distance(gs):
    case = C.pair_ties(gs)
    assert len(C.PAIRS) == 36 and {(j - i) % 4 for i, j in C.PAIRS} == {0, 1, 2, 3}      # same lane, neighbours, two apart
    rows = np.concatenate([g.reshape(g.shape[0], -1, g.shape[-1]) for g in case["grids"]], 1)
    built = rows[..., 5:].max(-1) > -3.0
    assert built.sum() == 72 and case["score_conf"].sum() == 36 and case["prob_one"].sum() == 72
    assert sorted(case["cls"][built].tolist()) == sorted(2 * [i for i, _ in C.PAIRS])
    # the saturated pairs hold DIFFERENT logits, the later class the larger one: only the probabilities tie
    sat = rows[case["score_conf"]][:, 5:]
    assert all(len(set(r[r > 0].tolist())) == 2 and r.argmax() > (r > 0).argmax() for r in sat)


def test_class_count_cases_end_on_partial_workgroups_and_scalar_tails():
    """decode_kernel: 64 boxes per workgroup, 16-byte copies plus a scalar tail of nbox * F % 4 floats."""
    B = C.CLASS_COUNTS_BATCH
    for nc in C.CLASS_COUNTS:
        sq, rc = C.workgroup_shape(C.SQUARE, B, nc), C.workgroup_shape(C.RECT, B, nc)
        assert [t for t, _, _ in sq] == [36, 144, 576] and [last for _, last, _ in sq] == [36, 16, 64]      # partial, partial, full
        assert all(tail == 0 for _, _, tail in sq)
        assert [t for t, _, _ in rc] == [27, 108, 432] and [last for _, last, _ in rc] == [27, 44, 48]      # every scale partial
        assert rc[0][2] == 27 * (5 + nc) % 4 and (rc[0][2] != 0) == ((5 + nc) % 4 != 0)
    tails = {nc: C.workgroup_shape(C.RECT, B, nc)[0][2] for nc in C.CLASS_COUNTS}
    assert set(tails.values()) == {0, 1, 2, 3}, tails      # nc = 3, 79: none; the other seven: 1, 2 and 3 floats


def test_limit_case_is_the_whole_lds_allowance():
    case = C.limit_case()
    assert C.DEC_BOXES * (5 + case["nc"]) * 4 == 160 * 1024 and case["nc"] == 635
    assert C.n_boxes(case["gs"]) == 63 and not C.in_avoided_range(case["grids"])
