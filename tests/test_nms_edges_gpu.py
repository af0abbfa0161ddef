"""nms_kernel on the cases of tests/nms_edge_cases.py, bit for bit against the oracle (which tests/test_nms_edges_host.py holds to the
tiled restatement on the same cases): both canonicalisation branches, negative and signed-zero scores, candidate counts on the kernel's
switches (128, 256, 512, 4096), and max_output_size reached on a word, a chunk and the API's boundary."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import oracle as O  # noqa: E402
from tests import nms_edge_cases as C  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(rt, boxes, scores, M, T, S):
    rs, rn = O.nms_padded(boxes, scores, M, T, S)
    gs, gn = rt.nms_padded(_cuda(boxes), _cuda(scores), M, T, S)
    torch.cuda.synchronize()
    gs, gn = gs.cpu().numpy(), gn.cpu().numpy()
    assert np.array_equal(gn, rn), (gn, rn)
    assert np.array_equal(gs, rs), int((gs != rs).sum())
    assert all(not gs[i, n:].any() for i, n in enumerate(gn))      # rows past num_valid are zero
    return rn


@pytest.mark.parametrize("name", C.CANONICAL)
def test_nms_canonicalisation_on_the_device(rt, name):
    nv = _check(rt, *C.canonical_case(name))
    assert nv.min() > 10


@pytest.mark.parametrize("name", C.SCORES)
def test_nms_negative_and_zero_scores(rt, name):
    nv = _check(rt, *C.score_case(name))
    assert nv.min() > 100


def test_nms_refuses_T_le_0_with_negative_S(rt):
    boxes, scores, M, _, _ = C.score_case("all_pass_S_minus_1")
    b, s = _cuda(boxes), _cuda(scores)
    for T in (0.0, -0.5):
        with pytest.raises(rt.Y3Error, match="iou_threshold <= 0 together with score_threshold < 0 is not supported"):
            rt.nms_padded(b, s, M, T, -1.0)
    sel, nv = rt.nms_padded(b, s, M, 0.0, 0.0)      # either alone is served
    torch.cuda.synchronize()
    rs, rn = O.nms_padded(boxes, scores, M, 0.0, 0.0)
    assert np.array_equal(nv.cpu().numpy(), rn) and np.array_equal(sel.cpu().numpy(), rs)


@pytest.mark.parametrize("nc", C.CANDIDATE_COUNTS)
def test_nms_candidate_counts_on_the_switches(rt, nc):
    nv = _check(rt, *C.count_case(nc))
    assert (nv >= 1).all() and (nc < 512 or (nv > 100).all())


@pytest.mark.parametrize("nc", C.DEGENERATE_COUNTS)
def test_nms_candidate_counts_at_T_zero(rt, nc):
    nv = _check(rt, *C.count_case(nc, T=0.0))
    assert (nv == min(nc, 512)).all()


@pytest.mark.parametrize("M", C.M_VALUES)
def test_nms_where_M_is_reached(rt, M):
    for k in (M - 1, M, M + 1):
        nv = _check(rt, *C.lattice_case(M, k))
        assert (nv == min(k, M)).all(), (k, nv)
