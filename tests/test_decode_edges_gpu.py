"""decode_kernel and class_scores_kernel on the cases of tests/decode_edge_cases.py (which tests/test_decode_edges_host.py holds to
the CPU reference): class counts 1 to 81, tied class probabilities, saturated fields, and the widest row launch_decode admits.
The square grid set goes through the square entry points (y3_yolo_decode, y3_yolo_decode_scores), the rectangular one through
the _hw entry points (runtime.yolo_decode, runtime.yolo_decode_scores)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import decode_edge_cases as E  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


@pytest.fixture(scope="module", params=list(E.GRID_SETS))
def gs(request):
    return E.GRID_SETS[request.param]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _decode_both(rt, grids, anchors, nc, square):
    """(boxes, conf, probs) of the decode and (boxes, cls, scores) of the fused decode + arg-max, as device tensors."""
    if not square:
        return rt.yolo_decode(grids, anchors, nc), rt.yolo_decode_scores(grids, anchors, nc)
    from yolo_v3_tf2_amd import _lib
    lib = _lib.load()
    B, N = grids[0].shape[0], sum(3 * g.shape[1] * g.shape[2] for g in grids)
    ptrs = (C.c_void_p * 3)(*[g.data_ptr() for g in grids])
    sizes = (C.c_int32 * 3)(*[g.shape[1] for g in grids])
    a = np.ascontiguousarray(anchors, np.float32)
    ap = a.ctypes.data_as(C.POINTER(C.c_float))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ob, oconf, oprobs = torch.empty((B, N, 4), device="cuda"), torch.empty((B, N, 1), device="cuda"), torch.empty((B, N, nc), device="cuda")
    _lib.check(lib.y3_yolo_decode(ptrs, sizes, B, nc, ap, p(ob), p(oconf), p(oprobs), _lib.stream_ptr()), "y3_yolo_decode")
    ob2, ocls, osc = torch.empty((B, N, 4), device="cuda"), torch.empty((B, N), dtype=torch.int64, device="cuda"), torch.empty((B, N), device="cuda")
    _lib.check(lib.y3_yolo_decode_scores(ptrs, sizes, B, nc, ap, p(ob2), p(ocls), p(osc), _lib.stream_ptr()), "y3_yolo_decode_scores")
    return (ob, oconf, oprobs), (ob2, ocls, osc)


def _check_case(rt, case, anchors):
    nc = case["nc"]
    square = all(gh == gw for gh, gw in case["gs"])
    rb, rc, rp, _, _ = E.reference(case, anchors)
    grids = [_cuda(g) for g in case["grids"]]
    (gb, gc, gp), (sb, scls, ssc) = _decode_both(rt, grids, anchors, nc, square)
    cls2, s2 = rt.class_scores(gc, gp)
    torch.cuda.synchronize()
    assert tuple(gb.shape) == rb.shape and tuple(gp.shape) == rp.shape and tuple(gc.shape) == rc.shape + (1,)
    # fused == two-step, bit for bit (NaN-safe: compared as bit patterns)
    assert torch.equal(sb.view(torch.int32), gb.view(torch.int32)), (case["name"], "boxes of the fused call")
    assert torch.equal(scls, cls2), (case["name"], "class index: fused against decode + class_scores", int((scls != cls2).sum()))
    assert torch.equal(ssc.view(torch.int32), s2.view(torch.int32)), (case["name"], "score: fused against decode + class_scores")
    b, conf, probs, cls, scores = gb.cpu().numpy(), gc.cpu().numpy().reshape(rc.shape), gp.cpu().numpy(), scls.cpu().numpy(), ssc.cpu().numpy()
    # non-finite: inf where the reference is inf, of its sign; never NaN
    for got, ref in ((b, rb), (conf, rc), (probs, rp)):
        assert not np.isnan(got).any(), (case["name"], "NaN")
        assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref)), (case["name"], "inf")
    # finite: the bar of test_decode_matches_oracle, boxes scaled by the largest finite reference magnitude
    fin = np.isfinite(rb)
    scale = max(1.0, float(np.abs(rb[fin]).max()))
    errs = float(np.abs(b[fin] - rb[fin]).max()) / scale, float(np.abs(conf - rc).max()), float(np.abs(probs - rp).max())
    print(case["name"], "square" if square else "rect", "box / conf / prob deviation", errs)
    assert max(errs) <= 2e-6, (case["name"], errs)
    # arg-max: the first maximum of the device's own probabilities, every box
    assert np.array_equal(cls, probs.argmax(-1)), (case["name"], "not the first maximum", np.argwhere(cls != probs.argmax(-1))[:5].tolist())
    assert np.array_equal(scores, conf * probs.max(-1)), (case["name"], "score != objectness * max probability")
    # what the case was built to give, exactly
    E.check_claims(case, b, conf, probs, cls, scores)


@pytest.mark.parametrize("index", range(len(E.case_ids())), ids=E.case_ids())
def test_decode_edge_case(rt, anchors, gs, index):
    _check_case(rt, E.all_cases(gs)[index], anchors)


def test_decode_widest_row_the_launch_admits(rt, anchors):
    """5 + nc = 640: 64 boxes x 640 floats = 160 KB, the whole LDS of a compute unit, on grids (1, 2, 4) with B = 1."""
    _check_case(rt, E.limit_case(), anchors)


def test_decode_refuses_a_row_wider_than_lds(rt, anchors):
    """5 + nc = 641 does not fit: Y3Error from both entry points (launch_decode returns before it launches), and the stream
    is left usable."""
    case = E.limit_case(E.LIMIT_F + 1)
    assert case["nc"] == 636
    grids = [_cuda(g) for g in case["grids"]]
    for fn in (rt.yolo_decode, rt.yolo_decode_scores):
        with pytest.raises(rt.Y3Error):
            fn(grids, anchors, case["nc"])
    torch.cuda.synchronize()      # and no launch failed asynchronously
    # the stream still serves the admitted size afterwards
    ok = E.limit_case()
    b, _, _ = rt.yolo_decode_scores([_cuda(g) for g in ok["grids"]], anchors, ok["nc"])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(b).all())
