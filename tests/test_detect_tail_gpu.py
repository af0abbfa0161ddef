"""The detection tail on the device: y3_net_detect_grids against the routes that existed before it (Net.detect, Net.forward,
ops.decode_candidates), and the rule that a refused call of y3_net_detect, y3_net_detect_grids or y3_merge_tile_detections enqueues
nothing.  Every net here takes the 64 x 64 network input (one case 64 x 96) with 3 images and 80 classes: grids 2 x 2, 4 x 4, 8 x 8,
N = 252, and 36, 144 and 576 boxes per scale over the batch -- a decode workgroup that is one partial block, one whose partial last block
straddles an image boundary, and whole blocks.  Every comparison is exact."""
import ctypes as C_

import numpy as np
import pytest

from tests import tile_cases as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, NC, M, IOU, SCORE = 3, 80, 100, 0.5, 0.03      # SCORE: tests/test_multilabel_gpu.py, some tens of candidates per image
SENTINEL = 0x5A5A5A5A
PER_CLASS_TEXT = "iou_threshold must be > 0 with Y3_NMS_PER_CLASS"
BOTH_TEXT = "iou_threshold <= 0 together with score_threshold < 0 is not supported"


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _net(rt, program, weights, dtype="f32", size=64):
    from yolo_v3_tf2_amd import _lib
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(B, size, {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16}[dtype])
    return net


def _input(size=64):
    H, W = (size, size) if isinstance(size, int) else size
    return _cuda(np.random.default_rng(1234).random((B, H, W, 3), dtype=np.float32))


def _buffers(net, fill=None):
    """-> (grids, packed, num_valid) as y3_net_detect_grids writes them for B images; fill: an int32 word every buffer is filled with."""
    grids = [torch.empty((B, gh, gw, 3, 5 + NC), dtype=torch.float32, device="cuda") for gh, gw in net._grid_hw()]
    packed = torch.empty((B, M, 7), dtype=torch.int32, device="cuda")
    nv = torch.empty((B,), dtype=torch.int32, device="cuda")
    if fill is not None:
        for t in grids + [packed, nv]:
            t.view(torch.int32).fill_(fill)
    return grids, packed, nv


def _call(net, name, xd, anchors, grids, packed, nv, iou=IOU, score=SCORE, max_boxes=M):
    """y3_net_detect (grids is None) or y3_net_detect_grids on the current stream -> (status, message)."""
    from yolo_v3_tf2_amd import _lib
    from yolo_v3_tf2_amd._args import _anchors, _dev, _fptr
    a = _anchors(anchors, reshape=True)
    head = (net._h, _dev(xd), B, _fptr(a), int(max_boxes), float(iou), float(score))
    tail = (_dev(packed), _dev(nv), _lib.stream_ptr())
    if name == "y3_net_detect":
        st = net.lib.y3_net_detect(*head, *tail)
    else:
        ptrs = None if grids is None else (C_.c_void_p * 3)(*[g.data_ptr() for g in grids])
        st = net.lib.y3_net_detect_grids(*head, ptrs, *tail)
    return st, net.lib.y3_last_error().decode()


# ------------------------------------------------------------------------------------------------ 1. against the existing routes
@pytest.mark.parametrize("per_class", [False, True], ids=["agnostic", "per_class"])
@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_detect_grids_equals_detect_and_forward(rt, program, weights, anchors, dtype, multi, per_class):
    _check_detect_grids(rt, _net(rt, program, weights, dtype), _input(), anchors, multi, per_class)


def test_detect_grids_with_a_binding_capacity(rt, program, weights, anchors):
    """multi_label_capacity at half the smallest total: every image is truncated."""
    net, xd = _net(rt, program, weights), _input()
    net.multi_label = True
    net.detect(xd, anchors, M, IOU, SCORE)
    totals = net.multi_label_totals.cpu().numpy()
    print("totals", totals.tolist())
    assert (totals >= 2).all(), totals
    cap = int(totals.min()) // 2
    got = _check_detect_grids(rt, net, xd, anchors, True, True, capacity=cap)
    assert (got > cap).all()


def test_detect_grids_on_a_rectangular_plan(rt, program, weights, anchors):
    """64 x 96: gh != gw through the shared prologue, on both decodes."""
    for multi in (False, True):
        _check_detect_grids(rt, _net(rt, program, weights, size=(64, 96)), _input((64, 96)), anchors, multi, False)


def _check_detect_grids(rt, net, xd, anchors, multi, per_class, capacity=0):
    from yolo_v3_tf2_amd import ops
    net.nms_per_class, net.multi_label, net.multi_label_capacity = per_class, multi, capacity
    want_packed, want_nv = (t.clone() for t in net.detect(xd, anchors, M, IOU, SCORE))
    want_grids = [g.clone() for g in net.forward(xd)]
    grids, packed, nv = _buffers(net, fill=SENTINEL)
    st, msg = _call(net, "y3_net_detect_grids", xd, anchors, grids, packed, nv)
    assert st == 0, msg
    assert torch.equal(nv, want_nv) and torch.equal(packed, want_packed)
    for g, w in zip(grids, want_grids):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32))
    print("num_valid", nv.tolist())
    assert int(nv.max()) > 0
    if not multi:
        return None
    n_boxes = sum(3 * gh * gw for gh, gw in net._grid_hw())
    totals = ops.decode_candidates(grids, anchors, NC, SCORE, capacity or n_boxes)[4]
    assert torch.equal(net.multi_label_totals, totals)
    return totals.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 2. refused calls enqueue nothing
@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_refused_detect_enqueues_nothing(rt, program, weights, anchors, multi):
    from yolo_v3_tf2_amd import _lib
    net, xd = _net(rt, program, weights), _input()
    net.multi_label = multi
    grids, packed, nv = _buffers(net, fill=SENTINEL)
    for name in ("y3_net_detect", "y3_net_detect_grids"):
        g = None if name == "y3_net_detect" else grids
        cases = [(True, dict(iou=0.0), PER_CLASS_TEXT), (True, dict(iou=float("nan")), PER_CLASS_TEXT),
                 (False, dict(iou=0.0, score=-1.0), BOTH_TEXT), (False, dict(max_boxes=0), "max_boxes must be in [1,1024]"),
                 (False, dict(max_boxes=1025), "max_boxes must be in [1,1024]")]
        for per_class, kw, text in cases:
            net.nms_per_class = per_class
            st, msg = _call(net, name, xd, anchors, g, packed, nv, **kw)
            assert st == _lib.Y3_ERR_INVALID and msg.startswith(name + ": ") and text in msg, (name, kw, st, msg)
        net.nms_per_class = False
        if multi:
            net.multi_label_capacity = 253
            st, msg = _call(net, name, xd, anchors, g, packed, nv)
            assert st == _lib.Y3_ERR_INVALID and msg.startswith(name + ": ") and "exceeds the 252 boxes of the plan" in msg, (name, st, msg)
            net.multi_label_capacity = 0
        for kw in (dict(packed=None), dict(nv=None), dict(xd=None)):
            a = dict(dict(xd=xd, packed=packed, nv=nv), **kw)
            st, msg = _call(net, name, a["xd"], anchors, g, a["packed"], a["nv"])
            assert st == _lib.Y3_ERR_INVALID and msg.startswith(name + ": bad argument"), (name, kw, st, msg)
    st, msg = _call(net, "y3_net_detect_grids", xd, anchors, None, packed, nv)
    assert st == _lib.Y3_ERR_INVALID and msg.startswith("y3_net_detect_grids: bad argument"), (st, msg)
    torch.cuda.synchronize()
    for t in grids + [packed, nv]:
        assert (t.view(torch.int32) == SENTINEL).all()
    # ... and the accepted call that follows them writes all of it
    st, msg = _call(net, "y3_net_detect_grids", xd, anchors, grids, packed, nv)
    assert st == 0, msg
    torch.cuda.synchronize()
    assert all(not (t.view(torch.int32) == SENTINEL).any() for t in grids) and not (nv == SENTINEL).any()


def test_refused_merge_enqueues_nothing(rt):
    from yolo_v3_tf2_amd import ops
    case = K.merge_case(B, 2, 4, seed=1, canvas=(64, 64))
    packed, nv = _cuda(case["packed"]), _cuda(case["nv"])
    out = (torch.full((B, 4, 7), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda"))
    ws = torch.full((ops.merge_tiles_workspace_bytes(B, 2, 4),), 0xFF, dtype=torch.uint8, device="cuda")
    for per_class, iou, score, text in ((True, 0.0, 0.05, PER_CLASS_TEXT), (False, 0.0, -1.0, BOTH_TEXT)):
        with pytest.raises(rt.Y3Error) as e:
            ops.merge_tile_detections(packed, nv, case["windows"], case["geoms"], case["frame_hw"], 64, iou, score, per_class=per_class,
                                      out=out, ws=ws)
        assert "y3_merge_tile_detections: " + text in str(e.value)
    torch.cuda.synchronize()
    assert (out[0] == SENTINEL).all() and (out[1] == SENTINEL).all() and (ws == 0xFF).all()
