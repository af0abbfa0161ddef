"""y3_net_detect_grids without a device: its row in the _lib.py table, its declaration in include/y3.h, and the refusals that need no
net -- the ones y3_net_detect makes, under its own name.  (A net needs a device: tests/test_detect_tail_gpu.py holds the refusals
that need one.)"""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_and_header():
    from yolo_v3_tf2_amd import _lib
    res, args = _lib.SYMBOLS["y3_net_detect_grids"]
    dres, dargs = _lib.SYMBOLS["y3_net_detect"]
    # y3_net_detect's arguments with the three grid pointers, y3_net_forward's form, in front of the outputs
    assert res is dres is C.c_int and args == dargs[:7] + [C.POINTER(C.c_void_p)] + dargs[7:]
    assert _lib.SYMBOLS["y3_net_forward"][1][3] == C.POINTER(C.c_void_p)
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "y3.h")).read())
    assert ("y3_status y3_net_detect_grids(y3_net *net, const float *images_dev, int batch, const float *anchors_host, int max_boxes, "
            "float iou_threshold, float score_threshold, float *const grids_out_dev[3], void *packed_dev, int32_t *num_valid_dev, "
            "void *stream);") in header


def test_refusals_without_a_net():
    from yolo_v3_tf2_amd import _lib
    lib = _lib.load()
    dev = C.c_void_p(4096)      # never followed: every call below is refused on the host
    a = (C.c_float * 18)()
    grids = (C.c_void_p * 3)(4096, 4096, 4096)
    good = dict(net=None, images=dev, B=1, anchors=a, M=100, grids=grids, packed=dev, nv=dev)
    for kw in (dict(), dict(grids=None), dict(packed=None), dict(nv=None), dict(images=None), dict(anchors=None), dict(M=0), dict(M=1025),
               dict(B=0)):
        v = dict(good, **kw)
        head = (v["net"], v["images"], v["B"], v["anchors"], v["M"], 0.5, 0.1)
        assert lib.y3_net_detect_grids(*head, v["grids"], v["packed"], v["nv"], None) == _lib.Y3_ERR_INVALID, kw
        msg = lib.y3_last_error()
        assert msg == b"y3_net_detect_grids: bad argument", (kw, msg)
        if "grids" not in kw:
            assert lib.y3_net_detect(*head, v["packed"], v["nv"], None) == _lib.Y3_ERR_INVALID, kw
            assert lib.y3_last_error() == msg.replace(b"_grids", b""), kw
