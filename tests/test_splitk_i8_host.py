"""Low-latency int8 plans without a GPU: the three entry points in the header, the binding, runtime.Net and the model object with their
argument checks; the teeth of the wide-accumulator case of tests/splitk_i8_cases.py (float32 slabs WOULD change its results); and the
number of K slices y3_choose_split_k gives each int8 conv shape of YOLOv3 for one 416 x 416 image.

The rule's inputs are the ones resolve_splits feeds it for an int8 conv: workgroups of the 64x64 LDS-DMA tile (id 11, where the chooser
ends for every conv that cannot reach 512 workgroups), K tiles of 128, 256 compute units, the bytes of one i32 slab [Mpad][CoutPad]."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# K tiles of 128 from which the rule acts (kSplitMinKTilesI8 in csrc/y3_net.cpp, set from profiles/latency_i8_splitk_sweep.txt)
I8_MIN_K_TILES = 36

# (ksize, Cin, Cout, grid side) -> (workgroups, K tiles, slab bytes, S of the rule, S in force): pinned literals, the int8 convs of YOLOv3
# (conv 9 on) that are no detection heads, stride-2 and stride-1 forms of a shape alike.  In force: the rule's S for a conv of at least
# I8_MIN_K_TILES K tiles, else 1; the library is held to that column on the GPU (tests/test_splitk_i8_gpu.py::test_low_latency_i8_network)
RULE_B1_S416 = [
    ((3, 512, 1024, 13), (48, 36, 786432, 9, 9)),
    ((1, 1024, 512, 13), (24, 8, 393216, 2, 1)),
    ((1, 512, 256, 13), (12, 4, 196608, 1, 1)),
    ((3, 256, 512, 26), (88, 18, 1441792, 4, 1)),
    ((1, 512, 256, 26), (44, 4, 720896, 1, 1)),       # 4 K tiles: one slice of at least 4 tiles is the unsplit launch
    ((1, 768, 256, 26), (44, 6, 720896, 1, 1)),       # the neck's up-sample + concat 1x1
    ((1, 256, 128, 26), (22, 2, 360448, 1, 1)),
    ((3, 128, 256, 52), (172, 9, 2818048, 2, 1)),
    ((1, 256, 128, 52), (86, 2, 1409024, 1, 1)),
    ((1, 384, 128, 52), (86, 3, 1409024, 1, 1)),
]


@pytest.mark.parametrize("shape,want", RULE_B1_S416)
def test_rule_for_one_416_image(shape, want):
    from yolo_v3_tf2_amd import _lib
    k, cin, cout, g = shape
    M = g * g
    tiles = -(-M // 64) * (cout // 64)
    k_tiles = k * k * cin // 128
    slab = -(-M // 64) * 64 * cout * 4
    assert (tiles, k_tiles, slab) == want[:3]
    assert _lib.load().y3_choose_split_k(tiles, k_tiles, 256, slab) == want[3]
    assert want[4] == (want[3] if k_tiles >= I8_MIN_K_TILES else 1)      # the table's own two columns agree with the floor as documented


def test_the_table_lists_every_int8_shape_of_the_network(program):
    from yolo_v3_tf2_amd import quant
    convs = program.conv_ops()
    cut = quant.first_i8_conv(program)
    assert cut == 9
    shapes = {(o.size, o.cin, o.cout, 416 // o.out_div) for o in convs[cut:] if o.dst not in program.outputs}
    assert shapes == {shape for shape, _ in RULE_B1_S416}


def test_entry_points_are_declared_and_bound():
    from yolo_v3_tf2_amd import _lib, runtime
    from yolo_v3_tf2_amd.core.parse_model import YoloModel
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "y3.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("y3_net_set_low_latency_i8", "y3_net_set_split_k_i8", "y3_net_get_split_k_i8"):
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
    for name in ("set_low_latency_i8", "set_split_k_i8", "split_k_i8"):
        assert callable(getattr(runtime.Net, name)), name
    assert callable(YoloModel.set_low_latency_i8)


def test_null_net_is_refused_by_the_library():
    """Argument refusals of the C entry points that need no device: a null net."""
    from yolo_v3_tf2_amd import _lib
    lib = _lib.load()
    assert lib.y3_net_set_low_latency_i8(None, 1) != 0 and b"y3_net_set_low_latency_i8" in lib.y3_last_error()
    assert lib.y3_net_set_split_k_i8(None, 0, 2) != 0 and b"y3_net_set_split_k_i8" in lib.y3_last_error()
    assert lib.y3_net_get_split_k_i8(None, 0) == 1


def test_python_argument_checks():
    """The checks run before the library is touched, so an object without a device net shows them."""
    from yolo_v3_tf2_amd import runtime
    Net, Y3Error = runtime.Net, runtime.Y3Error
    net = Net.__new__(Net)          # no device object: every call below must raise before it would need one
    net.conv_ops = [object()] * 3
    net._h = None
    for bad in (0, 17, -2, True, 2.0, None):
        with pytest.raises(Y3Error, match="split_k"):
            net.set_split_k_i8(0, bad)
    for bad_slot in (-1, 3, 1.0, None, True):
        with pytest.raises(Y3Error, match="conv slot"):
            net.set_split_k_i8(bad_slot, 2)
        with pytest.raises(Y3Error, match="conv slot"):
            net.split_k_i8(bad_slot)
    for bad in ("on", 2, 1.0):
        with pytest.raises(Y3Error, match="low_latency"):
            net.set_low_latency_i8(bad)


def test_model_remembers_the_switch_until_the_device_net_exists(program):
    from yolo_v3_tf2_amd.core.parse_model import YoloModel
    from yolo_v3_tf2_amd.runtime import Y3Error
    m = YoloModel(program)
    assert m.low_latency_i8 is False
    m.set_low_latency_i8(True)
    assert m.low_latency_i8 is True and m._net is None and m.low_latency is False and m.low_latency_f16 is False
    m.set_low_latency_i8(None)
    assert m.low_latency_i8 is False
    with pytest.raises(Y3Error):
        m.set_low_latency_i8(2)


# ---------------------------------------------------------------------------------------------- the wide case's teeth
def test_wide512_case_float_slabs_would_change_the_results():
    """On the case's own integers: the S slice sums add up to the conv's accumulator, single slices lie beyond 2^24, and a slab that held
    them as float32 ("slices converted to float32, then added") differs from float32(exact sum) in fp32-output elements at S = 2 and at
    S = 3 -- so the device test's bit-equality with quant.py cannot pass on float slabs."""
    from tests import splitk_i8_cases as C
    from tests.i8_edge_cases import parts
    from yolo_v3_tf2_amd import quant
    case, xq, ref = C.get()
    p = case.program
    assert quant.first_i8_conv(p) == 0
    for role, t in (("a", case.stored["a"]), ("h", case.heads["h"])):
        o = case.op(t)
        assert o.size == 3 and o.cin == 512 and o.size * o.size * o.cin // C.BK == 36 and quant.writes_f32(p, o) == (role == "h")
        acc = parts(case, ref, t)[0]
        assert 2 ** 24 < np.abs(acc).max() < 2 ** 31
        for S in C.WIDE_SPLITS:
            sl = C.slice_sums(o, case.weights, xq, S)
            assert np.array_equal(sl.sum(axis=0), acc)                       # the slices are the conv, cut along K
            assert all(np.abs(s).max() > 2 ** 24 for s in sl)
            exact = acc.astype(np.float32)
            via_float = sl[0].astype(np.float32)
            for s in sl[1:]:
                via_float = via_float + s.astype(np.float32)
            frac = float((via_float != exact).mean())
            print(f"wide512 {role} S={S}: {frac:.3f} of the accumulators differ through float32 slabs; slice |sum| max "
                  f"{[int(np.abs(s).max()) for s in sl]}, total {int(np.abs(acc).max())}")
            assert (via_float != exact).any(), (role, S)
            if role == "h":     # ... and the difference reaches the stored fp32 value: same epilogue on the two accumulators
                from tests.i8_edge_cases import F32
                _, sw = quant.quantize_weights(case.weights[f"conv{o.conv_index}.w"])
                bn_scale, shift = quant.bn_fold(o, case.weights)
                sc = ((F32(case.scales[o.src0]) * sw).astype(F32) * bn_scale).astype(F32)
                v_exact = (exact * sc).astype(F32) + shift
                v_float = (via_float * sc).astype(F32) + shift
                assert np.array_equal(v_exact.astype(F32), ref[t])
                assert (v_float.astype(F32) != ref[t]).any(), S
