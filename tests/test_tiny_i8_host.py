"""int8 plans of pooled nets on the CPU (Net.set_pools_i8; include/y3.h, "Stand-alone ops in int8"): the plan rules restated in quant.py on
the YOLOv3-tiny program, quant.forward_i8 against a brute-force walker, why a pool may keep its source's scale, the new bindings, and
the accuracy of the scheme against the fp32 oracle.  No GPU: the library is loaded for its host-side refusals only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from tests import tiny_cases as TC
from tests import tiny_i8_cases as IC
from yolo_v3_tf2_amd import _lib, quant
from yolo_v3_tf2_amd.graph import AuxOp
from yolo_v3_tf2_amd.maxpool import maxpool2x2_ref

ROOT = TC.ROOT


@pytest.fixture(scope="module")
def tiny():
    return TC.tiny_program(80)


# ---------------------------------------------------------------------------------------------- 1. the tiny program
def test_tiny_cut_crossing_and_classes(tiny):
    cut = quant.first_i8_conv(tiny)
    convs = tiny.conv_ops()
    assert cut == 4 and (convs[4].size, convs[4].cin, convs[4].cout, convs[4].out_div) == (3, 128, 256, 16)
    assert all(o.cin % 128 == 0 for o in convs[cut:]) and max(o.cin for o in convs[cut:]) == 1024
    assert any(o.cin == 384 and o.size == 3 for o in convs[cut:])                  # the conv behind the concat
    aux, behind = quant.i8_aux_ops(tiny, cut)
    assert [(o.kind, o.inputs, o.dst) for o in aux] == [("maxpool_s2", [9], 10), ("maxpool_s1", [11], 12), ("upsample", [18], 19),
                                                        ("concat", [19, 9], 20)]
    assert quant.crossing_tensors(tiny, cut) == [8] and 8 not in behind
    assert quant.scale_classes(tiny, cut) == [[9, 10, 18, 19, 20], [11, 12]] == quant.scale_classes(tiny)
    # the four pools before the cut stay what an fp16 plan runs
    assert [o.dst for o in tiny.ops if isinstance(o, AuxOp) and o not in aux] == [2, 4, 6, 8]
    # share of the FLOPs behind the cut, at the stored widths
    fl = [2.0 * o.size ** 2 * o.cin * o.cout / o.out_div ** 2 for o in convs]
    assert 0.68 < sum(fl[cut:]) / sum(fl) < 0.70


def test_equalize_concat_gives_every_class_its_largest_scale(tiny):
    s = [0.01 * (1 + (5 * t) % 7) for t in range(len(tiny.tensors))]
    e = quant.equalize_concat(tiny, s)
    for g in quant.scale_classes(tiny):
        assert all(e[t] == max(s[u] for u in g) for t in g)
    tied = {t for g in quant.scale_classes(tiny) for t in g}
    assert all(e[t] == s[t] for t in range(len(s)) if t not in tied) and 8 not in tied
    # an unset member takes the class's scale; a class with no scale at all stays unset
    s2 = [0.0] * len(s)
    s2[9] = 0.5
    e2 = quant.equalize_concat(tiny, s2)
    assert [e2[t] for t in (9, 10, 18, 19, 20)] == [0.5] * 5 and e2[11] == e2[12] == 0.0


def test_yolov3_keeps_its_concat_rule_and_has_no_int8_aux_ops():
    from yolo_v3_tf2_amd.graph import load_program
    p = load_program(os.path.join(ROOT, "config/models/yolov3/model.yaml"), 80)
    cut = quant.first_i8_conv(p)
    assert cut == 9 and quant.i8_aux_ops(p, cut)[0] == []
    convs = p.conv_ops()
    behind = {o.dst for o in convs[cut:]}
    assert quant.crossing_tensors(p, cut) == sorted({t for o in convs[cut:] for t in (o.src0, o.src1, o.residual) if t >= 0 and t not in behind})
    assert quant.scale_classes(p) == sorted(sorted((o.src0, o.src1)) for o in convs if o.src1 >= 0)


def test_refused_graphs_are_refused_by_the_restatement_too():
    q = IC.mixed_concat_program()
    with pytest.raises(ValueError, match="one source behind the int8 cut and one before it"):
        quant.i8_aux_ops(q, quant.first_i8_conv(q))
    q = IC.add_behind_cut_program()
    with pytest.raises(ValueError, match="stand-alone add"):
        quant.i8_aux_ops(q, quant.first_i8_conv(q))


# ---------------------------------------------------------------------------------------------- 2. forward_i8 against plain loops
@pytest.mark.parametrize("canvas,batch", [((8, 8), 1), ((12, 4), 2)], ids=["8x8", "12x4x2"])
def test_forward_i8_equals_the_brute_force_walker_on_a_reduced_pooled_program(canvas, batch):
    p, ids = IC.reduced_pooled_program()
    assert quant.first_i8_conv(p) == 0 and [o.dst for o in quant.i8_aux_ops(p, 0)[0]] == [ids[k] for k in ("pa", "pb", "up", "cat")]
    w, x = IC.reduced_inputs(p, batch, canvas)
    s = IC.class_scales(p)
    boundary = {p.input_tensor: quant.quantize(x, s[p.input_tensor])}
    got = quant.forward_i8(p, w, s, boundary)
    ref = IC.brute_walk(p, w, s, boundary, 0)
    assert sorted(got) == sorted(ref) == list(range(len(p.tensors)))
    for t in got:
        assert got[t].dtype == ref[t].dtype == (np.float32 if t in p.outputs else np.int8), t
        assert got[t].shape == ref[t].shape and np.array_equal(got[t], ref[t]), t
        assert np.abs(got[t]).max() > 0, t
    assert got[ids["cat"]].shape[3] == 384 and got[ids["pa"]].shape[1] == canvas[0] // 2


def test_forward_i8_refuses_unequal_scales_in_a_class():
    p, ids = IC.reduced_pooled_program()
    w, x = IC.reduced_inputs(p, 1, (8, 8))
    s = IC.class_scales(p)
    s[ids["pb"]] *= 2.0
    with pytest.raises(AssertionError, match="carry one scale"):
        quant.forward_i8(p, w, s, {p.input_tensor: quant.quantize(x, s[p.input_tensor])})


# ---------------------------------------------------------------------------------------------- 3. the quantiser is monotone
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("scale", [0.03125, 0.0173, 1.0])
def test_quantise_then_pool_equals_pool_then_quantise(stride, scale):
    """clamp(rint(x * inv)) is monotone non-decreasing in x, so the largest of a window quantises to the largest of the quantised window:
    a pool may keep its source's scale.  Rounding ties (x * inv = k + 0.5, exact for the power-of-two scale), values far beyond +-127
    scales, windows that are all negative."""
    rng = np.random.default_rng(17)
    shape = (2, 12, 10, 32)
    s = np.float32(scale)
    x = (rng.standard_normal(shape) * 40 * s).astype(np.float32)
    ties = ((rng.integers(-130, 130, shape) + 0.5) * s).astype(np.float32)
    x = np.where(rng.random(shape) < 0.3, ties, x)
    x = np.where(rng.random(shape) < 0.1, np.float32(1e4) * s * rng.choice([-1, 1], shape), x).astype(np.float32)
    x[:, :4] = -np.abs(x[:, :4]) - s                 # all-negative windows
    x[:, 4:6] = np.float32(-1e4) * s                 # ... and windows wholly below -127 scales
    x = x.astype(np.float16).astype(np.float32)      # what the device quantises: fp16 values
    a = quant.quantize(maxpool2x2_ref(x, stride), s)
    b = maxpool2x2_ref(quant.quantize(x, s), stride)
    assert a.dtype == b.dtype == np.int8 and np.array_equal(a, b)
    assert a.min() == -127 and a.max() == 127 and (a[:, :1] < 0).all()
    if scale == 0.03125:
        assert (np.abs(x / s - np.rint(x / s)) == 0.5).sum() > 100      # the ties survived fp16


def test_maxpool_ref_on_int8_compares_signed_bytes():
    for shape, strides in IC.POOL_SHAPES[:4]:
        for kind in IC.POOL_DATA:
            x = IC.pool_data_i8(shape, kind)
            for st in strides:
                assert np.array_equal(maxpool2x2_ref(x, st), TC.maxpool_loop(x, st)) and maxpool2x2_ref(x, st).dtype == np.int8
    x = IC.pool_data_i8((1, 4, 8, 16), "positions")      # every window position wins in every byte lane
    win = x.reshape(1, 2, 2, 4, 2, 16).transpose(0, 1, 3, 2, 4, 5).reshape(1, 2, 4, 4, 16).argmax(axis=3)
    assert all(set(win[..., c].ravel().tolist()) == {0, 1, 2, 3} for c in range(16))
    assert (IC.pool_data_i8((1, 2, 2, 16), "negative") < 0).all() and IC.pool_data_i8((2, 13, 13, 512), "random").min() == -128


# ---------------------------------------------------------------------------------------------- 4. bindings
def test_new_entries_are_bound_and_refuse_null():
    lib = _lib.load()
    for name in ("y3_net_set_pools_i8", "y3_net_pools_i8"):
        assert name in _lib.SYMBOLS and not getattr(getattr(lib, name), "missing", False)
        assert name in open(os.path.join(ROOT, "include", "y3.h")).read()
    assert lib.y3_net_set_pools_i8(None, 1) == _lib.Y3_ERR_INVALID
    assert b"y3_net_set_pools_i8" in lib.y3_last_error()
    assert lib.y3_net_pools_i8(None) == 0


def test_maxpool_entry_takes_int8_and_keeps_the_16_byte_rule():
    lib = _lib.load()
    buf = (C.c_char * 64)()
    ptr = C.c_void_p((C.addressof(buf) + 15) & ~15)
    st = lib.y3_maxpool2x2(ptr, ptr, 1, 2, 2, 8, 2, _lib.Y3_DTYPE_I8, None)
    assert st == _lib.Y3_ERR_INVALID and b"8 channels of 1 bytes are no multiple of 16 bytes" in lib.y3_last_error()
    assert lib.y3_maxpool2x2(None, ptr, 1, 2, 2, 16, 2, _lib.Y3_DTYPE_I8, None) == _lib.Y3_ERR_INVALID
    assert lib.y3_maxpool2x2(ptr, ptr, 1, 2, 2, 16, 2, 6, None) == _lib.Y3_ERR_INVALID and b"Y3_DTYPE_I8" in lib.y3_last_error()
    assert lib.y3_maxpool2x2(ptr, ptr, 1, 3, 2, 16, 2, _lib.Y3_DTYPE_I8, None) == _lib.Y3_ERR_INVALID and b"even extents" in lib.y3_last_error()


def test_python_surface_of_the_switch():
    from yolo_v3_tf2_amd import net as N
    from yolo_v3_tf2_amd.core.parse_model import ParseModel
    assert issubclass(N.Net, N._PoolsI8Switch) and "set_pools_i8" not in vars(N.Net) and "pools_i8" not in vars(N.Net)
    assert [N.Net._pools_i8_arg(v) for v in (None, False, True, 0, 1)] == [0, 0, 1, 0, 1]
    with pytest.raises(_lib.Y3Error, match="pools_i8"):
        N.Net._pools_i8_arg(2)
    model = ParseModel().create_model(80, TC.TINY_MODEL)
    assert model.pools_i8 == 0
    model.set_pools_i8()
    assert model.pools_i8 == 1
    model.set_pools_i8(None)
    assert model.pools_i8 == 0
    with pytest.raises(_lib.Y3Error):
        model.set_pools_i8("yes")


def test_packaged_tiny_i8_config_and_the_untouched_tiny_config():
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config/detect_config_tiny_i8.yaml")))
    assert cfg["dtype"] == "i8" and cfg["i8_pools"] is True and cfg["tiny_fused_stem"] is True and cfg["i8_calibration"]
    assert cfg["model_config_file"] == "config/models/yolov3_tiny/model.yaml"
    old = yaml.safe_load(open(os.path.join(ROOT, "config/detect_config_tiny.yaml")))
    assert "i8_pools" not in old and old.get("dtype") is None


# ---------------------------------------------------------------------------------------------- 5. accuracy
# Recorded by `tools/i8_accuracy.py --model tiny` ("YOLOv3-tiny in int8"): head-logit relative L2 of quant.forward_i8 against the
# fp32 oracle on the synthetic tiny network at 2 x 96^2, weight seed 4321, input seed 1234, absmax calibration, per head
RECORDED_REL_L2 = (4.069e-03, 3.962e-03)


def test_accuracy_of_tiny_in_int8_is_pinned(tiny):
    """A later change to the scheme that loses accuracy fails here: 1.5 x what was recorded (room for seed and BLAS order, as for YOLOv3
    in tests/test_i8_host.py)."""
    from yolo_v3_tf2_amd.weights import synthetic_weights
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import i8_accuracy
    x = np.random.default_rng(1234).random((2, 96, 96, 3), dtype=np.float32)
    _, rel = i8_accuracy.measure_pooled(tiny, synthetic_weights(tiny, seed=4321), x, percentiles=(100.0,))[100.0]
    print("tiny int8 absmax head-logit rel L2 vs the fp32 oracle:", " ".join(f"{v:.3e}" for v in rel))
    assert len(rel) == 2
    for got, rec in zip(rel, RECORDED_REL_L2):
        assert got <= 1.5 * rec, (got, rec)
