"""The fused stem of YOLOv3-tiny, host side, no GPU (include/y3.h, y3_net_set_tiny_stem_fusion; csrc/conv_tiny_stem.hip): the references of
tests/tiny_stem_cases.py in their three forms, the graph rule on lowered programs, the bindings with the argument refusals that need no
device, and the basis of the caps tests/test_tiny_stem_gpu.py holds the 16-bit device results to."""
import os
import re

import numpy as np
import pytest

from tests import tiny_cases as TC
from tests import tiny_stem_cases as C
from tests.helpers import f32_conv_bar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("case,variant", C.GPU_CASES)
def test_references_in_three_forms(case, variant):
    """fp32 sums, double sums, and rounded per format where a 16-bit pipeline stores: shapes, the formats' exactness, the distance of the two
    unrounded chains under the fp32 bar, and the property each variant is there for."""
    from oracle import oracle as O
    from tests.f16_oracle import round_f16
    (H, W), B = C.CASES[case]
    r = C.references(case, variant)
    assert all(a.shape == (B, H // 4, W // 4, 32) and a.dtype == np.float32 and not a.flags.writeable for a in r.values())
    assert float(np.abs(r["f32"] - r["f64"]).max()) <= f32_conv_bar(r["f64"])
    for fmt, rnd in (("bf16", O.round_bf16), ("f16", round_f16)):
        for name in (fmt, fmt + "_s32"):
            assert np.array_equal(rnd(r[name]), r[name]), "what a 16-bit pipeline stores is exact in its format"
        assert float((r[fmt] != r["f64"]).mean()) > 0.5, "the rounded chain is rounded"
    scale = float(np.abs(r["f64"]).max())
    if variant == "signs":
        assert float((r["f64"] < 0).mean()) > 0.9 and scale > 0.1      # whole pooling windows are negative: a maximum from 0 would be 0
    elif variant == "img255":
        assert scale > 100.0
    else:
        assert 0.2 < float((r["f64"] < 0).mean()) < 0.6 and scale > 1.0


def test_identity_heads_hand_pool_1_over_bit_for_bit():
    """The case program's heads through the oracle: a raw 1x1 conv with [I_32 | 0] and no bias returns its input in channels 0 .. 31, zeros
    behind them, with fp32 and with double sums."""
    from oracle import oracle as O
    p, w, x, p1 = C.stem_inputs("s32_b1")
    pooled = C.references("s32_b1")["f32"]
    for acc64 in (False, True):
        for i in (2, 3):
            y = O.conv_block(pooled, w, i, 1, 1, False, False, acc64)
            assert y.shape[-1] == 64 and np.array_equal(y[..., :32], pooled) and not y[..., 32:].any()
    assert p.tensors[p1].channels == 32 and p.tensors[p1].div == 4 and len(p.outputs) == 2 and p.nclasses == 0


# ---------------------------------------------------------------------------------------------- the graph rule
def test_graph_rule_on_lowered_programs():
    """yes: tiny itself and the case program; no: the pool net of tests/tiny_cases.py (widths 32 / 64) and a tiny stem whose conv0 output
    has a second reader.  The device's rule is the same at the stored widths (tests/test_tiny_stem_gpu.py asks it)."""
    from yolo_v3_tf2_amd.graph import AuxOp, ConvOp, tiny_stem_applicable
    tiny = TC.tiny_program(80)
    assert tiny_stem_applicable(tiny)
    ops = tiny.ops[:4]
    assert [type(o) for o in ops] == [ConvOp, AuxOp, ConvOp, AuxOp] and (ops[0].cout, ops[2].cin, ops[2].cout) == (32, 32, 32)
    assert tiny.tensors[ops[0].dst].channels == 16 and tiny.stored[ops[0].dst] == 32 and tiny.stored[ops[1].dst] == 32
    case, _ = C.stem_program()
    assert tiny_stem_applicable(case)
    pool_net, _ = TC.pool_net_program()
    assert not tiny_stem_applicable(pool_net)
    twice, _ = C.stem_program(second_reader=True)
    c0 = twice.ops[0]
    assert sum(isinstance(o, AuxOp) and o.inputs == [c0.dst] for o in twice.ops) == 2
    assert not tiny_stem_applicable(twice)
    from yolo_v3_tf2_amd.graph import load_program
    assert not tiny_stem_applicable(load_program(os.path.join(ROOT, "config/models/yolov3/model.yaml"), 80))


# ---------------------------------------------------------------------------------------------- bindings and refusals without a device
def test_entry_points_are_declared_and_bound():
    from yolo_v3_tf2_amd import _lib, runtime
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "y3.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("y3_net_set_tiny_stem_fusion", "y3_net_get_tiny_stem_fused"):
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name) and not getattr(getattr(lib, name), "missing", False), name
    assert callable(runtime.Net.set_tiny_stem_fusion) and isinstance(runtime.Net.tiny_stem_fused, property)


def test_null_net_is_refused_by_the_library():
    from yolo_v3_tf2_amd import _lib
    lib = _lib.load()
    assert lib.y3_net_set_tiny_stem_fusion(None, 1) != 0 and b"y3_net_set_tiny_stem_fusion" in lib.y3_last_error()
    assert lib.y3_net_get_tiny_stem_fused(None) == 0


def test_python_argument_checks():
    """The checks run before the library is touched, so an object without a device net shows them."""
    from yolo_v3_tf2_amd import runtime
    Net, Y3Error = runtime.Net, runtime.Y3Error
    assert [Net._tiny_stem_arg(v) for v in (None, False, True, 0, 1, np.int64(1))] == [0, 0, 1, 0, 1, 1]
    for bad in (2, -1, "on", 1.0, [1]):
        with pytest.raises(Y3Error, match="tiny stem fusion"):
            Net._tiny_stem_arg(bad)
    net = Net.__new__(Net)          # no device object: the call must raise before it would need one
    net._h = None
    with pytest.raises(Y3Error, match="tiny stem fusion"):
        net.set_tiny_stem_fusion(2)


def test_model_remembers_the_switch_until_the_device_net_exists():
    from yolo_v3_tf2_amd.core.parse_model import YoloModel
    from yolo_v3_tf2_amd.runtime import Y3Error
    m = YoloModel(TC.tiny_program(80))
    assert m.tiny_stem_fusion == 0
    m.set_tiny_stem_fusion()
    assert m.tiny_stem_fusion == 1 and m._net is None
    m.set_tiny_stem_fusion(None)
    assert m.tiny_stem_fusion == 0
    m.set_stem_fusion_f16(True)
    assert m.tiny_stem_fusion == 0 and m.stem_fusion_f16 == 1, "a switch of its own"
    with pytest.raises(Y3Error):
        m.set_tiny_stem_fusion(2)
    order = list(m._deferred)
    assert order.index("set_tiny_stem_fusion") < order.index("set_dtype"), "the switch reaches the device net before the dtype plans it"


@pytest.mark.parametrize("value,want", [(None, 0), (False, 0), (True, 1)])
def test_drivers_take_the_yaml_key(tmp_path, monkeypatch, value, want):
    """`tiny_fused_stem` of the inference config lands on Inference and from there on the model; the packaged tiny config leaves it off and
    stays fp32; evaluate_yolov3 has the flag."""
    import yaml
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev
    from yolo_v3_tf2_amd.inference import Inference
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config/detect_config_tiny.yaml")))
    assert cfg.get("tiny_fused_stem") is None and cfg.get("dtype") is None
    text = open(os.path.join(ROOT, "config/detect_config_tiny.yaml")).read()
    assert re.search(r"#\s*dtype: bf16", text) and re.search(r"#\s*tiny_fused_stem: true", text), "the commented example"
    assert Inference.tiny_fused_stem is None
    w, _ = TC.tiny_inputs(TC.tiny_program(80), 1, (32, 32))
    monkeypatch.chdir(tmp_path)                                       # build() writes model_inference_summary.txt
    inf = Inference()
    inf.tiny_fused_stem = value                                        # the way main() hands the YAML key over
    model, _ = inf.build(os.path.join(ROOT, cfg["model_config_file"]), os.path.join(ROOT, cfg["classes_name_file"]),
                         os.path.join(ROOT, cfg["anchors_file"]), None, 100, 0.5, 0.1, weights=w, dtype="bf16")
    assert model.model.tiny_stem_fusion == want and model.model.dtype == 1 and model.model._net is None
    a = ev._arg_parser().parse_args(["--on-device", "--tiny-fused-stem"])
    assert a.tiny_fused_stem is True and ev._arg_parser().parse_args([]).tiny_fused_stem is False


def test_time_tiny_has_the_two_options():
    text = open(os.path.join(ROOT, "tools", "time_tiny.py")).read()
    assert '"--dtype"' in text and '("f32", "bf16", "f16")' in text and '"--fused-stem"' in text


# ---------------------------------------------------------------------------------------------- the caps' basis
def test_caps_are_twice_what_the_reference_alone_reaches():
    """Per 16-bit format and case: the fraction of pool-1 elements on which the fp32-sum oracle chain and the double-sum chain differ at all,
    and by more than the element's own ulp + 1e-5 of the tensor's magnitude; no element beyond the per-element bound.  The caps of the GPU
    test are twice the largest such figure over the cases -- the reference alone stays within half the cap, and the cap is no wider."""
    for fmt in C.FORMATS:
        largest = [0.0, 0.0]
        for case, variant in C.GPU_CASES:
            r = C.references(case, variant)
            differ, beyond, worst = C.compare(fmt, r[fmt + "_s32"], r[fmt])
            print(f"{fmt} {case} / {variant}: differ {differ:.4e}  beyond one ulp {beyond:.4e}  worst {worst:.3f} of the per-element bound")
            assert differ <= C.CAPS[fmt][0] / 2 and beyond <= C.CAPS[fmt][1] / 2 and worst <= 1.0, (fmt, case, variant, differ, beyond, worst)
            largest = [max(largest[0], differ), max(largest[1], beyond)]
        for k in (0, 1):
            assert C.CAPS[fmt][k] == 2.0 * C.LARGEST[fmt][k]
            assert 0.999 * C.LARGEST[fmt][k] <= largest[k] <= C.LARGEST[fmt][k], (fmt, k, largest[k], "the constant is the measured figure, rounded up")
