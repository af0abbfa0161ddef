"""The fp16 fused stem and the fp16 split-K switches, host side, no GPU (include/y3.h: y3_net_set_stem_fusion_f16, y3_net_set_low_latency_f16,
y3_net_set_split_k_f16, y3_net_get_split_k_f16).

The stem: a NumPy restatement of the kernel's conv0 arithmetic (tests/f16_stem_cases.py) on the weights and images of the GPU cases, pushed
through conv1 by the fp16-emulating oracle.  It fixes the two caps of tests/test_f16_stem_gpu.py by the rule of tests/test_f16_host.py: a cap
means something only if the reference ALONE -- no device in sight -- stays within half of it.  Three reference-alone comparisons stand for
the three the GPU test makes: the restatement against the oracle (fused against oracle), the oracle summing in double against itself
summing in fp32 (a second pipeline with another order of the same sums: two-launch against oracle), the restatement against the
double-summing oracle (fused against two-launch).  Measured here over the seven GPU cases: at most 8.48e-3 of conv1's elements differ at
all (the 16,384 elements of the 32 x 32 case; 2.0e-3 .. 4.1e-3 in the larger ones) and at most 3.66e-4 by more than their own fp16 ulp."""
import os
import re

import numpy as np
import pytest

from tests import f16_stem_cases as C
from tests.f16_oracle import round_f16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The GPU caps (tests/test_f16_stem_gpu.py imports them): twice the worst reference-alone figure above.
STEM_DIFFER_CAP = 1.7e-2      # fraction of conv1's stored elements that differ at all
STEM_BEYOND_CAP = 7.4e-4      # ... that differ by more than the element's own fp16 ulp (+ 1e-5 of the layer's scale)


@pytest.mark.parametrize("case,variant", C.GPU_CASES)
def test_reference_alone_stays_within_half_of_the_gpu_caps(case, variant):
    r = C.references(case, variant)
    scale = float(np.abs(r["oracle"]).max())
    assert all(np.isfinite(a).all() and np.array_equal(round_f16(a), a) for a in r.values())
    for what, a, b in (("restated vs oracle", r["restated"], r["oracle"]), ("oracle, double vs fp32 sums", r["oracle64"], r["oracle"]),
                       ("restated vs oracle with double sums", r["restated"], r["oracle64"])):
        frac, beyond, worst = C.compare(a, b, scale)
        print(f"{case} {variant}, {what}: {frac:.3e} of the elements differ, {beyond:.3e} by more than their own ulp, worst {worst:.3f} of "
              f"(ulp + 2^-11 of the scale {scale:.3g})")
        assert frac <= STEM_DIFFER_CAP / 2 and beyond <= STEM_BEYOND_CAP / 2, (what, frac, beyond)
        assert worst <= 1.0, (what, worst)


def test_small_weights_variant_is_the_same_numbers():
    """conv0's weights x 2^-16 with gamma x 2^16: the normalisation brings them back, bit for bit, all the way through conv1."""
    a, b = C.references(C.VARIANT_CASE, "plain"), C.references(C.VARIANT_CASE, "w_small")
    assert np.array_equal(a["restated"], b["restated"])
    _, w, _ = C.stem_inputs(C.VARIANT_CASE, "plain")
    _, ws, _ = C.stem_inputs(C.VARIANT_CASE, "w_small")
    (n, e), (ns, es) = C.normalise_w0(w["conv0.w"]), C.normalise_w0(ws["conv0.w"])
    assert np.array_equal(n, ns) and np.array_equal(e - 16, es)


def test_conv0_sums_are_fp32_class():
    """The split sums against double on the 64 x 64 case: closer than sequential fp32 accumulation gets, far closer than fp16 products."""
    _, w, x = C.stem_inputs(C.VARIANT_CASE, "plain")
    w28, e = C.normalise_w0(w["conv0.w"])
    got = C.conv0_sums(x, w28).astype(np.float64)
    xp = np.zeros((x.shape[0], x.shape[1] + 2, x.shape[2] + 2, 3))
    xp[:, 1:-1, 1:-1] = x
    H, W = x.shape[1:3]
    cols = np.stack([xp[:, u:u + H, v:v + W, c] for u in range(3) for v in range(3) for c in range(3)], axis=-1)
    ref = cols @ w28[:27].astype(np.float64)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"conv0 split sums vs double: max error {err:.2e} of the largest sum")
    assert err < 2e-6                      # 27 products of 2^-22 relative error each and the fp32 roundings of the accumulator


def test_weight_normalisation_is_exact():
    rng = np.random.default_rng(3)
    w = (rng.standard_normal((3, 3, 3, 32)) * np.exp2(rng.integers(-30, 20, 32))[None, None, None, :]).astype(np.float32)
    w[..., 5] = 0.0                                                    # an all-zero channel
    w[..., 6] = np.float32(1.0)                                        # already at the lower end of [1, 2)
    w[1, 1, 1, 7] = np.float32(2.0) - np.float32(2.0 ** -23)           # largest magnitude just below 2: stays
    w28, e = C.normalise_w0(w)
    assert w28.shape == (28, 32) and not w28[27].any() and e[5] == 0 and not w28[:, 5].any() and e[6] == 0
    assert np.array_equal(np.ldexp(w28[:27], e[None, :]).astype(np.float32), w.reshape(27, 32))      # w' * 2^e == w, bit for bit
    mx = np.abs(w28).max(axis=0)
    live = np.arange(32) != 5
    assert (mx[live] >= 1.0).all() and (mx[live] < 2.0).all()
    scale = rng.standard_normal(32).astype(np.float32)
    scale_k = np.ldexp(scale, e).astype(np.float32)                    # the kernel's own scale array
    assert np.array_equal(np.ldexp(scale_k, -e).astype(np.float32), scale)


def test_split_reproduces_the_value():
    rng = np.random.default_rng(4)
    mag = np.exp2(rng.uniform(-14, 15.99, 200000))
    v = (mag * rng.choice([-1.0, 1.0], mag.size)).astype(np.float32)
    v = np.concatenate([v, np.float32([2.0 ** -14, -2.0 ** -14, 65504.0, -65504.0, 1.0, 255.0])])
    hi, lo = C.split_f16(v)
    assert np.array_equal(round_f16(hi), hi) and np.array_equal(round_f16(lo), lo)
    assert (np.abs(hi) >= 2.0 ** -14).all()                            # hi is never subnormal ...
    back = hi.astype(np.float64) + lo.astype(np.float64) * 2.0 ** -11
    assert (np.abs(back - v) <= 2.0 ** -22 * np.abs(v)).all()
    small = (np.exp2(rng.uniform(-40, -14, 100000)) * rng.choice([-1.0, 1.0], 100000)).astype(np.float32)
    small = small[np.abs(small) < 2.0 ** -14]
    small = np.concatenate([small, np.float32([0.0, -0.0, np.nextafter(np.float32(2.0 ** -14), np.float32(0))])])
    hi, lo = C.split_f16(small)
    assert not hi.any()                                                # ... the hi = 0 rule
    assert (np.abs(lo.astype(np.float64) * 2.0 ** -11 - small) <= 2.0 ** -25).all()
    # a subnormal lo' stands for less than 2^-25: flushing it cannot matter more than that
    hi, lo = C.split_f16(v)
    sub = (lo != 0) & (np.abs(lo) < 2.0 ** -14)
    assert (np.abs(lo[sub].astype(np.float64)) * 2.0 ** -11 < 2.0 ** -25).all()


def test_entry_points_are_declared_and_bound():
    from yolo_v3_tf2_amd import _lib, runtime
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "y3.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("y3_net_set_stem_fusion_f16", "y3_net_set_low_latency_f16", "y3_net_set_split_k_f16", "y3_net_get_split_k_f16"):
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
    for name in ("set_stem_fusion_f16", "set_low_latency_f16", "set_split_k_f16", "split_k_f16"):
        assert callable(getattr(runtime.Net, name)), name


def test_null_net_is_refused_by_the_library():
    """Argument refusals of the C entry points that need no device: a null net."""
    from yolo_v3_tf2_amd import _lib
    lib = _lib.load()
    assert lib.y3_net_set_stem_fusion_f16(None, 1) != 0 and b"y3_net_set_stem_fusion_f16" in lib.y3_last_error()
    assert lib.y3_net_set_low_latency_f16(None, 1) != 0 and b"y3_net_set_low_latency_f16" in lib.y3_last_error()
    assert lib.y3_net_set_split_k_f16(None, 0, 2) != 0 and b"y3_net_set_split_k_f16" in lib.y3_last_error()
    assert lib.y3_net_get_split_k_f16(None, 0) == 1


def test_python_argument_checks():
    """The checks run before the library is touched, so an object without a device net shows them."""
    from yolo_v3_tf2_amd import runtime
    Net, Y3Error = runtime.Net, runtime.Y3Error
    assert [Net._stem_fusion_arg(v) for v in (None, False, True, 0, 1, 2, np.int64(2))] == [0, 0, 1, 0, 1, 2, 2]
    for bad in (3, -1, "on", 1.0, [1]):
        with pytest.raises(Y3Error, match="stem fusion"):
            Net._stem_fusion_arg(bad)
    net = Net.__new__(Net)          # no device object: every call below must raise before it would need one
    net.conv_ops = [object()] * 3
    net._h = None
    with pytest.raises(Y3Error, match="stem fusion"):
        net.set_stem_fusion_f16(3)
    with pytest.raises(Y3Error, match="split_k"):
        net.set_split_k_f16(0, 0)
    for bad_slot in (-1, 3, 1.0, None, True):
        with pytest.raises(Y3Error, match="conv slot"):
            net.set_split_k_f16(bad_slot, 2)
        with pytest.raises(Y3Error, match="conv slot"):
            net.split_k_f16(bad_slot)
    with pytest.raises(Y3Error, match="low_latency"):
        net.set_low_latency_f16("on")


def test_model_remembers_the_switches_until_the_device_net_exists(program):
    from yolo_v3_tf2_amd.core.parse_model import YoloModel
    from yolo_v3_tf2_amd.runtime import Y3Error
    m = YoloModel(program)
    assert m.stem_fusion_f16 == 0 and m.low_latency_f16 is False
    m.set_stem_fusion_f16(True)
    m.set_low_latency_f16(True)
    assert m.stem_fusion_f16 == 1 and m.low_latency_f16 is True and m._net is None
    m.set_stem_fusion_f16(None)
    m.set_low_latency_f16(None)
    assert m.stem_fusion_f16 == 0 and m.low_latency_f16 is False
    with pytest.raises(Y3Error):
        m.set_stem_fusion_f16(3)


@pytest.mark.parametrize("value,want", [(None, 0), (False, 0), (True, 1)])
def test_inference_build_accepts_and_forwards_the_key(weights, tmp_path, monkeypatch, value, want):
    import inspect
    import yaml
    from yolo_v3_tf2_amd.inference import Inference
    for name in ("config/detect_config_coco.yaml",):
        cfg = yaml.safe_load(open(os.path.join(ROOT, name)))
        assert cfg.get("f16_fused_stem") is None                      # the packaged config leaves it off; a YAML without the key works too
    assert inspect.signature(Inference.build).parameters["f16_fused_stem"].default is None and Inference.f16_fused_stem is None
    assert "f16_fused_stem" not in inspect.signature(Inference.__call__).parameters      # __call__ keeps the packaged config's keys
    monkeypatch.chdir(tmp_path)                                       # build() writes model_inference_summary.txt
    kw = {} if value is None else {"f16_fused_stem": value}
    model, _ = Inference().build(os.path.join(ROOT, cfg["model_config_file"]), os.path.join(ROOT, cfg["classes_name_file"]),
                                 os.path.join(ROOT, cfg["anchors_file"]), None, 100, 0.5, 0.1, weights=weights, dtype="f16", **kw)
    assert model.model.stem_fusion_f16 == want and model.model._net is None
    inf = Inference()
    inf.f16_fused_stem = value                                         # the way main() hands the YAML key over
    model, _ = inf.build(os.path.join(ROOT, cfg["model_config_file"]), os.path.join(ROOT, cfg["classes_name_file"]),
                         os.path.join(ROOT, cfg["anchors_file"]), None, 100, 0.5, 0.1, weights=weights, dtype="f16")
    assert model.model.stem_fusion_f16 == want
    with pytest.raises(Exception, match="stem fusion"):
        Inference().build(os.path.join(ROOT, cfg["model_config_file"]), os.path.join(ROOT, cfg["classes_name_file"]),
                          os.path.join(ROOT, cfg["anchors_file"]), None, 100, 0.5, 0.1, weights=weights, f16_fused_stem="yes")
