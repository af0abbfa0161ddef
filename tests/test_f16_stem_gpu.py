"""The fused stem kernel in fp16 plans (csrc/conv_stem.hip, conv_stem16<F16Elem>; y3_net_set_stem_fusion_f16), on the GPU.

conv1's stored fp16 output is read bit for bit through identity 1x1 heads (tests/f16_stem_cases.py) from the fused kernel and from the
one-launch-per-conv form of the same plan, and both are held against the fp16-emulating oracle.  Bars: every element within its own fp16
ulp + 2^-11 of the layer's scale (a conv0 value rounded the other way moves a conv1 sum by |w| x one fp16 ulp of the conv0 value, an
absolute amount however small the element is); the fractions of elements that differ at all and by more than their own ulp within the
caps of tests/test_f16_stem_host.py, twice what the reference alone shows.  Off by default and for fp16 plans only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import f16_stem_cases as C  # noqa: E402
from tests.f16_oracle import round_f16  # noqa: E402
from tests.test_f16_stem_host import STEM_BEYOND_CAP, STEM_DIFFER_CAP  # noqa: E402
from yolo_v3_tf2_amd import _lib  # noqa: E402

F16, BF16 = _lib.Y3_DTYPE_F16, _lib.Y3_DTYPE_BF16


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("case,variant", C.GPU_CASES)
def test_f16_fused_stem_conv0_error_bounded_through_identity_heads(rt, case, variant):
    p, w, x = C.stem_inputs(case, variant)
    canvas, B = C.CASES[case]
    ref = C.references(case, variant)["oracle"]
    xd = _cuda(x)
    outs = {}
    for fused in (True, False):
        net = rt.Net(p)
        net.load_weights(w)
        net.plan(B, canvas, F16)
        net.set_lanes(1)
        ms = net.profile_convs(xd)
        assert ms[0] > 0.0 and ms[1] > 0.0, "an fp16 plan fuses nothing before it is asked to"
        if fused:
            net.set_stem_fusion_f16(2)
        got = net.forward(xd)[0].clone()
        ms = net.profile_convs(xd)
        assert (ms[0] == 0.0) == fused and ms[1] > 0.0, "the fp16 fused stem did not engage" if fused else "fused without the switch"
        again = net.forward(xd)[0]
        torch.cuda.synchronize()
        assert torch.equal(got, again)                                  # the persistent kernel is deterministic
        outs[fused] = got.cpu().numpy().reshape(ref.shape)
        assert np.isfinite(outs[fused]).all() and np.array_equal(round_f16(outs[fused]), outs[fused])
    scale = float(np.abs(ref).max())
    for name, a, b in (("fused vs two-launch", outs[True], outs[False]), ("fused vs oracle", outs[True], ref),
                       ("two-launch vs oracle", outs[False], ref)):
        frac, beyond, worst = C.compare(a, b, scale)
        print(f"f16 stem {case} {variant}, {name}: {frac:.3e} of the elements differ (cap {STEM_DIFFER_CAP:.1e}), {beyond:.3e} by more than "
              f"their own ulp (cap {STEM_BEYOND_CAP:.1e}), worst {worst:.3f} of (ulp + 2^-11 of the scale {scale:.3g})")
        assert worst <= 1.0, (name, worst)
        assert frac <= STEM_DIFFER_CAP and beyond <= STEM_BEYOND_CAP, (name, frac, beyond)


@pytest.mark.parametrize("S,B", [(32, 1), (64, 3), (416, 2)])
def test_f16_fused_stem_third_layer_bit_identical_to_its_own_launch(rt, S, B):
    """Mode 1 (the 64 -> 32 1x1 after conv1 computed from the staged fp16 tile, phase 3) against mode 2 (the 1x1 launched on its own):
    same operands, same MFMA and k grouping, so every head bit for bit; the 1x1 reports no launch of its own in mode 1."""
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    p = mini_program(3, [dict(filters=32, size=3), dict(filters=64, size=3, stride=2), dict(filters=32, size=1),
                         dict(filters=64, size=3, shortcut=-3)],
                     [dict(filters=32, size=1, bn=False, act="linear"), dict(filters=32, size=1, bn=False, act="linear"),
                      dict(filters=64, size=1)])
    w = synthetic_weights(p, seed=13)
    xd = _cuda(np.random.default_rng(13).random((B, S, S, 3), dtype=np.float32))
    outs = {}
    for mode in (1, 2, 0):
        net = rt.Net(p)
        net.load_weights(w)
        net.set_stem_fusion_f16(mode)            # before the plan: the plan takes it up
        net.plan(B, S, F16)
        net.set_lanes(1)
        outs[mode] = [g.clone() for g in net.forward(xd)]
        ms = net.profile_convs(xd)
        assert (ms[0] == 0.0) == (mode != 0), "wrong launch structure for this mode"
        assert (ms[2] == 0.0) == (mode == 1), "the 1x1 third layer: wrong launch structure for this mode"
        again = net.forward(xd)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs[mode], again))
    assert all(torch.equal(a, b) for a, b in zip(outs[1], outs[2])), "phase 3 differs from the stand-alone 1x1 launch"
    for a, b in zip(outs[1], outs[0]):           # two fp16 layers downstream of a few flipped conv0 roundings
        scale = max(1.0, float(b.abs().max()))
        assert float((a - b).abs().max()) <= 2.0 ** -8 * scale and float((a - b).abs().mean()) <= 2.0 ** -12 * scale


# ---------------------------------------------------------------------------------------------- the real network at 64 x 64
def _detect_composed(rt, net, x, anchors):
    grids = [g.clone() for g in net.forward(x)]
    bb, cc, ss = rt.yolo_decode_scores(grids, anchors, 80)
    sel, nv = rt.nms_padded(bb, ss, 100, 0.5, 0.05)
    return grids, (bb, cc, ss), rt.pack_detections(bb, cc, ss, sel, nv), nv


@pytest.mark.parametrize("lanes", [1, 2])
def test_f16_fused_stem_network_routes(rt, program, weights, anchors, lanes):
    """With the switch on: detect and forward_decode are the composed route bit for bit, image 0 of a two-image call is the image alone, and
    the stem's three convs report no launch of their own but conv1's."""
    x = _cuda(np.random.default_rng(41).random((2, 64, 64, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(2, 64, F16)
    net.set_lanes(lanes)
    off = [g.clone() for g in net.forward(x)]
    net.set_stem_fusion_f16(True)
    ms = net.profile_convs(x)
    assert ms[0] == 0.0 and ms[1] > 0.0 and ms[2] == 0.0
    grids, (bb, cc, ss), want, nv = _detect_composed(rt, net, x, anchors)
    assert any(not torch.equal(a, b) for a, b in zip(grids, off))       # another conv0 arithmetic: not the unfused plan's bits
    for a, b in zip(grids, off):
        assert float((a - b).abs().max()) <= 2e-2 * max(1.0, float(b.abs().max()))
    for _ in range(2):
        fb, fc, fs = net.forward_decode(x, anchors)
        packed, nv2 = net.detect(x, anchors, 100, 0.5, 0.05)
        torch.cuda.synchronize()
        assert torch.equal(fb, bb) and torch.equal(fc, cc) and torch.equal(fs, ss)
        assert torch.equal(nv2, nv) and torch.equal(packed, want) and int(nv.sum()) > 0
    g0 = net.forward(x[0:1].contiguous())
    torch.cuda.synchronize()
    assert all(torch.equal(a[0:1], b) for a, b in zip(grids, g0))
    net.set_stem_fusion_f16(0)                                          # and off again is the default plan
    back = net.forward(x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(off, back))


def test_f16_fused_stem_detect_graph_capture(rt, program, weights, anchors):
    x = _cuda(np.random.default_rng(31).random((2, 64, 64, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_stem_fusion_f16(True)
    net.plan(2, 64, F16)
    net.set_lanes(2)
    assert net.profile_convs(x)[0] == 0.0
    packed, nv = net.detect(x, anchors, 100, 0.5, 0.05)
    torch.cuda.synchronize()
    want_p, want_n = packed.clone(), nv.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net.detect(x, anchors, 100, 0.5, 0.05)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gp, gn = net.detect(x, anchors, 100, 0.5, 0.05)
    for _ in range(3):
        gp.zero_()
        gn.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(gn, want_n) and torch.equal(gp, want_p) and int(want_n.sum()) > 0


def test_each_stem_switch_acts_on_its_own_plans_only(rt, program, weights):
    x = _cuda(np.random.default_rng(5).random((1, 64, 64, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(1, 64, F16)
    base = [g.clone() for g in net.forward(x)]
    for mode in (0, 1, 2):                       # y3_net_set_stem_fusion still does nothing to an fp16 plan
        net.set_stem_fusion(mode)
        assert net.profile_convs(x)[0] > 0.0
        got = net.forward(x)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(base, got)), mode
    net.set_stem_fusion(1)
    net.plan(1, 64, BF16)                        # ... and the new switch nothing to a bf16 plan, fused (its default) or not
    for bf16_mode in (1, 0):
        net.set_stem_fusion(bf16_mode)
        want = [g.clone() for g in net.forward(x)]
        for mode in (1, 2, 0):
            net.set_stem_fusion_f16(mode)
            assert (net.profile_convs(x)[0] == 0.0) == (bf16_mode == 1)
            got = net.forward(x)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(want, got)), (bf16_mode, mode)
    with pytest.raises(rt.Y3Error, match="0, 1 or 2"):
        rt.check(net.lib.y3_net_set_stem_fusion_f16(net._h, 3), "y3_net_set_stem_fusion_f16")


def test_f16_fused_stem_carries_the_clock_stamps(rt, program, weights):
    """y3_net_measure_sclk on an fp16 plan: no launch carries stamps until the stem is fused; then a clock between idle and maximum, and
    the measurement leaves no trace."""
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(8, 96, F16)
    x = torch.rand((8, 96, 96, 3), device="cuda")
    g = [t.clone() for t in net.forward(x)]
    scratch = [torch.empty_like(t) for t in g]
    with pytest.raises(rt.Y3Error, match="stamps"):
        net.measure_sclk(x, scratch, forwards=2)
    net.set_stem_fusion_f16(True)
    fused = [t.clone() for t in net.forward(x)]
    mhz = net.measure_sclk(x, scratch, forwards=20)
    assert 100.0 < mhz < 2600.0, mhz
    assert all(torch.equal(a, b) for a, b in zip(fused, net.forward(x)))


def test_split_k_f16_refuses_a_conv_inside_the_fused_stem(rt):
    """The convs of the fp16 fused stem are never split: the first layer and conv1 (Cin = 32, a BK = 32 tile) are refused by name, fused
    or not, and nothing in the plan is split by the switch alone at this size."""
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    p = mini_program(3, [dict(filters=32, size=3), dict(filters=64, size=3, stride=2), dict(filters=64, size=1)],
                     [dict(filters=64, size=1), dict(filters=64, size=1), dict(filters=64, size=1)])
    net = rt.Net(p)
    net.load_weights(synthetic_weights(p, seed=3))
    net.set_stem_fusion_f16(2)
    net.plan(1, 64, F16)
    with pytest.raises(rt.Y3Error, match="first layer"):
        net.set_split_k_f16(0, 2)
    with pytest.raises(rt.Y3Error, match="BK = 32"):
        net.set_split_k_f16(1, 2)
    net.set_low_latency_f16(True)
    assert net.profile_convs(_cuda(np.zeros((1, 64, 64, 3), np.float32)))[0] == 0.0
    assert all(net.split_k_f16(i) == 1 for i in range(len(net.conv_ops)))
