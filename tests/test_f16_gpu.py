"""fp16 plans (Y3_DTYPE_F16) on the GPU: the fp16 instantiations of the 16-bit conv kernels (csrc/conv_f16.hip, csrc/conv_res_f16.hip),
conv_first / to_f32 in fp16, and the host layer around them, against the fp16-emulating oracle (tests/f16_oracle.py).

Bars: the project's per-layer ones with fp16 in place of bf16 -- an fp32 head fed fp16 inputs within 2e-5 * max(1, |ref|max); a stored
fp16 output within f16_ulp_elem + 1e-5 |ref|max of round_f16(reference), the reference accumulating in double.  The caps on the fraction
of elements that differ at all are twice what the reference alone shows when it sums in fp32 instead (tests/test_f16_host.py)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.f16_oracle import f16_emulation, f16_ulp_elem, free_running_floor, rel_l2, round_f16  # noqa: E402
from tests.helpers import check_f32_conv, mini_program, oracle_launch, unfolded_program  # noqa: E402
from yolo_v3_tf2_amd import _lib  # noqa: E402

F16, BF16 = _lib.Y3_DTYPE_F16, _lib.Y3_DTYPE_BF16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stored_check(got, ref, cap, what):
    """A stored fp16 output against round_f16 of the double-accumulating reference: -> (worst fraction of the bar, differing fraction)."""
    assert np.array_equal(round_f16(got), got), what
    exp = round_f16(ref)
    diff = np.abs(got.astype(np.float64) - exp.astype(np.float64))
    bar = f16_ulp_elem(got, exp) + 1e-5 * float(np.abs(exp).max())
    frac = float((diff > 0).mean())
    assert (diff <= bar).all(), (what, float((diff / bar).max()))
    assert frac <= cap, (what, frac)
    return float((diff / bar).max()), frac


# ---------------------------------------------------------------------------------------------- 2. weight-resident tile 32
@pytest.mark.parametrize("cin,cout,S,B", [(32, 64, 40, 3), (64, 128, 36, 2), (64, 64, 33, 2), (32, 128, 70, 1)])
def test_f16_weight_resident_3x3_matches_oracle_and_generic_tiles(rt, cin, cout, S, B):
    """Tile id 32 in an fp16 plan (csrc/conv_res_f16.hip), the shapes of test_bf16_weight_resident_3x3_matches_oracle_and_generic_tiles:
    with and without a shortcut, BN + leaky and linear + bias, ragged last tile columns and rows, several images (one tile per
    persistent workgroup at these shapes; walks of three tiles: tests/test_persistent_walk_gpu.py).  Every 3x3 launch
    against the fp16 oracle on its own device inputs, and the whole net bit for bit against the generic tile of the same MFMA shape."""
    from oracle import oracle as O
    from yolo_v3_tf2_amd.weights import synthetic_weights
    chain = [dict(filters=cout, size=3), dict(filters=cin, size=1), dict(filters=cout, size=3, shortcut=-3),
             dict(filters=cin, size=1, act="linear"), dict(filters=cout, size=3, bn=False, act="linear")]
    heads = [dict(filters=64, size=1), dict(filters=32, size=1), dict(filters=64, size=1, bn=False, act="linear")]
    p = mini_program(cin, chain, heads)
    w = synthetic_weights(p, seed=52)
    x = round_f16(np.random.default_rng(52).standard_normal((B, S, S, cin)).astype(np.float32))
    stored = [o.dst for o in p.conv_ops() if o.dst not in p.outputs]
    xin = _cuda(x).to(torch.float16)
    outs, mids = {}, {}
    for name, tile in (("resident", 32), ("generic", 5 if cin == 32 else 10)):
        net = rt.Net(p)
        net.load_weights(w)
        net.keep_activations(True)
        for slot, o in enumerate(net.conv_ops):
            if o.size == 3:
                net.set_tile_bf16(slot, tile)
        net.plan(B, S, F16)
        outs[name] = [g.clone() for g in net.forward(xin)]
        mids[name] = [net.read_tensor(t, B).clone() for t in stored]
        again = net.forward(xin)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs[name], again))
    for a, b in zip(mids["resident"] + outs["resident"], mids["generic"] + outs["generic"]):
        assert torch.equal(a, b)
    dev = {t: g.cpu().numpy() for t, g in zip(stored, mids["resident"])}
    dev[p.input_tensor] = x
    n3 = 0
    for o in p.conv_ops():
        if o.size != 3:
            continue
        with f16_emulation():
            ref = oracle_launch(O, o, w, dev.__getitem__, acc64=True, bf16_weights=True)
        worst, frac = _stored_check(dev[o.dst], ref, 1e-2, (cin, cout, S, o.conv_index))
        print(f"f16 weight-resident {cin}->{cout} @{S} x{B} conv {o.conv_index}: worst {worst:.3f} of the bar, {frac:.2e} of the elements differ")
        n3 += 1
    assert n3 == 3


# ---------------------------------------------------------------------------------------------- 3. every layer, teacher-forced
def test_f16_every_layer_teacher_forced(rt, program, weights):
    """The body of test_bf16_every_layer_teacher_forced_within_one_ulp with round_f16 and a double-accumulating reference: every fused
    launch of the real network recomputed by the oracle from the device's own input tensors."""
    from oracle import oracle as O
    S, B = 96, 2
    x = np.random.default_rng(31).random((B, S, S, 3), dtype=np.float32)
    net = rt.Net(program)
    net.load_weights(weights)
    net.keep_activations(True)
    net.plan(B, S, F16)
    grids = net.forward(_cuda(x))
    torch.cuda.synchronize()
    outs = {t: g.cpu().numpy().reshape(B, g.shape[1], g.shape[2], -1) for t, g in zip(program.outputs, grids)}
    cache = {}

    def dev(t):
        if t == program.input_tensor:
            return x
        if t not in cache:
            cache[t] = net.read_tensor(t, B).cpu().numpy()
        return cache[t]

    worst_bar, worst_frac, worst_head = 0.0, 0.0, 0.0
    for o in program.conv_ops():
        with f16_emulation():       # the Cin = 3 first layer is fp32 arithmetic on fp32 weights
            y = oracle_launch(O, o, weights, dev, acc64=True, bf16_weights=(o.cin != 3))
        if o.dst in outs:                                   # head conv: fp32 straight from the accumulators
            err, bar = check_f32_conv(outs[o.dst], y, o.conv_index)
            worst_head = max(worst_head, err / bar)
            continue
        w_, f_ = _stored_check(dev(o.dst), y, 1.2e-2, o.conv_index)
        worst_bar, worst_frac = max(worst_bar, w_), max(worst_frac, f_)
    print(f"f16 teacher-forced, real network 2 x 96^2: worst stored element {worst_bar:.3f} of the bar, worst differing fraction "
          f"{worst_frac:.2e} (cap 1.2e-2), worst fp32 head {worst_head:.3f} of the 2e-5 bar")


# ---------------------------------------------------------------------------------------------- 4. free running
def test_f16_network_free_running(rt, program, weights):
    """The whole network in fp16, free running: no further from the fp16 oracle than twice (relative L2) / three times (max abs) what the
    oracle is from itself under double accumulation -- the floor, computed here -- and every head closer to the fp32 oracle than the
    bf16-emulating oracle is.  The bf16 plan's distances on the same input are printed beside it."""
    S, B = 96, 2
    x = np.random.default_rng(1234).random((B, S, S, 3), dtype=np.float32)
    r = free_running_floor(program, weights, x)
    net = rt.Net(program)
    net.load_weights(weights)
    got = {}
    for tag, dt in (("f16", F16), ("bf16", BF16)):
        net.plan(B, S, dt)
        got[tag] = [g.cpu().numpy() for g in net.forward(_cuda(x))]
    for k in range(3):
        g, gb = got["f16"][k], got["bf16"][k]
        rel16, max16 = rel_l2(g, r["f16"][k]), float(np.abs(g - r["f16"][k]).max())
        rel32, max32 = rel_l2(g, r["f32"][k]), float(np.abs(g - r["f32"][k]).max())
        orc_bf = rel_l2(r["bf16"][k], r["f32"][k])
        print(f"f16 free running head {k}: device vs fp16 oracle rel {rel16:.3e} max {max16:.3e} (floor rel {r['floor_rel'][k]:.3e} max "
              f"{r['floor_max'][k]:.3e}); device vs fp32 oracle rel {rel32:.3e} max {max32:.3e}; bf16 oracle vs fp32 oracle rel {orc_bf:.3e}; "
              f"bf16 device vs fp32 oracle rel {rel_l2(gb, r['f32'][k]):.3e} max {float(np.abs(gb - r['f32'][k]).max()):.3e}")
        assert np.isfinite(g).all()
        assert 2e-4 < r["floor_rel"][k] < 2e-3
        assert rel16 <= 2.0 * r["floor_rel"][k] and max16 <= 3.0 * r["floor_max"][k], (k, rel16, max16)
        assert rel32 < orc_bf, (k, rel32, orc_bf)


# ---------------------------------------------------------------------------------------------- 5. routes
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("canvas", [64, (64, 96)], ids=["64", "64x96"])
def test_f16_detect_and_forward_decode_equal_the_composed_route(rt, program, weights, anchors, canvas, lanes):
    """detect and forward_decode (the head convs decode in their own tiles) are the composed route bit for bit; image 0 of a two-image
    call is the image alone."""
    H, W = rt.canvas_hw(canvas)
    B = 2
    x = _cuda(np.random.default_rng(41).random((B, H, W, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(B, canvas, F16)
    net.set_lanes(lanes)
    assert net.dtype == F16
    grids = [g.clone() for g in net.forward(x)]
    bb, cc, ss = rt.yolo_decode_scores(grids, anchors, 80)
    sel, nv = rt.nms_padded(bb, ss, 100, 0.5, 0.05)
    want = rt.pack_detections(bb, cc, ss, sel, nv)
    for _ in range(2):
        fb, fc, fs = net.forward_decode(x, anchors)
        packed, nv2 = net.detect(x, anchors, 100, 0.5, 0.05)
        torch.cuda.synchronize()
        assert torch.equal(fb, bb) and torch.equal(fc, cc) and torch.equal(fs, ss)
        assert torch.equal(nv2, nv) and torch.equal(packed, want) and int(nv.sum()) > 0
    g0 = net.forward(x[0:1].contiguous())
    torch.cuda.synchronize()
    assert all(torch.equal(a[0:1], b) for a, b in zip(grids, g0))
    p0, n0 = net.detect(x[0:1].contiguous(), anchors, 100, 0.5, 0.05)
    assert torch.equal(p0, want[0:1]) and torch.equal(n0, nv[0:1])


def test_f16_detect_graph_capture(rt, program, weights, anchors):
    """A captured detect on an fp16 plan, two lanes, replayed three times, equals eager."""
    x = _cuda(np.random.default_rng(31).random((2, 64, 64, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(2, 64, F16)
    net.set_lanes(2)
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


def test_f16_heuristic_tiles_same_bits_at_batch_1_and_3(rt, program, weights, monkeypatch):
    """Without a tuning table: an image's bits depend neither on the batch of the call nor on the batch of the plan."""
    monkeypatch.setenv("Y3_NO_TUNING", "1")
    x = _cuda(np.random.default_rng(11).random((3, 64, 64, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(3, 64, F16)
    a = [g.clone() for g in net.forward(x)]
    for i in range(3):
        gi = net.forward(x[i:i + 1].contiguous())
        torch.cuda.synchronize()
        assert all(torch.equal(u[i:i + 1], v) for u, v in zip(a, gi)), i
    one = rt.Net(program)
    one.load_weights(weights)
    one.plan(1, 64, F16)
    g1 = one.forward(x[1:2].contiguous())
    torch.cuda.synchronize()
    assert all(torch.equal(u[1:2], v) for u, v in zip(a, g1))


# ---------------------------------------------------------------------------------------------- 6. edges
def test_f16_overflow_stores_inf(rt):
    """IEEE overflow, no saturation: a conv whose BN scale drives outputs beyond 65504 stores inf where round_f16 of the reference does
    (elements whose reference lies within 1e-5 of the 65520 boundary are left out: their side follows the summation order), and what
    stays finite stays within the bar."""
    from oracle import oracle as O
    from yolo_v3_tf2_amd.weights import synthetic_weights
    p = mini_program(64, [dict(filters=64, size=3)], [dict(filters=64, size=1), dict(filters=32, size=1), dict(filters=64, size=1)])
    w = dict(synthetic_weights(p, seed=9))
    B, S = 2, 12
    x = round_f16(np.random.default_rng(9).standard_normal((B, S, S, 64)).astype(np.float32))
    op = p.conv_ops()[0]
    plain = oracle_launch(O, op, w, {p.input_tensor: x}.__getitem__)
    w["conv0.gamma"] = (w["conv0.gamma"] * np.float32(4 * 65504.0 / np.abs(plain).max())).astype(np.float32)   # the largest output at 4 x the limit
    w["conv0.beta"] = np.zeros_like(w["conv0.beta"])
    net = rt.Net(p)
    net.load_weights(w)
    net.keep_activations(True)
    net.plan(B, S, F16)
    net.forward(_cuda(x).to(torch.float16))
    got = net.read_tensor(op.dst, B).cpu().numpy()
    with f16_emulation():
        ref = oracle_launch(O, op, w, {p.input_tensor: x}.__getitem__, acc64=True, bf16_weights=True)
    exp = round_f16(ref)
    clear = np.abs(np.abs(ref) / 65520.0 - 1.0) > 1e-5
    n_inf = int(np.isinf(exp).sum())
    print(f"f16 overflow: {n_inf} of {exp.size} reference elements are inf, largest finite {np.abs(exp[np.isfinite(exp)]).max():.0f}")
    assert 0.01 * exp.size < n_inf < 0.9 * exp.size                      # both sides of the limit are exercised
    assert np.array_equal(np.isinf(got)[clear], np.isinf(exp)[clear]) and not np.isnan(got).any()
    assert np.array_equal(np.sign(got[np.isinf(got) & clear]), np.sign(exp[np.isinf(got) & clear]))
    fin = np.isfinite(got) & np.isfinite(exp)
    diff = np.abs(got[fin].astype(np.float64) - exp[fin].astype(np.float64))
    bar = f16_ulp_elem(got[fin], exp[fin]) + 1e-5 * float(np.abs(exp[fin]).max())
    assert (diff <= bar).all(), float((diff / bar).max())


def test_f16_plans_never_split_and_never_fuse_the_stem(rt, program, weights):
    x = _cuda(np.random.default_rng(5).random((1, 64, 64, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_low_latency_bf16(True)
    net.plan(1, 64, F16)
    assert all(net.split_k_bf16(i) == 1 and net.split_k(i) == 1 for i in range(len(net.conv_ops)))
    slot = next(i for i, o in enumerate(net.conv_ops) if o.size == 3 and o.cin == 512)
    with pytest.raises(rt.Y3Error, match="only Y3_DTYPE_BF16 plans take a bf16 split"):
        net.set_split_k_bf16(slot, 2)
    assert net.split_k_bf16(slot) == 1
    net.set_stem_fusion(0)
    a = [g.clone() for g in net.forward(x)]
    net.set_stem_fusion(1)
    b = net.forward(x)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    net.plan(1, 64, BF16)       # the same switches do act on a bf16 plan of the same net
    assert any(net.split_k_bf16(i) > 1 for i in range(len(net.conv_ops)))


def test_f16_standalone_aux_ops_are_refused(rt):
    from yolo_v3_tf2_amd.weights import synthetic_weights
    p, _ = unfolded_program()
    net = rt.Net(p)
    net.load_weights(synthetic_weights(p, seed=12))
    net.plan(2, 12, F16)
    x = np.random.default_rng(12).standard_normal((2, 12, 12, 64)).astype(np.float32)
    with pytest.raises(rt.Y3Error, match="stand-alone add/upsample/concat ops are fp32 only"):
        net.forward(_cuda(x).to(torch.float16))
    with pytest.raises(rt.Y3Error, match="float16"):
        net.forward(_cuda(x))                   # an input that feeds an MFMA conv directly is handed over in fp16
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 7. the YAML key
def test_inference_yaml_dtype_f16_reaches_an_fp16_plan(rt, weights, tmp_path, monkeypatch):
    import yaml
    from yolo_v3_tf2_amd.inference import Inference
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config/detect_config_coco.yaml")))
    assert cfg.get("dtype") is None                                   # the packaged config leaves it at fp32
    for k in ("model_config_file", "classes_name_file", "anchors_file", "image_file_path", "images_dir"):
        cfg[k] = os.path.join(ROOT, cfg[k])
    cfg.update(image_size=64, output_dir=str(tmp_path / "out"), input_weights_path=None, dtype="f16")
    monkeypatch.chdir(tmp_path)                                       # build() writes model_inference_summary.txt
    inf = Inference()
    results = inf(weights=weights, **cfg)
    assert len(results) == 1
    net = inf.detect_model.model._device_net()
    assert net.dtype == F16 and net.canvas == (64, 64) and net.max_batch == 1
    with pytest.raises(rt.Y3Error, match="dtype"):
        inf.detect_model.model.set_dtype("half")
    inf.detect_model.model.set_dtype(None)                            # absent means fp32: the planned net is planned again
    assert net.dtype == _lib.Y3_DTYPE_F32
