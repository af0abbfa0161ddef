"""int8 plans (Y3_DTYPE_I8) on the GPU: csrc/conv_i8.hip, quantize16_to_i8 / i8_to_f32 and the host layer around them, against the NumPy
restatement of the scheme (yolo_v3_tf2_amd/quant.py).  i32 accumulation is exact and the epilogue is a fixed sequence of fp32
operations, so EVERY comparison here is torch.equal / np.array_equal: no tolerance anywhere."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import _Graph, mini_program  # noqa: E402
from yolo_v3_tf2_amd import _lib, quant  # noqa: E402

I8, F16 = _lib.Y3_DTYPE_I8, _lib.Y3_DTYPE_F16


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _round_f16(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def _check_convs(net, p, w, scales, B, grids, first):
    """Every conv from slot `first` on against quant.conv_i8 on the device's own input bytes; -> number of launches checked."""
    outs = {t: g.cpu().numpy().reshape(B, g.shape[1], g.shape[2], -1) for t, g in zip(p.outputs, grids)}
    cache = {}

    def dev_q(t):
        if t not in cache:
            cache[t] = net.read_tensor_i8(t, B).cpu().numpy()
        return cache[t]

    n = 0
    for o in p.conv_ops()[first:]:
        f32 = quant.writes_f32(p, o)
        exp = quant.conv_i8(o, w, dev_q, scales, f32)
        got = outs[o.dst] if f32 else dev_q(o.dst)
        assert got.dtype == exp.dtype and got.shape == exp.shape, (o.conv_index, got.dtype, got.shape, exp.shape)
        assert np.array_equal(got, exp), (o.conv_index, int((got != exp).sum()), got.size)
        if not f32:   # y3_net_read_tensor on an int8 tensor: (float)q * s
            assert np.array_equal(net.read_tensor(o.dst, B).cpu().numpy(), quant.dequantize(got, scales[o.dst])), o.conv_index
            assert np.abs(got).max() > 8, o.conv_index      # not a comparison of two empty buffers
        n += 1
    return n


# ---------------------------------------------------------------------------------------------- 1. per-tile matrix
def _matrix_program():
    """fp16 input of 128 channels, so c* = 0 and the input goes through quantize16_to_i8:
      a   1x1    128 -> 256, BN, leaky                    one K tile
      b   3x3/1  256 -> 128, BN, linear, + input          18 K tiles, a tap change every second tile; the shortcut is the int8 copy
      d   3x3/2  128 -> 128, BN, leaky       (reads b)    stride 2
      f   1x1    [up(d), a] -> 256, BN, leaky             upsample + concat 128 (+) 256
      h0  1x1    256 -> 255, bias, linear    (reads f)    fp32 out, ragged N
      h1  3x3/2  256 -> 256, BN, leaky       (reads f)    fp32 out
      h2  1x1    128 -> 256, BN, linear      (reads b)    fp32 out"""
    g = _Graph(128)
    g._keep(g.input)
    a = g.conv(g.input, 256, 1)
    b = g.shortcut(g.conv(a, 128, 3, act="linear"), g.input)
    d = g.conv(b, 128, 3, stride=2)
    f = g.conv(g.route(g.upsample(d), a), 256, 1)
    h0 = g.conv(f, 255, 1, bn=False, act="linear", sub="head")
    h1 = g.conv(f, 256, 3, stride=2, sub="head")
    h2 = g.conv(b, 256, 1, act="linear", sub="head")
    return g.program([h0, h1, h2])


MATRIX_CANVASES = ((2, (40, 48)), (3, (24, 24)))     # M no multiple of the tile's rows, tiles span an image boundary
_matrix_cache = {}


def _matrix_case(rt, B, canvas):
    """(program, weights, fp16-exact input, calibrated scales) of a canvas: made once, shared by the tiles, left unchanged."""
    if (B, canvas) not in _matrix_cache:
        from yolo_v3_tf2_amd.weights import synthetic_weights
        p = _matrix_program()
        w = synthetic_weights(p, seed=8)
        x = _round_f16(np.random.default_rng(8).standard_normal((B, canvas[0], canvas[1], 128)))
        cal = rt.Net(p)
        cal.load_weights(w)
        scales = cal.calibrate_i8(_cuda(x))
        _matrix_cache[(B, canvas)] = (p, w, x, scales)
    return _matrix_cache[(B, canvas)]


@pytest.mark.parametrize("B,canvas", MATRIX_CANVASES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("tile", _lib.TILES_I8_BUILT)
def test_i8_every_tile_every_launch_form_bit_exact(rt, tile, B, canvas):
    p, w, x, scales = _matrix_case(rt, B, canvas)
    assert _lib.tile_built(I8, tile)
    net = rt.Net(p)
    net.load_weights(w)
    net.set_act_scales(scales)
    bn = _lib.TILES_BF16[tile][1]
    forced = 0
    for slot, o in enumerate(net.conv_ops):
        if ((o.cout + 31) // 32 * 32) % bn == 0:
            net.set_tile_bf16(slot, tile)
            forced += 1
    assert forced >= 4      # a, f and the three heads at the least (every conv below 256 wide)
    net.keep_activations(True)
    net.plan(B, canvas, I8)
    assert net.i8_first_conv() == 0
    xin = _cuda(x).to(torch.float16)
    first = [g.clone() for g in net.forward(xin)]
    grids = net.forward(xin)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, grids)), "two forwards of one plan differ"
    # the input's int8 copy
    assert np.array_equal(net.read_tensor_i8(p.input_tensor, B).cpu().numpy(), quant.quantize(x, scales[p.input_tensor]))
    assert _check_convs(net, p, w, scales, B, grids, 0) == 7


def test_i8_tile_built_reports_the_int8_tiles():
    built = [t for t in range(len(_lib.TILES_BF16) + 4) if _lib.tile_built(I8, t)]
    assert built == list(_lib.TILES_I8_BUILT)
    assert all(_lib.tile_built(_lib.Y3_DTYPE_BF16, t) and _lib.TILES_BF16[t][3] == 64 for t in built)


# ---------------------------------------------------------------------------------------------- 2, 3. the real network at 2 x 96^2
@pytest.fixture(scope="module")
def real96(rt, program, weights):
    S, B = 96, 2
    x = np.random.default_rng(1234).random((B, S, S, 3), dtype=np.float32)
    cal = rt.Net(program)
    cal.load_weights(weights)
    scales = cal.calibrate_i8(_cuda(x))
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_act_scales(scales)
    net.keep_activations(True)
    net.plan(B, S, I8)
    grids = [g.clone() for g in net.forward(_cuda(x))]
    torch.cuda.synchronize()
    return dict(S=S, B=B, x=x, scales=scales, net=net, grids=grids)


def test_i8_real_network_teacher_forced(rt, program, weights, real96):
    net, B, S, scales = real96["net"], real96["B"], real96["S"], real96["scales"]
    cut = net.i8_first_conv()
    assert cut == 9 == quant.first_i8_conv(program)
    assert net.act_scales() == [float(np.float32(s)) for s in scales]
    f16 = rt.Net(program)
    f16.load_weights(weights)
    f16.keep_activations(True)
    f16.plan(B, S, F16)
    f16.forward(_cuda(real96["x"]))
    convs = program.conv_ops()
    for o in convs[:cut]:       # before the cut: an fp16 plan's launches, bit for bit
        assert torch.equal(net.read_tensor(o.dst, B), f16.read_tensor(o.dst, B)), o.conv_index
    behind = {o.dst for o in convs[cut:]}
    crossing = sorted({t for o in convs[cut:] for t in (o.src0, o.src1, o.residual) if t >= 0 and t not in behind})
    assert crossing == [convs[cut - 1].dst]     # conv 8's output only
    for t in crossing:          # the boundary copy
        assert np.array_equal(net.read_tensor_i8(t, B).cpu().numpy(), quant.quantize(net.read_tensor(t, B).cpu().numpy(), scales[t]))
    assert _check_convs(net, program, weights, scales, B, real96["grids"], cut) == len(convs) - cut


def test_i8_real_network_free_running_from_the_boundary_bytes(program, weights, real96):
    net, B, scales = real96["net"], real96["B"], real96["scales"]
    cut = net.i8_first_conv()
    t8 = program.conv_ops()[cut - 1].dst
    out = quant.forward_i8(program, weights, scales, {t8: net.read_tensor_i8(t8, B).cpu().numpy()}, cut)
    for t, g in zip(program.outputs, real96["grids"]):
        g = g.cpu().numpy().reshape(out[t].shape)
        assert np.array_equal(g, out[t]) and np.isfinite(g).all() and np.abs(g).max() > 0, t


# ---------------------------------------------------------------------------------------------- 4. routes
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("canvas", [64, (64, 96)], ids=["64", "64x96"])
def test_i8_detect_and_forward_decode_equal_the_composed_route(rt, program, weights, anchors, real96, canvas, lanes):
    H, W = rt.canvas_hw(canvas)
    B = 2
    x = _cuda(np.random.default_rng(41).random((B, H, W, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_act_scales(real96["scales"])
    net.plan(B, canvas, I8)
    net.set_lanes(lanes)
    assert net.dtype == I8 and net.i8_first_conv() == 9
    grids = [g.clone() for g in net.forward(x)]
    again = net.forward(x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(grids, again)), "two forwards differ"
    assert all(float(g.abs().max()) > 0 for g in grids)
    bb, cc, ss = rt.yolo_decode_scores(grids, anchors, 80)
    sel, nv = rt.nms_padded(bb, ss, 100, 0.5, 0.05)
    want = rt.pack_detections(bb, cc, ss, sel, nv)
    for _ in range(2):
        fb, fc, fs = net.forward_decode(x, anchors)
        packed, nv2 = net.detect(x, anchors, 100, 0.5, 0.05)
        torch.cuda.synchronize()
        assert torch.equal(fb, bb) and torch.equal(fc, cc) and torch.equal(fs, ss)
        assert torch.equal(nv2, nv) and torch.equal(packed, want)
    g0 = net.forward(x[0:1].contiguous())
    torch.cuda.synchronize()
    assert all(torch.equal(a[0:1], b) for a, b in zip(grids, g0)), "image 0 of a batch is not the image alone"
    p0, n0 = net.detect(x[0:1].contiguous(), anchors, 100, 0.5, 0.05)
    assert torch.equal(p0, want[0:1]) and torch.equal(n0, nv[0:1])
    # none of the low-latency switches acts on an int8 plan
    net.set_low_latency(True)
    net.set_low_latency_bf16(True)
    net.set_low_latency_f16(True)
    net.plan(B, canvas, I8)
    net.set_lanes(lanes)
    assert all(net.split_k(i) == 1 and net.split_k_bf16(i) == 1 and net.split_k_f16(i) == 1 for i in range(len(net.conv_ops)))
    ll = net.forward(x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(grids, ll))


def test_i8_detect_graph_capture(rt, program, weights, anchors, real96):
    """A captured detect on an int8 plan, two lanes, replayed three times, equals eager."""
    x = _cuda(np.random.default_rng(31).random((2, 64, 64, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_act_scales(real96["scales"])
    net.plan(2, 64, I8)
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
        assert torch.equal(gn, want_n) and torch.equal(gp, want_p)


def test_i8_plan_with_the_fp16_fused_stem(rt, program, weights, anchors, real96):
    """set_stem_fusion_f16 acts on the convs before the cut of an int8 plan as on an fp16 plan: the stem kernel runs, the routes stay
    bit-identical to each other, and the switch of the fp32 / bf16 plans changes nothing."""
    x = _cuda(np.random.default_rng(41).random((2, 64, 64, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_act_scales(real96["scales"])
    net.plan(2, 64, I8)
    plain = [g.clone() for g in net.forward(x)]
    net.set_stem_fusion(0)
    same = net.forward(x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(plain, same))
    net.set_stem_fusion_f16(1)
    grids = [g.clone() for g in net.forward(x)]
    bb, cc, ss = rt.yolo_decode_scores(grids, anchors, 80)
    fb, fc, fs = net.forward_decode(x, anchors)
    torch.cuda.synchronize()
    assert torch.equal(fb, bb) and torch.equal(fc, cc) and torch.equal(fs, ss)
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grids)
    assert net.measure_sclk(x, grids, forwards=2) > 0      # only the stem kernel carries clock stamps in this plan: it did run
    net.set_stem_fusion_f16(0)
    with pytest.raises(rt.Y3Error, match="carries clock stamps"):
        net.measure_sclk(x, grids, forwards=2)


# ---------------------------------------------------------------------------------------------- 5. calibration file and the YAML keys
def test_i8_calibration_file_and_inference_yaml(rt, program, weights, real96, tmp_path, monkeypatch):
    import os
    import yaml
    from yolo_v3_tf2_amd.inference import Inference
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cal = rt.Net(program)
    cal.set_act_scales(real96["scales"])
    path = str(tmp_path / "cal.json")
    cal.save_calibration(path)
    fresh = rt.Net(program)
    assert fresh.load_calibration(path) == cal.act_scales() == fresh.act_scales()
    other = rt.Net(_matrix_program())
    with pytest.raises(rt.Y3Error, match="another graph"):
        other.load_calibration(path)
    cfg = yaml.safe_load(open(os.path.join(root, "config/detect_config_coco.yaml")))
    assert cfg.get("dtype") is None and cfg.get("i8_calibration") is None      # the packaged config leaves both out
    for k in ("model_config_file", "classes_name_file", "anchors_file", "image_file_path", "images_dir"):
        cfg[k] = os.path.join(root, cfg[k])
    cfg.update(image_size=64, output_dir=str(tmp_path / "out"), input_weights_path=None, dtype="i8", i8_calibration=path)
    monkeypatch.chdir(tmp_path)                                       # build() writes model_inference_summary.txt
    inf = Inference()
    results = inf(weights=weights, **cfg)
    assert len(results) == 1
    net = inf.detect_model.model._device_net()
    assert net.dtype == I8 and net.canvas == (64, 64) and net.i8_first_conv() == 9
    # without the file the plan names the tensor it has no scale for
    cfg["i8_calibration"] = None
    with pytest.raises(rt.Y3Error, match=r"needs the scale of tensor \d+"):
        Inference()(weights=weights, **cfg)


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_i8_refusals(rt):
    from yolo_v3_tf2_amd.weights import synthetic_weights
    p = _matrix_program()
    net = rt.Net(p)
    net.load_weights(synthetic_weights(p, seed=8))
    with pytest.raises(rt.Y3Error, match=r"needs the scale of tensor \d+"):
        net.plan(2, 24, I8)                                 # no scales
    with pytest.raises(rt.Y3Error, match="scales for a net of"):
        net.set_act_scales([1.0] * (len(p.tensors) + 1))    # wrong length
    scales = [0.05] * len(p.tensors)
    net.set_act_scales(scales)
    net.plan(2, 24, I8)                                     # every scale set, concat sources equal: planned
    cat = next(o for o in p.conv_ops() if o.src1 >= 0)
    scales[cat.src1] = 0.1
    net.set_act_scales(scales)
    with pytest.raises(rt.Y3Error, match=r"conv \d+ concatenates tensors .* different int8 scales"):
        net.plan(2, 24, I8)
    net.plan(2, 24, F16)                                    # the net itself is unharmed
    # a graph with no qualifying conv: the last conv reads 64 channels
    q = mini_program(128, [dict(filters=64, size=1)], [dict(filters=64, size=1), dict(filters=64, size=1), dict(filters=64, size=1)])
    net2 = rt.Net(q)
    net2.load_weights(synthetic_weights(q, seed=8))
    net2.set_act_scales([0.05] * len(q.tensors))
    with pytest.raises(rt.Y3Error, match="no conv of this graph qualifies for int8"):
        net2.plan(2, 24, I8)
