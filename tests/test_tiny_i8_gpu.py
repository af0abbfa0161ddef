"""int8 plans of pooled nets on the GPU (Net.set_pools_i8; include/y3.h, "Stand-alone ops in int8"): the max-pool kernel on signed bytes,
the up-sample and the concat on int8 tensors, and YOLOv3-tiny planned in int8 with the fused tiny stem before its cut -- every stored
byte and every head logit against the NumPy restatement (yolo_v3_tf2_amd/quant.py).  Every comparison is torch.equal / np.array_equal:
int8 has no tolerance anywhere."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import tiny_cases as TC  # noqa: E402
from tests import tiny_i8_cases as IC  # noqa: E402
from yolo_v3_tf2_amd import _lib, ops, quant  # noqa: E402
from yolo_v3_tf2_amd.graph import ConvOp  # noqa: E402
from yolo_v3_tf2_amd.maxpool import maxpool2x2_ref  # noqa: E402

NC = 80
LOW = 0.007          # inside the score range of the random-init tiny heads (tests/test_tiny_gpu.py)
I8, F16, F32 = _lib.Y3_DTYPE_I8, _lib.Y3_DTYPE_F16, _lib.Y3_DTYPE_F32
OLD_REFUSAL = ("y3_net_plan: the net holds a max-pool op (Y3_AUX_MAXPOOL2X2_*), which has no calibrated int8 form; "
               "Y3_DTYPE_F32, Y3_DTYPE_BF16 and Y3_DTYPE_F16 run it")
NO_STEM_REFUSAL = "conv 1 (Cin 32, c0 -1, Cout 32) has no fp16 tile (it lies before the int8 cut, conv 4, and runs in fp16)"


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    _lib.require_gpu()      # fail loudly, never fall back
    return runtime


@pytest.fixture(scope="module")
def tiny():
    return TC.tiny_program(NC)


def _cuda(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _i8_net(rt, program, weights, scales, batch, canvas, keep=False, stem=True, pools=True, setup=None):
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_tiny_stem_fusion(stem)
    net.set_pools_i8(pools)
    net.set_act_scales(scales)
    if setup:
        setup(net)
    net.keep_activations(keep)
    net.plan(batch, canvas, I8)
    return net


_cases = {}


def _tiny_case(rt, tiny, canvas):
    """(weights, images, calibrated scales) of real tiny at 2 images of a canvas: made once, shared, left unchanged."""
    if canvas not in _cases:
        w, x = TC.tiny_inputs(tiny, 2, canvas)
        cal = rt.Net(tiny)
        cal.load_weights(w)
        cal.set_pools_i8(True)
        scales = cal.calibrate_i8(_cuda(x))
        _cases[canvas] = (w, x, scales)
    return _cases[canvas]


def _stored(net, program, B, cut):
    """{tensor id: the device's int8 bytes} of the boundary copies, every int8 conv output and every int8 aux output."""
    ids = set(quant.crossing_tensors(program, cut)) | {o.dst for o in quant.i8_aux_ops(program, cut)[0]}
    ids |= {o.dst for o in program.conv_ops()[cut:] if not quant.writes_f32(program, o)}
    return {t: net.read_tensor_i8(t, B).cpu().numpy() for t in sorted(ids)}


def _check_launches(net, program, weights, scales, B, grids, cut):
    """Every launch behind the cut -- conv and int8 aux op -- against quant.py on the device's own input bytes; -> (convs, aux ops) checked."""
    outs = {t: g.cpu().numpy().reshape(B, g.shape[1], g.shape[2], -1) for t, g in zip(program.outputs, grids)}
    dev = _stored(net, program, B, cut)
    aux = quant.i8_aux_ops(program, cut)[0]
    n_conv = n_aux = 0
    for o in program.ops[program.ops.index(program.conv_ops()[cut]):]:
        if isinstance(o, ConvOp):
            f32 = quant.writes_f32(program, o)
            exp = quant.conv_i8(o, weights, dev.__getitem__, scales, f32)
            got = outs[o.dst] if f32 else dev[o.dst]
            n_conv += 1
        elif any(o is a for a in aux):
            exp, got = quant.aux_i8(o, dev.__getitem__, scales), dev[o.dst]
            n_aux += 1
        else:
            continue
        assert got.dtype == exp.dtype and got.shape == exp.shape, (o, got.dtype, got.shape, exp.shape)
        assert np.array_equal(got, exp), (o, int((got != exp).sum()), got.size)
        if got.dtype == np.int8:      # y3_net_read_tensor on an int8 tensor: (float)q * s; and not two empty buffers
            assert np.array_equal(net.read_tensor(o.dst, B).cpu().numpy(), quant.dequantize(got, scales[o.dst])), o
            assert np.abs(got).max() > 8, o
    return n_conv, n_aux


def _check_free_running(net, program, weights, scales, B, grids, cut, images=None):
    """Every stored byte and both head grids against quant.forward_i8 from the device's boundary copy (images: a slice of the batch)."""
    dev = _stored(net, program, B, cut)
    sl = slice(None) if images is None else images
    out = quant.forward_i8(program, weights, scales, {t: dev[t][sl] for t in quant.crossing_tensors(program, cut)}, cut)
    for t, q in dev.items():
        assert np.array_equal(q[sl], out[t]), (t, int((q[sl] != out[t]).sum()))
    for t, g in zip(program.outputs, grids):
        g = g.cpu().numpy()[sl]
        assert np.array_equal(g.reshape(out[t].shape), out[t]) and np.isfinite(g).all() and np.abs(g).max() > 0, t
    return out


# ---------------------------------------------------------------------------------------------- 1. the pool kernel in int8
@pytest.mark.parametrize("kind", IC.POOL_DATA)
@pytest.mark.parametrize("shape,stride", [(s, st) for s, sts in IC.POOL_SHAPES for st in sts], ids=lambda v: str(v).replace(" ", ""))
def test_maxpool_int8_equals_the_reference(rt, shape, stride, kind):
    x = IC.pool_data_i8(shape, kind)
    want = maxpool2x2_ref(x, stride)
    out = torch.full(want.shape, 7, dtype=torch.int8, device="cuda")
    got = ops.maxpool2x2(_cuda(x), stride, out=out)
    torch.cuda.synchronize()
    assert got is out and got.dtype == torch.int8 and np.array_equal(got.cpu().numpy(), want)
    again = ops.maxpool2x2(_cuda(x), stride)
    assert torch.equal(again, got)


def test_maxpool_int8_refusals_and_graph_capture(rt):
    with pytest.raises(rt.Y3Error, match="8 channels of 1 bytes are no multiple of 16 bytes"):
        ops.maxpool2x2(torch.zeros((1, 2, 2, 8), dtype=torch.int8, device="cuda"), 2)
    with pytest.raises(rt.Y3Error, match="float32, bfloat16, float16 or int8"):
        ops.maxpool2x2(torch.zeros((1, 2, 2, 16), dtype=torch.int16, device="cuda"), 2)
    x = _cuda(IC.pool_data_i8((2, 13, 13, 512), "random"))
    want = maxpool2x2_ref(x.cpu().numpy(), 1)
    out = torch.full(want.shape, 7, dtype=torch.int8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.maxpool2x2(x, 1, out=out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.maxpool2x2(x, 1, out=out)
    for _ in range(2):
        out.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------- 2. up-sample and concat on int8 tensors
@pytest.mark.parametrize("canvas,B,lanes", [((8, 8), 1, 1), ((12, 4), 3, 1), ((12, 20), 2, 2)], ids=["8x8", "12x4x3", "12x20-two-lanes"])
def test_reduced_pooled_net_every_aux_op_bit_for_bit(rt, canvas, B, lanes):
    p, ids = IC.reduced_pooled_program()
    w, x = IC.reduced_inputs(p, B, canvas)
    s = IC.class_scales(p)
    net = _i8_net(rt, p, w, s, B, canvas, keep=True)
    net.set_lanes(lanes)
    assert net.pools_i8 == 1 and net.i8_first_conv() == 0 and net.tiny_stem_fused == 0
    grids = net.forward(_cuda(x).to(torch.float16))
    torch.cuda.synchronize()
    dev = _stored(net, p, B, 0)
    assert np.array_equal(dev[p.input_tensor], quant.quantize(x, s[p.input_tensor]))
    # the moves on their own, stated here without quant.py
    c = next(o for o in p.conv_ops() if o.src0 == ids["pb"]).dst
    a = p.conv_ops()[0].dst
    assert np.array_equal(dev[ids["up"]], dev[c].repeat(2, axis=1).repeat(2, axis=2))
    assert np.array_equal(dev[ids["cat"]], np.concatenate([dev[ids["up"]], dev[a]], axis=3)) and dev[ids["cat"]].shape[3] == 384
    assert np.array_equal(dev[ids["pa"]], maxpool2x2_ref(dev[a], 2))
    assert _check_launches(net, p, w, s, B, grids, 0) == (5, 4)
    ref = _check_free_running(net, p, w, s, B, grids, 0)
    brute = IC.brute_walk(p, w, s, {p.input_tensor: dev[p.input_tensor]}, 0)
    assert all(np.array_equal(ref[t], brute[t]) for t in ref)


# ---------------------------------------------------------------------------------------------- 3. real tiny
@pytest.fixture(scope="module", params=[(96, 96), (96, 64)], ids=["96x96", "96x64"])
def planned(rt, tiny, request):
    canvas = request.param
    w, x, scales = _tiny_case(rt, tiny, canvas)
    net = _i8_net(rt, tiny, w, scales, 2, canvas, keep=True)
    grids = [g.clone() for g in net.forward(_cuda(x))]
    torch.cuda.synchronize()
    return dict(canvas=canvas, w=w, x=x, scales=scales, net=net, grids=grids)


def test_tiny_plans_in_int8_with_both_switches(rt, tiny, planned):
    net = planned["net"]
    assert net.dtype == I8 and net.pools_i8 == 1 and net.tiny_stem_fused == 1 and net.i8_first_conv() == 4 == quant.first_i8_conv(tiny)
    assert net.act_scales() == [float(np.float32(s)) for s in planned["scales"]]
    s = planned["scales"]
    assert s[9] == s[10] == s[18] == s[19] == s[20] and s[11] == s[12] and s[8] > 0
    for t in (1, 2, 3):      # inside the fused tiny stem: never stored
        with pytest.raises(rt.Y3Error, match="inside the fused tiny stem"):
            net.read_tensor(t, 2)
    with pytest.raises(rt.Y3Error, match="not held as int8"):
        net.read_tensor_i8(7, 2)      # an fp16 tensor before the cut


def test_tiny_teacher_forced(rt, tiny, planned):
    net, w, x, scales = planned["net"], planned["w"], planned["x"], planned["scales"]
    f16 = rt.Net(tiny)
    f16.load_weights(w)
    f16.set_tiny_stem_fusion(True)
    f16.keep_activations(True)
    f16.plan(2, planned["canvas"], F16)
    f16.forward(_cuda(x))
    for t in (4, 5, 6, 7, 8):       # before the cut: an fp16 plan's launches, bit for bit (1, 2, 3 lie inside the stem launch)
        assert torch.equal(net.read_tensor(t, 2), f16.read_tensor(t, 2)) and float(net.read_tensor(t, 2).abs().max()) > 0, t
    # the boundary copy of pool 3's output
    assert np.array_equal(net.read_tensor_i8(8, 2).cpu().numpy(), quant.quantize(net.read_tensor(8, 2).cpu().numpy(), scales[8]))
    assert _check_launches(net, tiny, w, scales, 2, planned["grids"], 4) == (9, 4)


def test_tiny_free_running_and_deterministic(rt, tiny, planned):
    net = planned["net"]
    _check_free_running(net, tiny, planned["w"], planned["scales"], 2, planned["grids"], 4)
    before = _stored(net, tiny, 2, 4)
    again = net.forward(_cuda(planned["x"]))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(planned["grids"], again)), "two forwards of one plan differ"
    after = _stored(net, tiny, 2, 4)
    assert all(np.array_equal(before[t], after[t]) for t in before)


def test_tiny_saturating_scales(rt, tiny, planned):
    """Scales a quarter of the calibrated ones: most values clamp at +-127, and the device still equals the restatement byte for byte."""
    w, x = planned["w"], planned["x"]
    scales = [float(np.float32(s) * np.float32(0.25)) for s in planned["scales"]]
    net = _i8_net(rt, tiny, w, scales, 2, planned["canvas"], keep=True)
    grids = net.forward(_cuda(x))
    torch.cuda.synchronize()
    dev = _stored(net, tiny, 2, 4)
    sat = {t: float((np.abs(q) == 127).mean()) for t, q in dev.items()}
    assert sat[8] > 0.02 and sat[9] > 0.02 and sat[10] > 0.02, sat      # the data does saturate: the boundary copy, the first conv, the first int8 pool
    assert _check_launches(net, tiny, w, scales, 2, grids, 4) == (9, 4)
    _check_free_running(net, tiny, w, scales, 2, grids, 4)


def test_tiny_two_lanes_batch_position_and_graph_replay(rt, tiny, planned):
    w, x, scales, canvas = planned["w"], planned["x"], planned["scales"], planned["canvas"]
    xin = _cuda(x)
    net = _i8_net(rt, tiny, w, scales, 2, canvas, keep=True)
    net.set_lanes(2)
    grids = [g.clone() for g in net.forward(xin)]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(grids, planned["grids"])), "two lanes change the bits"
    _check_free_running(net, tiny, w, scales, 2, grids, 4)
    # graph replay of the two-lane forward
    out = [torch.zeros_like(g) for g in grids]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net.forward(xin, out=out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        net.forward(xin, out=out)
    for _ in range(2):
        for o in out:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, grids))
    _check_free_running(net, tiny, w, scales, 2, out, 4)
    # image 1 of the batch alone: the same bits, and the restatement from its own boundary bytes
    net.set_lanes(1)
    alone = net.forward(xin[1:2].contiguous())
    torch.cuda.synchronize()
    assert all(torch.equal(a[1:2], b) for a, b in zip(grids, alone)), "image 1 of a batch is not the image alone"
    _check_free_running(planned["net"], tiny, w, scales, 2, planned["grids"], 4, images=slice(1, 2))


def test_tiny_detect_equals_the_composed_calls(rt, tiny, planned):
    w, x, scales, canvas = planned["w"], planned["x"], planned["scales"], planned["canvas"]
    anchors = TC.tiny_anchors()
    xin = _cuda(x)
    for lanes in (1, 2):
        net = _i8_net(rt, tiny, w, scales, 2, canvas)
        net.set_lanes(lanes)
        grids = [g.clone() for g in net.forward(xin)]
        assert all(torch.equal(a, b) for a, b in zip(grids, planned["grids"])), "keep_activations changes the bits"
        bb, cc, ss = rt.yolo_decode_scores(grids, anchors, NC)
        sel, nv = rt.nms_padded(bb, ss, 100, 0.5, LOW)
        want = rt.pack_detections(bb, cc, ss, sel, nv)
        for _ in range(2):
            fb, fc, fs = net.forward_decode(xin, anchors)
            packed, nv2 = net.detect(xin, anchors, 100, 0.5, LOW)
            torch.cuda.synchronize()
            assert torch.equal(fb, bb) and torch.equal(fc, cc) and torch.equal(fs, ss)
            assert torch.equal(nv2, nv) and torch.equal(packed, want) and int(nv.sum()) > 0


# ---------------------------------------------------------------------------------------------- 4. low latency
def test_tiny_low_latency_i8_equals_the_default_plan(rt, tiny):
    w, x, scales = _tiny_case(rt, tiny, (96, 96))
    xin = _cuda(x[:1])
    base = _i8_net(rt, tiny, w, scales, 1, 96, keep=True)
    want = [g.clone() for g in base.forward(xin)]
    ll = _i8_net(rt, tiny, w, scales, 1, 96, keep=True, setup=lambda n: n.set_low_latency_i8(True))
    if all(ll.split_k_i8(i) == 1 for i in range(len(ll.conv_ops))):      # the rule splits none at this size: force conv 6 (K = 4608, 36 K tiles)
        ll.set_split_k_i8(6, 2)
    split = [ll.split_k_i8(i) for i in range(len(ll.conv_ops))]
    assert max(split) > 1 and all(s == 1 for s in split[:4]), split
    got = ll.forward(xin)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    a, b = _stored(base, tiny, 1, 4), _stored(ll, tiny, 1, 4)
    assert sorted(a) == sorted(b) and all(np.array_equal(a[t], b[t]) for t in a)
    _check_free_running(ll, tiny, w, scales, 1, got, 4)


# ---------------------------------------------------------------------------------------------- 5. switch discipline
def test_switch_off_keeps_the_old_refusal_word_for_word(rt, tiny):
    w, _, scales = _tiny_case(rt, tiny, (96, 96))
    for setup in (None, lambda n: n.set_pools_i8(False), lambda n: n.set_pools_i8(None)):
        net = rt.Net(tiny)
        net.load_weights(w)
        net.set_tiny_stem_fusion(True)
        net.set_act_scales(scales)
        if setup:
            setup(net)
        with pytest.raises(rt.Y3Error) as e:
            net.plan(2, 96, I8)
        assert OLD_REFUSAL in str(e.value) and net.pools_i8 == 0


def test_switch_on_a_planned_net_waits_for_the_next_plan(rt, tiny):
    w, x, scales = _tiny_case(rt, tiny, (96, 96))
    xin = _cuda(x)
    net = _i8_net(rt, tiny, w, scales, 2, 96)
    want = [g.clone() for g in net.forward(xin)]
    net.set_pools_i8(False)
    assert net.pools_i8 == 1
    same = net.forward(xin)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(want, same))
    with pytest.raises(rt.Y3Error) as e:
        net.plan(2, 96, I8)
    assert OLD_REFUSAL in str(e.value)
    # and the other way: an fp32 plan is no int8 plan whatever the switch says
    net.set_pools_i8(True)
    net.plan(2, 96, F32)
    assert net.pools_i8 == 0 and net.tiny_stem_fused == 1
    net.plan(2, 96, I8)
    assert net.pools_i8 == 1
    back = net.forward(xin)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(want, back))


def test_on_yolov3_the_switch_changes_nothing(rt, program, weights):
    x = _cuda(np.random.default_rng(1234).random((2, 64, 64, 3), dtype=np.float32))
    grids = {}
    off = rt.Net(program)
    off.load_weights(weights)
    scales = off.calibrate_i8(x)
    on = rt.Net(program)
    on.load_weights(weights)
    on.set_pools_i8(True)
    assert on.calibrate_i8(x) == scales      # nothing more to measure on a net without aux ops
    for flag, net in ((False, off), (True, on)):
        net.plan(2, 64, I8)
        assert net.pools_i8 == 0 and net.i8_first_conv() == 9
        grids[flag] = [g.clone() for g in net.forward(x)]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) and float(a.abs().max()) > 0 for a, b in zip(grids[False], grids[True]))


def test_calibrate_with_the_switch_off_returns_what_it_returned(rt, tiny):
    w, x, scales = _tiny_case(rt, tiny, (96, 96))
    cal = rt.Net(tiny)
    cal.load_weights(w)
    off = cal.calibrate_i8(_cuda(x))
    conv_dsts = {o.dst for o in tiny.conv_ops()}
    assert all((off[t] > 0) == (t in conv_dsts) for t in range(len(off)))
    assert all(off[t] == scales[t] for t in conv_dsts if t not in (9, 18))      # tied classes took their largest member
    # with the fused tiny stem the tensors it keeps on chip are skipped
    cal.set_pools_i8(True)
    cal.set_tiny_stem_fusion(True)
    fused = cal.calibrate_i8(_cuda(x))
    written = {o.dst for o in tiny.ops} - {1, 2, 3}
    assert fused[1] == fused[2] == fused[3] == 0.0 and all((fused[t] > 0) == (t in written) for t in range(len(fused)))
    assert fused[9] == fused[10] == fused[18] == fused[19] == fused[20] and fused[11] == fused[12]
    # (the fp32 stem kernel sums in another order than the launches it replaces: the same scales to a few ulps, not to the bit)
    assert np.allclose([fused[t] for t in sorted(written)], [scales[t] for t in sorted(written)], rtol=1e-3, atol=0.0)


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_tiny_refusals(rt, tiny):
    w, _, scales = _tiny_case(rt, tiny, (96, 96))

    def refused(scales_, stem=True, dtype=I8):
        net = rt.Net(tiny)
        net.load_weights(w)
        net.set_tiny_stem_fusion(stem)
        net.set_pools_i8(True)
        net.set_act_scales(scales_)
        with pytest.raises(rt.Y3Error) as e:
            net.plan(2, 96, dtype)
        assert net.max_batch == 0 and net.pools_i8 == 0
        return str(e.value)

    assert NO_STEM_REFUSAL in refused(scales, stem=False)
    for t in (10, 20):                                        # a pool's and the concat's destination
        s = list(scales)
        s[t] = 0.0
        assert f"an int8 plan needs the scale of tensor {t} " in refused(s)
    s = list(scales)
    s[12] = 2.0 * s[12]
    msg = refused(s)
    assert "aux op 5 moves int8 bytes between tensors 11 and 12 with different int8 scales" in msg and "they must be equal" in msg
    s = list(scales)
    s[19] = 0.5 * s[19]
    assert "tensors 18 and 19 with different int8 scales" in refused(s)
    for dt, tag in ((_lib.Y3_DTYPE_F32X3, "f32x3"), (_lib.Y3_DTYPE_F32X2, "f32x2")):
        assert "does not read plane-split tensors" in refused(scales, dtype=dt), tag


def test_graphs_refused_by_name_with_the_plan_in_force_left_alone(rt):
    from yolo_v3_tf2_amd.weights import synthetic_weights
    p = IC.add_behind_cut_program()
    net = rt.Net(p)
    net.load_weights(synthetic_weights(p, seed=5))
    net.set_act_scales([0.05] * len(p.tensors))
    net.set_pools_i8(True)
    net.plan(1, 8, F16)
    with pytest.raises(rt.Y3Error, match=r"aux op 0 \(add\) reads tensor \d+ behind the int8 cut, conv 0"):
        net.plan(1, 8, I8)
    assert net.max_batch == 1 and net.dtype == F16 and net.canvas == (8, 8)      # refused before anything was freed
    q = IC.mixed_concat_program()
    net = rt.Net(q)
    net.load_weights(synthetic_weights(q, seed=5))
    net.set_act_scales([0.05] * len(q.tensors))
    net.set_pools_i8(True)
    with pytest.raises(rt.Y3Error, match=r"aux op 0 \(concat\) joins tensor 2 behind the int8 cut, conv 1, with tensor 1 before it"):
        net.plan(1, 8, I8)
    # an aux op behind the cut that reads a net output, and one that writes one
    r, h0 = IC.aux_reads_output_program()
    net = rt.Net(r)
    net.set_act_scales([0.05] * len(r.tensors))
    net.set_pools_i8(True)
    with pytest.raises(rt.Y3Error, match=rf"aux op 0 \(up-sample\) reads tensor {h0}, a net output behind the int8 cut"):
        net.plan(1, 8, I8)
    v, pool = IC.aux_writes_output_program()
    net = rt.Net(v)
    net.set_act_scales([0.05] * len(v.tensors))
    net.set_pools_i8(True)
    with pytest.raises(rt.Y3Error, match=rf"aux op 0 \(max-pool, stride 2\) writes tensor {pool}, a net output"):
        net.plan(1, 8, I8)
    assert net.max_batch == 0 and net.pools_i8 == 0


# ---------------------------------------------------------------------------------------------- 7. streams and drivers
def test_tiny_i8_detect_stream_with_letterbox_equals_detect_composed_by_hand(rt, tiny):
    from tests.test_evaluate_gpu import _detect
    from tests.test_tiny_gpu import STREAM_S, _frames
    anchors = TC.tiny_anchors()
    w, x, _ = _tiny_case(rt, tiny, (96, 96))
    cal = rt.Net(tiny)
    cal.load_weights(w)
    cal.set_pools_i8(True)
    scales = cal.calibrate_i8(torch.rand((2, STREAM_S, STREAM_S, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(3)))
    net = _i8_net(rt, tiny, w, scales, 3, STREAM_S)
    batches = _frames()
    dets = [_detect(rt, net, b, anchors, STREAM_S, LOW, True) for b in batches]
    got = list(net.detect_stream(batches, anchors, 100, 0.5, LOW, letterbox=True))
    assert len(got) == 2 and net.pools_i8 == 1 and net.tiny_stem_fused == 1 and net.dtype == I8
    for (gp, gn), (wp, wn) in zip(got, dets):
        assert np.array_equal(gn, wn) and np.array_equal(gp, wp)
    assert sum(int(wn.sum()) for _, wn in dets) > 0


def test_tiny_i8_evaluate_driver_on_device_with_the_yaml_keys(rt, tiny, tmp_path):
    """evaluate_yolov3.evaluate(on_device=True) on the tiny model config with dtype: i8, i8_pools, tiny_fused_stem and a calibration file:
    its counters are those of sweep_counters over Net.detect composed by hand; without i8_pools the plan is refused as it always was."""
    from tests.helpers import jpeg_bytes
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev
    from yolo_v3_tf2_amd.core import load_tfrecords as m
    from yolo_v3_tf2_amd.evaluate_detections import sweep_counters
    names = [ln.strip() for ln in open(os.path.join(TC.ROOT, "datasets/coco2012/coco.names")) if ln.strip()]
    rng = np.random.default_rng(23)
    payloads = []
    for i in range(4):
        lo = (rng.random((2, 2)) * 0.5).astype(np.float32)
        hi = lo + 0.3
        payloads.append(m.make_example({"image/encoded": jpeg_bytes(rng, 60, 75),
                                        "image/object/class/text": [names[(7 * i + j) % NC].encode() for j in range(2)],
                                        "image/object/bbox/xmin": lo[:, 0], "image/object/bbox/ymin": lo[:, 1],
                                        "image/object/bbox/xmax": hi[:, 0], "image/object/bbox/ymax": hi[:, 1]}))
    d = tmp_path / "set"
    d.mkdir()
    m.write_records(str(d / "set.tfrec"), payloads)
    S = 96
    w, x, scales = _tiny_case(rt, tiny, (96, 96))
    cal = rt.Net(tiny)
    cal.set_act_scales(scales)
    path = str(tmp_path / "tiny_cal.json")
    cal.save_calibration(path)
    cfg = dict(tfrecords_dir=str(d), image_size=S, batch_size=2, yolo_max_boxes=100, nms_iou_threshold=0.5,
               classes_name_file=os.path.join(TC.ROOT, "datasets/coco2012/coco.names"), anchors_file=TC.TINY_ANCHORS,
               model_config_file=TC.TINY_MODEL, dtype="i8", tiny_fused_stem=True, i8_pools=True, i8_calibration=path)
    thresholds = [0.006, LOW]
    dev = ev.evaluate(cfg, thresholds, evaluate_iou_threshold=0.1, weights=w, on_device=True)
    anchors = TC.tiny_anchors()
    net = _i8_net(rt, tiny, w, scales, 2, S)
    data = list(ev.parse_tfrecords(cfg["tfrecords_dir"], image_size=S, max_bboxes=100, class_file=cfg["classes_name_file"]))
    assert len(data) == 4
    total = 0
    for k in (0, 2):
        images = np.stack([np.asarray(data[k + j][0], np.float32) for j in range(2)])
        gt = []
        for j in range(2):
            y = np.asarray(data[k + j][1])
            y = y[y[..., 4] == 1]
            gt.append((y[:, 0:4], y[:, 5].astype(np.int32)))
        packed, nv = net.detect(_cuda(images), anchors, 100, 0.5, min(thresholds))
        gb, gc, cnt = rt.pack_ground_truth(gt, 100)
        total = total + sweep_counters(packed.cpu().numpy(), nv.cpu().numpy(), gb, gc, cnt, NC, 0.1, thresholds)
    for t in range(len(thresholds)):
        want, got = ev.counters_from_row(total[t], NC), dev[t][3]
        assert sorted(want) == sorted(got) and all(np.array_equal(want[k], got[k]) for k in want), t
    assert dev[0][3]["examples"] == 4 and dev[0][3]["preds"].sum() > 0
    with pytest.raises(rt.Y3Error) as e:
        ev.evaluate(dict(cfg, i8_pools=None), thresholds, evaluate_iou_threshold=0.1, weights=w, on_device=True)
    assert OLD_REFUSAL in str(e.value)
