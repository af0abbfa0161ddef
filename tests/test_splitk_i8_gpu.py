"""Low-latency int8 plans on the GPU: split-K int8 convs (csrc/conv_16bit.h: SPLIT = true for I8Elem; csrc/conv_i8.hip: splitk_finish_i8,
launch_conv_i8_split; y3_net_set_low_latency_i8 / y3_net_set_split_k_i8) against the NumPy restatement yolo_v3_tf2_amd/quant.py and
against the unsplit plan.  The slabs hold i32 sums and integer sums do not depend on order, so a split conv must give the unsplit conv's
bits on all data and at every S: EVERY comparison here is torch.equal / np.array_equal, no tolerance anywhere.  Every case asserts the
slices in force of every conv, so none silently runs unsplit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests import splitk_i8_cases as C  # noqa: E402
from tests.test_i8_gpu import MATRIX_CANVASES, _check_convs, _cuda, _matrix_case  # noqa: E402
from yolo_v3_tf2_amd import _lib, quant  # noqa: E402

I8, F16, BF16, F32 = _lib.Y3_DTYPE_I8, _lib.Y3_DTYPE_F16, _lib.Y3_DTYPE_BF16, _lib.Y3_DTYPE_F32
BK = 128


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _splits(net):
    return [net.split_k_i8(i) for i in range(len(net.conv_ops))]


def _others_stay_out(net):
    return all(net.split_k(i) == 1 and net.split_k_bf16(i) == 1 and net.split_k_f16(i) == 1 for i in range(len(net.conv_ops)))


def _k_tiles(o):
    return o.size * o.size * o.cin // BK


def _stored(net, p, B, first=0):
    """The bytes of every int8 tensor a conv from slot `first` on stores."""
    return [net.read_tensor_i8(o.dst, B).clone() for o in p.conv_ops()[first:] if not quant.writes_f32(p, o)]


# ---------------------------------------------------------------------------------------------- 1. every launch form
def _matrix_run(rt, B, canvas, tile, S):
    """The seven-conv program with `tile` forced everywhere and S slices forced on every conv with at least S K tiles (S = 1: none)."""
    p, w, x, scales = _matrix_case(rt, B, canvas)
    net = rt.Net(p)
    net.load_weights(w)
    net.set_act_scales(scales)
    want = []
    for slot, o in enumerate(net.conv_ops):
        net.set_tile_bf16(slot, tile)       # every conv of the program is 128, 255 or 256 wide: tiles 11 and 12 divide them all
        if S > 1 and _k_tiles(o) >= S:
            net.set_split_k_i8(slot, S)
            want.append(S)
        else:
            if S > 1:
                with pytest.raises(rt.Y3Error, match="K tiles"):
                    net.set_split_k_i8(slot, S)
            want.append(1)
    net.keep_activations(True)
    net.plan(B, canvas, I8)
    assert net.i8_first_conv() == 0
    assert _splits(net) == want and _others_stay_out(net)
    xin = _cuda(x).to(torch.float16)
    first = [g.clone() for g in net.forward(xin)]
    grids = net.forward(xin)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, grids)), "two forwards of one plan differ"
    assert _check_convs(net, p, w, scales, B, grids, 0) == 7
    return want, first, _stored(net, p, B)


@pytest.mark.parametrize("B,canvas", MATRIX_CANVASES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("tile", [11, 12])
def test_split_i8_every_launch_form_bit_exact(rt, tile, B, canvas):
    """a (1 K tile) and h2 (1) never split; b: 18 K tiles with the int8 shortcut; d: stride 2, 9; f: up-sample + concat 128 (+) 256, 3 K
    tiles, so S = 2 cuts beside the source boundary and S = 3 on it; h0 (Cout 255, 2 K tiles), h1 (18): the fp32-output finish."""
    base_splits, base_grids, base_bytes = _matrix_run(rt, B, canvas, tile, 1)
    assert base_splits == [1] * 7
    p = _matrix_case(rt, B, canvas)[0]
    kt = [_k_tiles(o) for o in p.conv_ops()]
    assert kt == [1, 18, 9, 3, 2, 18, 1]
    for S in (2, 3, 4, 8):
        splits, grids, stored = _matrix_run(rt, B, canvas, tile, S)
        assert splits == [S if k >= S else 1 for k in kt] and max(splits) == S
        assert all(torch.equal(a, b) for a, b in zip(base_grids, grids)), (tile, S)
        assert len(stored) == len(base_bytes) == 4 and all(torch.equal(a, b) for a, b in zip(base_bytes, stored)), (tile, S)


# ---------------------------------------------------------------------------------------------- 2. the slabs are integers
def test_split_i8_slabs_hold_integers_beyond_2_to_24(rt):
    """tests/splitk_i8_cases.py::wide512_case: the sums of single slices lie beyond 2^24 (tests/test_splitk_i8_host.py shows that float32
    slabs would change fp32-output elements at S = 2 and at S = 3).  Bit-equal to quant.py and to the unsplit plan."""
    case, xq, ref = C.get()
    p = case.program
    slots = {t: next(i for i, o in enumerate(p.conv_ops()) if o.dst == t) for t in (case.stored["a"], case.heads["h"])}
    got = {}
    for S in (1,) + C.WIDE_SPLITS:
        net = rt.Net(p)
        net.load_weights(case.weights)
        net.set_act_scales(case.scales)
        for slot in range(len(net.conv_ops)):
            net.set_tile_bf16(slot, C.WIDE_TILE)
        if S > 1:
            for slot in slots.values():
                net.set_split_k_i8(slot, S)
        net.keep_activations(True)
        net.plan(case.B, case.canvas, I8)
        assert _splits(net) == [S if i in slots.values() else 1 for i in range(len(net.conv_ops))] and _others_stay_out(net)
        grids = [g.clone() for g in net.forward(_cuda(case.x).to(torch.float16))]
        torch.cuda.synchronize()
        assert np.array_equal(net.read_tensor_i8(p.input_tensor, case.B).cpu().numpy(), xq)
        assert _check_convs(net, p, case.weights, case.scales, case.B, grids, 0) == len(p.conv_ops())
        a = net.read_tensor_i8(case.stored["a"], case.B).clone()
        assert np.array_equal(a.cpu().numpy(), ref[case.stored["a"]]), S
        for t, g in zip(p.outputs, grids):
            assert np.array_equal(g.cpu().numpy().reshape(ref[t].shape), ref[t]), (S, t)
        got[S] = grids + [a]
    for S in C.WIDE_SPLITS:
        assert all(torch.equal(u, v) for u, v in zip(got[1], got[S])), S


# ---------------------------------------------------------------------------------------------- 3. the low-latency network
@pytest.fixture(scope="module")
def scales96(rt, program, weights):
    """The activation scales of the 75-conv network, calibrated as real96 of tests/test_i8_gpu.py does."""
    x = np.random.default_rng(1234).random((2, 96, 96, 3), dtype=np.float32)
    cal = rt.Net(program)
    cal.load_weights(weights)
    return cal.calibrate_i8(_cuda(x))


def _i8_net(rt, program, weights, scales, keep=False):
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_act_scales(scales)
    if keep:
        net.keep_activations(True)
    return net


@pytest.mark.parametrize("size,B", [(416, 1), (64, 2)])
def test_low_latency_i8_network(rt, program, weights, anchors, scales96, size, B):
    """The 75-conv network in a low-latency int8 plan: which convs split (at one 416 x 416 image: the pinned table of
    tests/test_splitk_i8_host.py), and the results ARE the default int8 plan's -- grids and every stored int8 tensor -- since the sums
    are exact; y3_net_detect is the composed route, image 0 of a batch is the image alone, switching off restores the unsplit launches."""
    x = _cuda(np.random.default_rng(21).random((B, size, size, 3), dtype=np.float32))
    net = _i8_net(rt, program, weights, scales96, keep=True)
    net.set_low_latency_i8(True)
    net.plan(B, size, I8)
    cut = net.i8_first_conv()
    assert cut == 9
    splits = _splits(net)
    print(f"split_k_i8 per conv, {B} x {size}^2:", splits)
    heads = [i for i, o in enumerate(net.conv_ops) if o.dst in program.outputs]
    assert max(splits) > 1 and _others_stay_out(net)
    assert len(heads) == 3 and all(splits[i] == 1 for i in heads) and all(s == 1 for s in splits[:cut])
    if (size, B) == (416, 1):
        from tests.test_splitk_i8_host import RULE_B1_S416
        table = {shape: want[4] for shape, want in RULE_B1_S416}
        for i, o in enumerate(net.conv_ops):
            shape = (o.size, o.cin, o.cout, 416 // o.out_div)
            want = 1 if i in heads or i < cut else table[shape]
            assert splits[i] == want, (i, shape, splits[i], want)
    grids = [g.clone() for g in net.forward(x)]
    again = net.forward(x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(grids, again)) and all(bool(torch.isfinite(g).all()) for g in grids)
    stored = _stored(net, program, B, cut)
    # the default int8 plan: the same bits everywhere
    base = _i8_net(rt, program, weights, scales96, keep=True)
    base.plan(B, size, I8)
    assert all(s == 1 for s in _splits(base))
    default = [g.clone() for g in base.forward(x)]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(default, grids))
    base_stored = _stored(base, program, B, cut)
    assert len(stored) == len(base_stored) == len(net.conv_ops) - cut - 3
    assert all(torch.equal(a, b) for a, b in zip(base_stored, stored))
    assert all(int(t.abs().max()) > 8 for t in stored)          # not a comparison of empty buffers
    # detect against the composed route
    bb, cc, ss = rt.yolo_decode_scores(grids, anchors, 80)
    sel, nv = rt.nms_padded(bb, ss, 100, 0.5, 0.05)
    want = rt.pack_detections(bb, cc, ss, sel, nv)
    packed, nv2 = net.detect(x, anchors, 100, 0.5, 0.05)
    torch.cuda.synchronize()
    assert torch.equal(nv2, nv) and torch.equal(packed, want)
    if B > 1:
        alone = net.forward(x[0:1].contiguous())
        torch.cuda.synchronize()
        assert all(torch.equal(a[0:1], b) for a, b in zip(grids, alone))
    # the other modes' switches still do not act on an int8 plan, and this one acts on no other plan
    net.set_low_latency(True)
    net.set_low_latency_bf16(True)
    net.set_low_latency_f16(True)
    assert _splits(net) == splits and _others_stay_out(net)
    # off again: all ones, the same bits
    net.set_low_latency_i8(False)
    assert all(s == 1 for s in _splits(net))
    off = net.forward(x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(default, off))


def test_forced_i8_splits_two_lanes_equal_one_lane(rt, program, weights, scales96):
    """Four images, every eligible conv forced to two slices: two concurrent lanes (each with its own slab workspace) give one lane's bits."""
    x = _cuda(np.random.default_rng(41).random((4, 64, 64, 3), dtype=np.float32))
    net = _i8_net(rt, program, weights, scales96)
    forced = set()
    for i in range(len(net.conv_ops)):
        try:
            net.set_split_k_i8(i, 2)
            forced.add(i)
        except rt.Y3Error:
            pass
    net.plan(4, 64, I8)
    cut = net.i8_first_conv()
    # a request on a conv that this plan runs in fp16 (before the cut) is not acted on; every int8 conv but the heads takes it
    want = [2 if i in forced and i >= cut else 1 for i in range(len(net.conv_ops))]
    assert _splits(net) == want and sum(s == 2 for s in want) == len(net.conv_ops) - cut - 3
    net.set_lanes(1)
    one = [g.clone() for g in net.forward(x)]
    net.set_lanes(2)
    assert _splits(net) == want
    for _ in range(2):
        two = net.forward(x)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(one, two))


def test_low_latency_i8_detect_graph_capture(rt, program, weights, anchors, scales96):
    """The split launches and their finish launches enqueue work only: a one-image detect is captured and replayed three times."""
    x = _cuda(np.random.default_rng(31).random((1, 64, 64, 3), dtype=np.float32))
    net = _i8_net(rt, program, weights, scales96)
    net.set_low_latency_i8(True)
    net.plan(1, 64, I8)
    assert any(s > 1 for s in _splits(net))
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


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_split_i8_refusals(rt, program, weights, scales96):
    net = _i8_net(rt, program, weights, scales96)
    ops = net.conv_ops
    head = next(i for i, o in enumerate(ops) if o.dst in program.outputs)
    with pytest.raises(rt.Y3Error, match="y3_net_set_split_k_i8.*first layer"):
        net.set_split_k_i8(0, 2)
    with pytest.raises(rt.Y3Error, match="head"):
        net.set_split_k_i8(head, 2)
    small = next(i for i, o in enumerate(ops) if o.size == 1 and o.cin == 256 and o.cout == 128)
    with pytest.raises(rt.Y3Error, match="K tiles"):
        net.set_split_k_i8(small, 4)                  # 2 K tiles of 128
    net.set_split_k_i8(small, 2)
    big = next(i for i, o in enumerate(ops) if o.size == 3 and o.stride == 1 and o.cin == 512)
    net.set_tile_bf16(big, 29)                        # a 16x16x64 tile: no split form
    with pytest.raises(rt.Y3Error, match="no split form"):
        net.set_split_k_i8(big, 2)
    for slot in (0, head, big):                       # "off" and "the rule" are never refused
        net.set_split_k_i8(slot, 1)
        net.set_split_k_i8(slot, -1)
    for bad in (0, 17, -2, True, 2.0):
        with pytest.raises(rt.Y3Error):
            net.set_split_k_i8(small, bad)
    with pytest.raises(rt.Y3Error, match="0 or 1"):
        rt.check(net.lib.y3_net_set_low_latency_i8(net._h, 2), "y3_net_set_low_latency_i8")
    with pytest.raises(rt.Y3Error, match="-1, 1 or 2..16"):
        rt.check(net.lib.y3_net_set_split_k_i8(net._h, small, 17), "y3_net_set_split_k_i8")
    # plans of the other modes take no int8 split and refuse a forced value
    net.set_low_latency_i8(True)
    for dtype in (F16, BF16, F32):
        net.plan(1, 64, dtype)
        assert all(s == 1 for s in _splits(net)) and _others_stay_out(net)
        with pytest.raises(rt.Y3Error, match="only Y3_DTYPE_I8 plans take an int8 split"):
            net.set_split_k_i8(small, 3 if dtype == F32 else 2)
        net.set_split_k_i8(big, 1)                    # off and the rule are taken on any plan
        net.set_split_k_i8(big, -1)
    # the same net planned int8: the value forced on `small` before, the rule elsewhere; the forced 16x16x64 tile keeps its conv unsplit
    net.plan(1, 64, I8)
    cut = net.i8_first_conv()
    splits = _splits(net)
    assert splits[small] == 2 and splits[head] == 1 and splits[big] == 1 and max(splits) > 2 and _others_stay_out(net)
    with pytest.raises(rt.Y3Error, match="no split form"):
        net.set_split_k_i8(big, 2)                    # its tile at the planned rows
    before = next(i for i, o in enumerate(ops) if 0 < i < cut and o.size == 3 and o.cin == 64)     # 4.5 K tiles of 128, were it int8
    with pytest.raises(rt.Y3Error, match="runs in fp16 in this plan"):
        net.set_split_k_i8(before, 2)
    net.set_split_k_i8(before, 1)
    net.set_split_k_i8(before, -1)
    with pytest.raises(rt.Y3Error, match="only Y3_DTYPE_F16 plans take an fp16 split"):
        net.set_split_k_f16(before, 2)                # nor do the fp16 calls reach the fp16 convs of an int8 plan
    with pytest.raises(rt.Y3Error, match="only Y3_DTYPE_BF16 plans take a bf16 split"):
        net.set_split_k_bf16(small, 2)
    with pytest.raises(rt.Y3Error, match="F32"):
        net.set_split_k(small, 2)
    assert _splits(net) == splits
