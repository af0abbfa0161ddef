"""Low-latency fp16 plans on the GPU: split-K fp16 convs (csrc/conv_16bit.h: SPLIT = true + splitk_finish16, instantiated for F16Elem by
csrc/conv_f16.hip; y3_net_set_low_latency_f16 / y3_net_set_split_k_f16) against the fp16-emulating oracle, bit for bit against the unsplit
launch where every partial sum is exact, and the invariants of a plan that uses them.  The cases are those of
tests/test_splitk_bf16_gpu.py with fp16 inputs.

Bars: a stored fp16 output under _stored_check of tests/test_f16_gpu.py (f16_ulp_elem + 1e-5 |ref|max of round_f16 of the
double-accumulating reference, at most 1e-2 of the elements different at all); an fp32 head within 2e-5 max(1, |ref|max).  Every case
asserts the slices in force of every conv, so none silently runs unsplit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.f16_oracle import f16_emulation, forward_f16, rel_l2, round_f16  # noqa: E402
from tests.helpers import oracle_launch  # noqa: E402
from tests.test_f16_gpu import _stored_check  # noqa: E402
from tests.test_splitk_bf16_gpu import CASE_SEED, LAYER_CASES, LAYERS, _concat_program, _integer_case  # noqa: E402
from yolo_v3_tf2_amd import _lib  # noqa: E402

F16, BF16 = _lib.Y3_DTYPE_F16, _lib.Y3_DTYPE_BF16


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _splits(net):
    return [net.split_k_f16(i) for i in range(len(net.conv_ops))]


def _others_stay_out(net):
    return all(net.split_k(i) == 1 and net.split_k_bf16(i) == 1 for i in range(len(net.conv_ops)))


# ---------------------------------------------------------------------------------------------- 1. layers against the fp16 oracle
_layer_cache = {}


def _layer_setup(name):
    """Program, weights, fp16-exact input and, per split slot, the double-accumulating reference of its launch (the split convs read the
    net's input and take their shortcut from it: teacher-forced).  Computed once per case name, left read-only."""
    if name not in _layer_cache:
        from oracle import oracle as O
        from tests.helpers import mini_program
        from yolo_v3_tf2_amd.weights import synthetic_weights
        in_ch, S, B, chain, heads, slots = LAYERS[name]
        p = mini_program(in_ch, chain, heads)
        w = synthetic_weights(p, seed=500 + CASE_SEED[name])
        x = round_f16(np.random.default_rng(CASE_SEED[name]).standard_normal((B, S, S, in_ch)).astype(np.float32))
        convs = list(p.conv_ops())
        refs = {}
        with f16_emulation():
            for s in slots:
                assert convs[s].src0 == p.input_tensor
                refs[s] = oracle_launch(O, convs[s], w, {p.input_tensor: x}.__getitem__, acc64=True, bf16_weights=True)
                refs[s].setflags(write=False)
        _layer_cache[name] = (p, w, x, refs)
    return _layer_cache[name]


@pytest.mark.parametrize("name,S,tile", LAYER_CASES)
def test_split_f16_conv_layers_match_f16_oracle(rt, name, S, tile):
    p, w, x, refs = _layer_setup(name)
    in_ch, size, B, chain, heads, slots = LAYERS[name]
    net = rt.Net(p)
    net.load_weights(w)
    net.keep_activations(True)
    for slot in slots:
        net.set_tile_bf16(slot, tile)        # the 16-bit plans share the forced tile
        net.set_split_k_f16(slot, S)
    net.plan(B, size, F16)
    assert _splits(net) == [S if slot in slots else 1 for slot in range(len(net.conv_ops))]
    assert _others_stay_out(net)
    got = net.forward(_cuda(x).to(torch.float16))
    torch.cuda.synchronize()
    outs = dict(zip(p.outputs, got))
    for slot in slots:
        t, r = net.conv_ops[slot].dst, refs[slot]
        if t in outs:
            g = outs[t].cpu().numpy().reshape(r.shape)
            err, bar = float(np.abs(g - r).max()), 2e-5 * max(1.0, float(np.abs(r).max()))
            print(f"{name} S={S} tile={tile} head slot {slot}: max|diff| = {err:.3e}, bar {bar:.3e}")
            assert err <= bar, (name, slot, err, bar)
        else:
            g = net.read_tensor(t, B).cpu().numpy()
            worst, frac = _stored_check(g, r.reshape(g.shape), 1e-2, (name, S, tile, slot))
            print(f"{name} S={S} tile={tile} stored slot {slot}: worst {worst:.3f} of the bar, {frac:.2e} of the elements differ")


# ---------------------------------------------------------------------------------------------- 2. exact sums
def _run_bits(rt, p, w, x, B, size, split_slots, S, tile, read):
    net = rt.Net(p)
    net.load_weights(w)
    net.keep_activations(True)
    for slot in split_slots:
        net.set_tile_bf16(slot, tile)
        if S > 1:
            net.set_split_k_f16(slot, S)
    net.plan(B, size, F16)
    assert _splits(net) == [S if slot in split_slots else 1 for slot in range(len(net.conv_ops))]
    outs = [g.clone() for g in net.forward(x)]
    torch.cuda.synchronize()
    return outs + [net.read_tensor(t, B).clone() for t in read]


@pytest.mark.parametrize("name,tile", [("c128_13", 11), ("c128_13", 12), ("c128_13_head", 12), ("c64_13", 11), ("c64_13_head", 11),
                                       ("c128_13_res", 11), ("c128_13_res", 12), ("s2_14", 11), ("b3_14", 12)])
def test_split_f16_exact_sums_equal_the_unsplit_bits(rt, name, tile):
    """Inputs from the integers in [-4, 4], weights from {-1, 0, 1}: every partial sum is exact in fp32 in any order (and below 2048 x 18,
    far inside fp16's range after the BN of the synthetic weights), so a split plan must give the unsplit plan's bits."""
    p, w0, _, _ = _layer_setup(name)
    in_ch, size, B, chain, heads, slots = LAYERS[name]
    w, x = _integer_case(p, w0, (B, size, size, in_ch), 77)
    convs = list(p.conv_ops())
    read = [convs[s].dst for s in slots if convs[s].dst not in p.outputs]
    xin = _cuda(x).to(torch.float16)
    want = _run_bits(rt, p, w, xin, B, size, slots, 1, tile, read)
    assert any(float(t.abs().max()) > 0 for t in want) and all(bool(torch.isfinite(t).all()) for t in want)
    for S in (2, 3, 4, 8):
        got = _run_bits(rt, p, w, xin, B, size, slots, S, tile, read)
        assert all(torch.equal(a, b) for a, b in zip(want, got)), (name, S)


@pytest.mark.parametrize("tile", [11, 12])
def test_split_f16_concat_exact_sums(rt, tile):
    """Through the fused up-sample + concat gather (512 channels, C0 = 256, 8 K tiles): slice boundaries on, beside and across the source
    boundary.  A tile covered twice, skipped or read from the wrong source cannot give the unsplit bits."""
    from yolo_v3_tf2_amd.weights import synthetic_weights
    p, f = _concat_program()
    convs = list(p.conv_ops())
    slot = next(i for i, o in enumerate(convs) if o.dst == f)
    w, x = _integer_case(p, synthetic_weights(p, seed=9), (2, 14, 14, 128), 78)
    for o in convs:
        if not o.bn:
            w[f"conv{o.conv_index}.bias"][...] = 0
    xin = _cuda(x).to(torch.float16)
    want = _run_bits(rt, p, w, xin, 2, 14, (slot,), 1, tile, [f])
    assert float(want[-1].abs().max()) > 0 and bool(torch.isfinite(want[-1]).all())
    for S in (2, 3, 4, 8):
        got = _run_bits(rt, p, w, xin, 2, 14, (slot,), S, tile, [f])
        assert all(torch.equal(a, b) for a, b in zip(want, got)), S


# ---------------------------------------------------------------------------------------------- 3. the low-latency network
@pytest.mark.parametrize("size,B", [(416, 1), (64, 2)])
def test_low_latency_f16_network(rt, program, weights, anchors, size, B):
    """The 75-conv network in a low-latency fp16 plan: the slices are those of a low-latency bf16 plan of the same net (the same rule on
    the same inputs), the heads stay as close to the fp16 oracle as the default fp16 plan's bar asks at 64 x 64, two runs are bit-identical,
    y3_net_detect is the composed route, and image 0 of a batch is the image alone."""
    x = _cuda(np.random.default_rng(21).random((B, size, size, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_low_latency_f16(True)
    net.set_low_latency_bf16(True)
    net.plan(B, size, BF16)
    want_splits = [net.split_k_bf16(i) for i in range(len(net.conv_ops))]
    assert all(s == 1 for s in _splits(net))
    net.plan(B, size, F16)
    splits = _splits(net)
    print(f"split_k_f16 per conv, {B} x {size}^2:", splits)
    assert splits == want_splits and max(splits) > 1 and _others_stay_out(net)
    heads = [i for i, o in enumerate(net.conv_ops) if o.dst in program.outputs]
    assert len(heads) == 3 and all(splits[i] == 1 for i in heads) and splits[0] == splits[1] == splits[2] == 1
    grids = [g.clone() for g in net.forward(x)]
    again = net.forward(x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(grids, again)) and all(bool(torch.isfinite(g).all()) for g in grids)
    if size == 64:
        ref = forward_f16(program, weights, x.cpu().numpy())
        ref64 = forward_f16(program, weights, x.cpu().numpy(), acc64=True)
        for k, (g, r, r64) in enumerate(zip(grids, ref, ref64)):
            rel, floor = rel_l2(g.cpu().numpy().reshape(r.shape), r), rel_l2(r64, r)
            print(f"low-latency f16 head {k}: rel {rel:.3e} against the fp16 oracle, floor {floor:.3e}")
            assert rel <= 2.0 * floor, (k, rel, floor)         # the bar of test_f16_network_free_running: another order of the same sums
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
    # everything off again: the default plan's bits
    base = rt.Net(program)
    base.load_weights(weights)
    base.plan(B, size, F16)
    assert all(s == 1 for s in _splits(base))
    default = [g.clone() for g in base.forward(x)]
    net.set_low_latency_f16(False)
    assert all(s == 1 for s in _splits(net))
    off = net.forward(x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(default, off))
    assert any(not torch.equal(a, b) for a, b in zip(default, grids))   # and the split plan was another summation order


def test_low_latency_f16_detect_graph_capture(rt, program, weights, anchors):
    """The split launches and their finish launches enqueue work only: a one-image detect is captured and replayed three times."""
    x = _cuda(np.random.default_rng(31).random((1, 64, 64, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_low_latency_f16(True)
    net.plan(1, 64, F16)
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


def test_forced_f16_splits_two_lanes_equal_one_lane(rt, program, weights):
    """Four images, every eligible conv forced to two slices: two concurrent lanes (each with its own slab workspace) give one lane's bits."""
    x = _cuda(np.random.default_rng(41).random((4, 64, 64, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    forced = 0
    for i in range(len(net.conv_ops)):
        try:
            net.set_split_k_f16(i, 2)
            forced += 1
        except rt.Y3Error:
            pass
    net.plan(4, 64, F16)
    n_split = sum(s == 2 for s in _splits(net))
    assert forced >= 60 and n_split == forced
    net.set_lanes(1)
    one = [g.clone() for g in net.forward(x)]
    net.set_lanes(2)
    assert sum(s == 2 for s in _splits(net)) == n_split
    for _ in range(2):
        two = net.forward(x)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(one, two))


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_split_f16_refusals(rt, program, weights):
    net = rt.Net(program)
    net.load_weights(weights)
    ops = net.conv_ops
    head = next(i for i, o in enumerate(ops) if o.dst in program.outputs)
    with pytest.raises(rt.Y3Error, match="y3_net_set_split_k_f16.*first layer"):
        net.set_split_k_f16(0, 2)
    with pytest.raises(rt.Y3Error, match="head"):
        net.set_split_k_f16(head, 2)
    res = next(i for i, o in enumerate(ops) if o.size == 3 and o.stride == 1 and o.cin == 32)
    with pytest.raises(rt.Y3Error, match="tile 32"):
        net.set_split_k_f16(res, 2)                   # the weight-resident tile
    bk32 = next(i for i, o in enumerate(ops) if o.size == 3 and o.stride == 2 and o.cin == 32)
    with pytest.raises(rt.Y3Error, match="BK = 32"):
        net.set_split_k_f16(bk32, 2)
    small = next(i for i, o in enumerate(ops) if o.size == 1 and o.cin == 128 and o.cout == 64)
    with pytest.raises(rt.Y3Error, match="K tiles"):
        net.set_split_k_f16(small, 4)                 # 2 K tiles of 64
    net.set_split_k_f16(small, 2)
    net.set_split_k_f16(head, 1)                      # "off" is never refused
    net.set_split_k_f16(head, -1)
    for bad in (0, 17, True, 2.0):
        with pytest.raises(rt.Y3Error):
            net.set_split_k_f16(small, bad)
    with pytest.raises(rt.Y3Error, match="0 or 1"):
        rt.check(net.lib.y3_net_set_low_latency_f16(net._h, 2), "y3_net_set_low_latency_f16")
    # a bf16 plan takes no fp16 split and refuses a forced value; its own getter and the fp32 one answer 1 for the fp16 request
    net.set_low_latency_f16(True)
    net.plan(1, 64, BF16)
    assert all(s == 1 for s in _splits(net)) and _others_stay_out(net)
    with pytest.raises(rt.Y3Error, match="only Y3_DTYPE_F16 plans take an fp16 split"):
        net.set_split_k_f16(small, 2)
    net.plan(1, 64, _lib.Y3_DTYPE_F32)
    assert all(s == 1 for s in _splits(net))
    with pytest.raises(rt.Y3Error, match="only Y3_DTYPE_F16 plans take an fp16 split"):
        net.set_split_k_f16(small, 3)
    # the same net planned fp16 takes the forced value and the rule; the other modes' calls keep to their plans
    net.plan(1, 64, F16)
    assert net.split_k_f16(small) == 2 and net.split_k_f16(head) == 1 and net.split_k_f16(0) == 1
    assert any(s > 2 for s in _splits(net)) and _others_stay_out(net)
    with pytest.raises(rt.Y3Error, match="only Y3_DTYPE_BF16 plans take a bf16 split"):
        net.set_split_k_bf16(small, 2)
    with pytest.raises(rt.Y3Error, match="F32"):
        net.set_split_k(small, 2)
