"""Low-latency bf16 plans on the GPU: split-K bf16 convs (csrc/conv_bf16.hip, SPLIT = true + splitk_finish_bf16) against the bf16-emulating
CPU oracle, bit for bit against the unsplit launch where every partial sum is exact, and the invariants of a plan that uses them (bit-stable
results, detect == composed route, graph capture, lanes, refusals).

Bars.  A stored bf16 tensor whose launch reads exact inputs (the net's bf16 input, or the device's own tensors handed to the oracle):
per element one bf16 ulp of the element + 1e-5 |ref|max, the bar of tests/test_gpu_parity.py::
test_bf16_every_layer_teacher_forced_within_one_ulp.  An fp32 head read from the input: 2e-4 max(1, |ref|max), the bar of
test_bf16_conv_layers_match_bf16_oracle.  Every case asserts the slices in force of every conv, so none silently runs unsplit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from yolo_v3_tf2_amd import _lib  # noqa: E402

BF16 = _lib.Y3_DTYPE_BF16


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bf16_in(x):
    from oracle import oracle as O
    return _cuda(O.round_bf16(x)).to(torch.bfloat16)


def _bf16_ulp_elem(a, b):
    """Per element: the spacing of bf16 numbers (8 significand bits) in the binade of the larger of |a|, |b|."""
    m = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.float32(2.0 ** -126)).astype(np.float64)
    return np.ldexp(1.0, np.floor(np.log2(m)).astype(np.int64) - 7)


def _assert_stored(got, ref, what):
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bar = _bf16_ulp_elem(got, ref) + 1e-5 * float(np.abs(ref).max())
    print(f"{what}: worst {float((d / bar).max()):.3f} of the bar, {float((d > 0).mean()):.2e} of the elements differ")
    assert (d <= bar).all(), (what, float((d / bar).max()))


def _assert_head(got, ref, what):
    err, bar = float(np.abs(got - ref).max()), 2e-4 * max(1.0, float(np.abs(ref).max()))
    print(f"{what}: max|diff| = {err:.3e}, bar {bar:.3e}")
    assert err <= bar, (what, err)


def _splits(net):
    return [net.split_k_bf16(i) for i in range(len(net.conv_ops))]


# ---------------------------------------------------------------------------------------------- 1. layers against the bf16 oracle
from tests.splitk_cases import C3, H1, LAYERS_16 as LAYERS  # noqa: E402,F401  -- the table is shared with the host tiers
LAYER_CASES = [
    ("c128_13", 2, 11), ("c128_13", 3, 12), ("c128_13", 4, 11), ("c128_13", 8, 12),
    ("c128_13_head", 2, 12), ("c128_13_head", 3, 11), ("c128_13_head", 4, 12), ("c128_13_head", 8, 11),
    ("c64_13", 2, 11), ("c64_13", 3, 11), ("c64_13", 4, 11), ("c64_13", 8, 11),
    ("c64_13_head", 2, 11), ("c64_13_head", 3, 11), ("c64_13_head", 4, 11), ("c64_13_head", 8, 11),
    ("cin64_13_head", 3, 11),
    ("c128_13_res", 3, 11), ("c128_13_res", 4, 12),
    ("s2_14", 2, 12), ("s2_14_head", 4, 11),
    ("head255", 2, 12), ("head255", 4, 11),
    ("b3_14", 3, 12), ("b3_14", 4, 11), ("b3_14_head", 4, 12),
]
# fixed per case: weights are seeded 500 + n, the input n, whatever runs before
CASE_SEED = {"c128_13": 0, "c128_13_head": 1, "c128_13_res": 2, "s2_14": 3, "s2_14_head": 4, "head255": 5, "b3_14": 6, "b3_14_head": 7,
             "c64_13": 8, "c64_13_head": 9, "cin64_13_head": 10}
_layer_cache = {}


def _layer_setup(name):
    """Program, weights, input and the bf16 oracle's outputs / kept tensors of a layer case: computed once per case name."""
    if name not in _layer_cache:
        from tests.helpers import mini_program
        from yolo_v3_tf2_amd.weights import synthetic_weights
        from oracle import oracle as O
        in_ch, S, B, chain, heads, slots = LAYERS[name]
        p = mini_program(in_ch, chain, heads)
        w = synthetic_weights(p, seed=500 + CASE_SEED[name])
        x = O.round_bf16(np.random.default_rng(CASE_SEED[name]).standard_normal((B, S, S, in_ch)).astype(np.float32))
        convs = list(p.conv_ops())
        keep = {convs[s].dst for s in slots if convs[s].dst not in p.outputs}
        if keep:
            ref, kept = O.forward(p, w, x, bf16=True, keep=keep)
        else:
            ref, kept = O.forward(p, w, x, bf16=True), {}
        for a in list(ref) + list(kept.values()):
            a.setflags(write=False)
        _layer_cache[name] = (p, w, x, ref, kept)
    return _layer_cache[name]


def _layer_net(rt, name, S, tile):
    p, w, x, ref, kept = _layer_setup(name)
    in_ch, size, B, chain, heads, slots = LAYERS[name]
    net = rt.Net(p)
    net.load_weights(w)
    net.keep_activations(True)
    for slot in slots:
        net.set_tile_bf16(slot, tile)
        if S > 1:
            net.set_split_k_bf16(slot, S)
    net.plan(B, size, BF16)
    assert _splits(net) == [S if slot in slots else 1 for slot in range(len(net.conv_ops))]
    assert all(net.split_k(slot) == 1 for slot in range(len(net.conv_ops)))     # the fp32 decision stays out of a bf16 plan
    return net


@pytest.mark.parametrize("name,S,tile", LAYER_CASES)
def test_split_bf16_conv_layers_match_bf16_oracle(rt, name, S, tile):
    p, w, x, ref, kept = _layer_setup(name)
    in_ch, size, B, chain, heads, slots = LAYERS[name]
    net = _layer_net(rt, name, S, tile)
    got = net.forward(_bf16_in(x))
    torch.cuda.synchronize()
    outs = dict(zip(p.outputs, zip(ref, got)))
    for slot in slots:
        t = net.conv_ops[slot].dst
        if t in outs:
            if net.conv_ops[slot].src0 != p.input_tensor:
                continue           # a head behind the stored conv is not teacher-forced; the stored tensor itself is held below
            r, g = outs[t]
            _assert_head(g.cpu().numpy().reshape(r.shape), r, f"{name} S={S} tile={tile} head slot {slot}")
        else:
            g = net.read_tensor(t, B).cpu().numpy()
            _assert_stored(g, kept[t].reshape(g.shape), f"{name} S={S} tile={tile} stored slot {slot}")


# ---------------------------------------------------------------------------------------------- 2. exact sums
def _integer_case(p, w, x_shape, seed):
    """Inputs from the integers in [-4, 4], conv weights from {-1, 0, 1}: every product and every partial sum is an integer below 2^24,
    exact in fp32 in any order, so a split plan must give the unsplit plan's bits."""
    rng = np.random.default_rng(seed)
    w = {k: np.array(v, copy=True) for k, v in w.items()}
    for o in p.conv_ops():
        k = f"conv{o.conv_index}.w"
        w[k][...] = rng.integers(-1, 2, w[k].shape).astype(np.float32)
    x = rng.integers(-4, 5, x_shape).astype(np.float32)
    return w, x


def _run_bits(rt, p, w, x, B, size, split_slots, S, tile, read):
    net = rt.Net(p)
    net.load_weights(w)
    net.keep_activations(True)
    for slot in split_slots:
        net.set_tile_bf16(slot, tile)
        if S > 1:
            net.set_split_k_bf16(slot, S)
    net.plan(B, size, BF16)
    assert _splits(net) == [S if slot in split_slots else 1 for slot in range(len(net.conv_ops))]
    outs = [g.clone() for g in net.forward(x)]
    torch.cuda.synchronize()
    return outs + [net.read_tensor(t, B).clone() for t in read]


@pytest.mark.parametrize("name,tile", [("c128_13", 11), ("c128_13_head", 12), ("c64_13", 11), ("c64_13_head", 11), ("c128_13_res", 12),
                                       ("s2_14", 11), ("b3_14", 12)])
def test_split_bf16_exact_sums_equal_the_unsplit_bits(rt, name, tile):
    p, w0, _, _, _ = _layer_setup(name)
    in_ch, size, B, chain, heads, slots = LAYERS[name]
    w, x = _integer_case(p, w0, (B, size, size, in_ch), 77)
    convs = list(p.conv_ops())
    read = [convs[s].dst for s in slots if convs[s].dst not in p.outputs]
    xin = _cuda(x).to(torch.bfloat16)
    want = _run_bits(rt, p, w, xin, B, size, slots, 1, tile, read)
    assert any(float(t.abs().max()) > 0 for t in want)
    for S in (2, 3, 4, 8):
        got = _run_bits(rt, p, w, xin, B, size, slots, S, tile, read)
        assert all(torch.equal(a, b) for a, b in zip(want, got)), (name, S)


def _concat_program():
    """input [B,14,14,128] -> d = 3x3/2 -> 256 and e = 1x1 -> 256 (both bias 0, linear: integer outputs from integer inputs) ->
    f = 1x1 [up(d), e] -> 128 with BN and leaky: 512 channels, C0 = 256, 8 K tiles -> three 1x1 heads."""
    from tests.helpers import _Graph
    g = _Graph(128)
    d = g.conv(g.input, 256, 3, stride=2, bn=False, act="linear")
    e = g.conv(g.input, 256, 1, bn=False, act="linear")
    f = g.conv(g.route(g.upsample(d), e), 128, 1)
    return g.program([g.conv(f, 64, 1, sub="head") for _ in range(3)]), f


@pytest.mark.parametrize("tile", [11, 12])
def test_split_bf16_concat_exact_sums(rt, tile):
    """S = 2: the slice boundary on the source boundary; 3: slices of 2, 3, 3 tiles, the second straddles the sources; 4, 8: slices inside
    either source.  A tile covered twice, skipped or read from the wrong source cannot give the unsplit bits."""
    from yolo_v3_tf2_amd.weights import synthetic_weights
    p, f = _concat_program()
    convs = list(p.conv_ops())
    slot = next(i for i, o in enumerate(convs) if o.dst == f)
    assert convs[slot].src1 >= 0 and convs[slot].c0 == 256 and convs[slot].cin == 512 and convs[slot].src0_upsample
    w, x = _integer_case(p, synthetic_weights(p, seed=9), (2, 14, 14, 128), 78)
    for o in convs:
        if not o.bn:
            w[f"conv{o.conv_index}.bias"][...] = 0
    xin = _cuda(x).to(torch.bfloat16)
    want = _run_bits(rt, p, w, xin, 2, 14, (slot,), 1, tile, [f])
    assert float(want[-1].abs().max()) > 0
    for S in (2, 3, 4, 8):
        got = _run_bits(rt, p, w, xin, 2, 14, (slot,), S, tile, [f])
        assert all(torch.equal(a, b) for a, b in zip(want, got)), S


# ---------------------------------------------------------------------------------------------- 3. the neck's up-sample + concat 1x1
def test_split_bf16_upsample_concat_conv(rt, program, weights):
    """The real program at 64 x 64, two images: the fused up-sample + concat 1x1 with 384 channels (C0 = 128: 6 K tiles of 64).  S = 3 puts
    a slice boundary on the source boundary, S = 2 starts a slice inside src1, with S = 4 a slice straddles the two sources.  The launch is
    recomputed by the oracle from the device's own input tensors (bf16 weights, rounded where the kernel rounds) and held to the stored bar."""
    from oracle import oracle as O
    from tests.helpers import oracle_launch
    S_img, B = 64, 2
    x = np.random.default_rng(3).random((B, S_img, S_img, 3), dtype=np.float32)
    cat = [(slot, o) for slot, o in enumerate(program.conv_ops()) if o.src1 >= 0 and o.cin == 384]
    assert len(cat) == 1 and cat[0][1].c0 == 128 and cat[0][1].src0_upsample
    slot, o = cat[0]
    net = rt.Net(program)
    net.load_weights(weights)
    net.keep_activations(True)
    net.plan(B, S_img, BF16)
    ref = None
    for S in (1, 3, 2, 4):
        net.set_split_k_bf16(slot, S)        # on a planned net: decided again at once
        assert net.split_k_bf16(slot) == S and sum(s > 1 for s in _splits(net)) == int(S > 1)
        net.forward(_cuda(x))
        if ref is None:                      # the conv's inputs do not depend on its own split
            ref = O.round_bf16(oracle_launch(O, o, weights, lambda t: net.read_tensor(t, B).cpu().numpy(), bf16_weights=True))
        g = net.read_tensor(o.dst, B).cpu().numpy()
        _assert_stored(g, ref.reshape(g.shape), f"concat 1x1 S={S}")
    with pytest.raises(rt.Y3Error, match="K tiles"):
        net.set_split_k_bf16(slot, 7)


# ---------------------------------------------------------------------------------------------- 4. off is the default plan
def test_split_bf16_off_on_every_conv_gives_the_default_plans_bits(rt, program, weights):
    x = _cuda(np.random.default_rng(8).random((1, 64, 64, 3), dtype=np.float32))
    base = rt.Net(program)
    base.load_weights(weights)
    base.plan(1, 64, BF16)
    assert all(s == 1 for s in _splits(base))     # off by default
    want = [g.clone() for g in base.forward(x)]
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_low_latency_bf16(True)
    for i in range(len(net.conv_ops)):
        net.set_split_k_bf16(i, 1)
    net.plan(1, 64, BF16)
    assert all(s == 1 for s in _splits(net))
    got = net.forward(x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    for i in range(len(net.conv_ops)):       # handing the convs back to the heuristic splits some of them
        net.set_split_k_bf16(i, -1)
    assert any(s > 1 for s in _splits(net))
    net.set_low_latency_bf16(False)
    assert all(s == 1 for s in _splits(net))
    again = net.forward(x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(want, again))


# ---------------------------------------------------------------------------------------------- 5. the 75-conv network
@pytest.mark.parametrize("size", [64, (64, 96)])
def test_low_latency_bf16_network(rt, program, weights, anchors, size):
    """The 75-conv network in a low-latency bf16 plan for one image: heads below 1.5e-2 in relative norm against the bf16 oracle (the
    free-running bar of tests/test_rect_gpu.py and test_gpu_parity.py), y3_net_detect bit-identical to the composed route, two runs
    bit-identical, and -- in a plan for two -- image 0 of a two-image call bit-identical to the same image alone."""
    from oracle import oracle as O
    H, W = rt.canvas_hw(size)
    x = np.random.default_rng(21).random((2, H, W, 3), dtype=np.float32)
    ref = O.forward(program, weights, x[:1], bf16=True)
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_low_latency_bf16(True)
    net.plan(1, size, BF16)
    splits = _splits(net)
    print("split_k_bf16 per conv:", splits)
    assert max(splits) > 1 and all(1 <= s <= 16 for s in splits)
    heads = [i for i, o in enumerate(net.conv_ops) if o.dst in program.outputs]
    assert len(heads) == 3 and all(splits[i] == 1 for i in heads) and splits[0] == splits[1] == splits[2] == 1
    x1 = _cuda(x[:1])
    grids = [g.clone() for g in net.forward(x1)]
    torch.cuda.synchronize()
    rel = max(float(np.linalg.norm(g.cpu().numpy().reshape(r.shape) - r) / np.linalg.norm(r)) for g, r in zip(grids, ref))
    print(f"low-latency bf16 grids {size}: relative norm {rel:.3e}")
    assert rel < 1.5e-2
    again = net.forward(x1)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(grids, again))
    bb, cc, ss = rt.yolo_decode_scores(grids, anchors, 80)
    sel, nv = rt.nms_padded(bb, ss, 100, 0.5, 0.05)
    want = rt.pack_detections(bb, cc, ss, sel, nv)
    packed, nv2 = net.detect(x1, anchors, 100, 0.5, 0.05)
    torch.cuda.synchronize()
    assert torch.equal(nv2, nv) and torch.equal(packed, want)
    net2 = rt.Net(program)                   # a plan for two images: the bits of image 0 do not depend on the batch of the call
    net2.load_weights(weights)
    net2.set_low_latency_bf16(True)
    net2.plan(2, size, BF16)
    assert max(_splits(net2)) > 1
    both = [g.clone() for g in net2.forward(_cuda(x))]
    alone = net2.forward(x1)
    torch.cuda.synchronize()
    assert net2.max_batch == 2
    assert all(torch.equal(a[:1], b) for a, b in zip(both, alone))


def test_low_latency_bf16_plan_follows_the_pinned_table(rt, program, weights):
    """Planning only: the slices in force in a low-latency bf16 plan for one 416 x 416 image are the pinned table of
    tests/test_splitk_bf16_host.py, and 1 for every conv the table does not list."""
    from tests.test_splitk_bf16_host import RULE_B1_S416
    table = {shape: want[4] for shape, want in RULE_B1_S416}
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_low_latency_bf16(True)
    net.plan(1, 416, BF16)
    heads = {i for i, o in enumerate(net.conv_ops) if o.dst in program.outputs}
    seen = set()
    for i, o in enumerate(net.conv_ops):
        shape = (o.size, o.cin, o.cout, 416 // o.out_div)
        want = 1 if i in heads else table.get(shape, 1)
        assert net.split_k_bf16(i) == want, (i, shape, net.split_k_bf16(i), want)
        seen.add(shape)
    assert all(shape in seen for shape in table)


# ---------------------------------------------------------------------------------------------- 6. graph and lanes
def test_low_latency_bf16_detect_graph_capture(rt, program, weights, anchors):
    """The split launches and their finish launches enqueue work only: a one-image detect is captured and replayed three times."""
    x = _cuda(np.random.default_rng(31).random((1, 64, 64, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_low_latency_bf16(True)
    net.plan(1, 64, BF16)
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


def test_forced_bf16_splits_two_lanes_equal_one_lane(rt, program, weights):
    """Four images, every eligible conv forced to two slices: two concurrent lanes (each with its own slab workspace) give the bits of one
    lane.  Of the 75 convs, 66 can split: not the first layer, the two Cin = 32 convs, the 64 -> 32 1x1 (a 32-wide tile), the two
    weight-resident 64 -> 128 3x3 convs and the three heads."""
    x = _cuda(np.random.default_rng(41).random((4, 64, 64, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    forced = 0
    for i in range(len(net.conv_ops)):
        try:
            net.set_split_k_bf16(i, 2)
            forced += 1
        except rt.Y3Error:
            pass
    net.plan(4, 64, BF16)
    n_split = sum(s == 2 for s in _splits(net))
    print(f"forced {forced} convs, {n_split} split after planning")
    assert forced >= 60 and n_split == forced
    net.set_lanes(1)
    one = [g.clone() for g in net.forward(x)]
    net.set_lanes(2)
    assert sum(s == 2 for s in _splits(net)) == n_split
    for _ in range(2):
        two = net.forward(x)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(one, two))


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_split_bf16_refusals(rt, program, weights):
    net = rt.Net(program)
    net.load_weights(weights)
    ops = net.conv_ops
    head = next(i for i, o in enumerate(ops) if o.dst in program.outputs)
    with pytest.raises(rt.Y3Error, match="first layer"):
        net.set_split_k_bf16(0, 2)
    with pytest.raises(rt.Y3Error, match="head"):
        net.set_split_k_bf16(head, 2)
    res = next(i for i, o in enumerate(ops) if o.size == 3 and o.stride == 1 and o.cin == 32)
    with pytest.raises(rt.Y3Error, match="tile 32"):
        net.set_split_k_bf16(res, 2)                  # the weight-resident tile
    bk32 = next(i for i, o in enumerate(ops) if o.size == 3 and o.stride == 2 and o.cin == 32)
    with pytest.raises(rt.Y3Error, match="BK = 32"):
        net.set_split_k_bf16(bk32, 2)
    small = next(i for i, o in enumerate(ops) if o.size == 1 and o.cin == 128 and o.cout == 64)
    with pytest.raises(rt.Y3Error, match="K tiles"):
        net.set_split_k_bf16(small, 4)                # 2 K tiles of 64
    net.set_split_k_bf16(small, 2)
    net.set_split_k_bf16(head, 1)                     # "off" is never refused
    net.set_split_k_bf16(head, -1)
    for bad in (0, 17, True, 2.0):
        with pytest.raises(rt.Y3Error):
            net.set_split_k_bf16(small, bad)
    # an fp32 plan takes no bf16 split and refuses a forced value
    net.set_low_latency_bf16(True)
    net.plan(1, 64, _lib.Y3_DTYPE_F32)
    assert all(s == 1 for s in _splits(net)) and all(net.split_k(i) == 1 for i in range(len(ops)))
    with pytest.raises(rt.Y3Error, match="BF16"):
        net.set_split_k_bf16(small, 2)
    # the same net planned bf16 takes the forced value and the heuristic; the fp32 calls keep to fp32 plans
    net.plan(1, 64, BF16)
    assert net.split_k_bf16(small) == 2 and net.split_k_bf16(head) == 1 and net.split_k_bf16(0) == 1
    assert any(s > 2 for s in _splits(net))
    assert all(net.split_k(i) == 1 for i in range(len(ops)))
    with pytest.raises(rt.Y3Error, match="F32"):
        net.set_split_k(small, 2)


# ---------------------------------------------------------------------------------------------- 8. one value in force, requests per mode
def test_one_split_in_force_follows_the_plans_mode(rt, program, weights):
    """ConvSlot::split_k is the one value in force while the requests and switches stay per mode: a net with both switches on and one
    forced split per mode, planned fp32, bf16, fp16 and fp32 again, shows after every plan the slices (own mode's getter; all 1 from the
    other's, all 1 from both on the fp16 plan) and the three grids, bit for bit, of a fresh net planned once in that mode."""
    F32, F16 = _lib.Y3_DTYPE_F32, _lib.Y3_DTYPE_F16
    x = _cuda(np.random.default_rng(51).random((1, 64, 64, 3), dtype=np.float32))

    def make():
        net = rt.Net(program)
        net.load_weights(weights)
        net.set_low_latency(True)
        net.set_low_latency_bf16(True)
        return net

    ops = make().conv_ops
    s32 = next(i for i, o in enumerate(ops) if o.size == 1 and o.cin == 128 and o.cout == 64)     # 4 K tiles of 32
    s16 = next(i for i, o in enumerate(ops) if o.size == 1 and o.cin == 256 and o.cout == 128)    # 4 K tiles of 64
    ones = [1] * len(ops)

    def state(net):
        grids = [g.clone() for g in net.forward(x)]
        torch.cuda.synchronize()
        return [net.split_k(i) for i in range(len(ops))], _splits(net), grids

    fresh = {}
    for dtype in (BF16, F16, F32):     # the fp32 one, fresh here, is the net that is planned again below
        net = make()
        net.set_split_k(s32, 4)
        net.set_split_k_bf16(s16, 2)
        net.plan(1, 64, dtype)
        fresh[dtype] = state(net)
    assert fresh[F32][0][s32] == 4 and any(s > 1 for i, s in enumerate(fresh[F32][0]) if i != s32) and fresh[F32][1] == ones
    assert fresh[BF16][1][s16] == 2 and any(s > 1 for i, s in enumerate(fresh[BF16][1]) if i != s16) and fresh[BF16][0] == ones
    assert fresh[F16][0] == ones and fresh[F16][1] == ones
    for dtype in (BF16, F16, F32):
        net.plan(1, 64, dtype)
        f32_splits, bf16_splits, grids = state(net)
        assert f32_splits == fresh[dtype][0] and bf16_splits == fresh[dtype][1], dtype
        assert all(torch.equal(a, b) for a, b in zip(grids, fresh[dtype][2])), dtype
