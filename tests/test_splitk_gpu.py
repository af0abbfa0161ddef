"""Low-latency fp32 plans on the GPU: split-K convs (csrc/conv_f32.hip, SPLIT = true + splitk_finish_f32) against the CPU oracle,
and the invariants of a plan that uses them (bit-stable results, detect == composed route, graph capture, lanes, refusals).

Layer bar: |diff| <= 2e-5 * max(1, |ref|max), the figure of tests/test_gpu_parity.py::test_conv_layers_match_oracle for a reordered
fp32 sum over K <= 4608.  Every layer case asserts the number of slices in force, so none silently runs unsplit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from yolo_v3_tf2_amd import _lib  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bar(r):
    return 2e-5 * max(1.0, float(np.abs(r).max()))


from tests.splitk_cases import C3, LAYERS_F32 as LAYERS  # noqa: E402,F401  -- the table is shared with the host tiers
LAYER_CASES = [
    ("c64_13", 2, 11), ("c64_13", 3, 11), ("c64_13", 4, 11), ("c64_13", 8, 11),
    ("c64_13_res", 3, 11), ("c64_13_res", 4, 11),
    ("c256_13", 2, 10), ("c256_13", 4, 10), ("c256_13", 9, 10), ("c256_13", 4, 11), ("c256_13", 9, 11),
    ("s2_14", 2, 10), ("s2_14", 4, 11),
    ("head255", 2, 10), ("head255", 4, 11),
    ("b3_14", 3, 10), ("b3_14", 4, 11),
]
_layer_cache = {}


def _layer_setup(name):
    """Program, weights, input and the oracle's outputs / kept tensors of a layer case: computed once per case name."""
    if name not in _layer_cache:
        from tests.helpers import mini_program
        from yolo_v3_tf2_amd.weights import synthetic_weights
        from oracle import oracle as O
        in_ch, S, B, chain, heads, slots = LAYERS[name]
        p = mini_program(in_ch, chain, heads)
        w = synthetic_weights(p, seed=300 + len(_layer_cache))
        x = np.random.default_rng(len(_layer_cache)).standard_normal((B, S, S, in_ch)).astype(np.float32)
        convs = list(p.conv_ops())
        keep = {convs[s].dst for s in slots}
        ref, kept = O.forward(p, w, x, keep=keep)
        for a in list(ref) + list(kept.values()):
            a.setflags(write=False)
        _layer_cache[name] = (p, w, x, ref, kept)
    return _layer_cache[name]


@pytest.mark.parametrize("name,S,tile", LAYER_CASES)
def test_split_conv_layers_match_oracle(rt, name, S, tile):
    p, w, x, ref, kept = _layer_setup(name)
    in_ch, size, B, chain, heads, slots = LAYERS[name]
    net = rt.Net(p)
    net.load_weights(w)
    net.keep_activations(True)
    for slot in slots:
        net.set_tile(slot, tile)
        net.set_split_k(slot, S)
    net.plan(B, size)
    for slot in range(len(net.conv_ops)):
        assert net.split_k(slot) == (S if slot in slots else 1), slot
    got = net.forward(_cuda(x))
    torch.cuda.synchronize()
    for slot in slots:
        t = net.conv_ops[slot].dst
        if t in p.outputs:      # a head of the mini program: compared below
            continue
        g = net.read_tensor(t, B).cpu().numpy()
        err = float(np.abs(g - kept[t].reshape(g.shape)).max())
        print(f"{name} S={S} tile={tile} slot={slot}: max|diff| = {err:.3e}, bar {_bar(kept[t]):.3e}")
        assert err <= _bar(kept[t]), (name, S, tile, slot, err)
    for r, g in zip(ref, got):
        g = g.cpu().numpy().reshape(r.shape)
        assert np.abs(g - r).max() <= _bar(r), (name, S, tile, float(np.abs(g - r).max()))


def test_split_upsample_concat_conv(rt, program, weights):
    """The neck's fused upsample + concat 1x1 (C0 = 128 channels read through the x2 up-sampling, 256 direct: 12 K tiles).  S = 3 puts a
    slice boundary on the source boundary, S = 2 starts a slice inside src1, with S = 4 the second slice straddles the two sources."""
    from oracle import oracle as O
    S_img, B = 64, 2
    x = np.random.default_rng(3).random((B, S_img, S_img, 3), dtype=np.float32)
    cat = [(slot, o) for slot, o in enumerate(program.conv_ops()) if o.src1 >= 0 and o.cin == 384]
    assert len(cat) == 1 and cat[0][1].c0 == 128 and cat[0][1].src0_upsample
    slot, o = cat[0]
    _, kept = O.forward(program, weights, x, keep={o.dst})
    r = kept[o.dst]
    net = rt.Net(program)
    net.load_weights(weights)
    net.keep_activations(True)
    net.plan(B, S_img)
    for S in (1, 3, 2, 4):
        net.set_split_k(slot, S)        # on a planned net: decided again at once
        assert net.split_k(slot) == S and sum(net.split_k(i) > 1 for i in range(len(net.conv_ops))) == int(S > 1)
        net.forward(_cuda(x))
        g = net.read_tensor(o.dst, B).cpu().numpy()
        err = float(np.abs(g - r).max())
        print(f"concat 1x1 S={S}: max|diff| = {err:.3e}, bar {_bar(r):.3e}")
        assert err <= _bar(r), (S, err)
    with pytest.raises(rt.Y3Error, match="K tiles"):
        net.set_split_k(slot, 13)


def test_split_off_on_every_conv_gives_the_default_plans_bits(rt, program, weights):
    x = _cuda(np.random.default_rng(8).random((1, 64, 64, 3), dtype=np.float32))
    base = rt.Net(program)
    base.load_weights(weights)
    base.plan(1, 64)
    assert all(base.split_k(i) == 1 for i in range(len(base.conv_ops)))     # off by default
    want = [g.clone() for g in base.forward(x)]
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_low_latency(True)
    for i in range(len(net.conv_ops)):
        net.set_split_k(i, 1)
    net.plan(1, 64)
    assert all(net.split_k(i) == 1 for i in range(len(net.conv_ops)))
    got = net.forward(x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    # ... and handing the convs back to the heuristic splits some of them
    for i in range(len(net.conv_ops)):
        net.set_split_k(i, -1)
    assert any(net.split_k(i) > 1 for i in range(len(net.conv_ops)))
    net.set_low_latency(False)
    assert all(net.split_k(i) == 1 for i in range(len(net.conv_ops)))
    again = net.forward(x)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(want, again))


@pytest.mark.parametrize("size", [64, (64, 96)])
def test_low_latency_network(rt, program, weights, anchors, size):
    """The 75-conv network in a low-latency plan for one image: grids within 1e-4 of the oracle (the bar of test_network_grids_match_oracle),
    y3_net_detect bit-identical to the composed route, two runs bit-identical, and -- in a plan for two -- image 0 of a two-image call
    bit-identical to the same image alone."""
    from oracle import oracle as O
    H, W = rt.canvas_hw(size)
    x = np.random.default_rng(21).random((2, H, W, 3), dtype=np.float32)
    ref = O.forward(program, weights, x[:1])
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_low_latency(True)
    net.plan(1, size)
    splits = [net.split_k(i) for i in range(len(net.conv_ops))]
    print("split_k per conv:", splits)
    assert max(splits) > 1 and all(1 <= s <= 16 for s in splits)
    heads = [i for i, o in enumerate(net.conv_ops) if o.dst in program.outputs]
    assert len(heads) == 3 and all(splits[i] == 1 for i in heads) and splits[0] == splits[1] == splits[2] == 1
    x1 = _cuda(x[:1])
    grids = [g.clone() for g in net.forward(x1)]
    torch.cuda.synchronize()
    for r, g in zip(ref, grids):
        err = float(np.abs(g.cpu().numpy().reshape(r.shape) - r).max())
        print(f"low-latency grids {size}: max|diff| = {err:.3e}")
        assert err <= 1e-4
    again = net.forward(x1)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(grids, again))
    bb, cc, ss = rt.yolo_decode_scores(grids, anchors, 80)
    sel, nv = rt.nms_padded(bb, ss, 100, 0.5, 0.05)
    want = rt.pack_detections(bb, cc, ss, sel, nv)
    packed, nv2 = net.detect(x1, anchors, 100, 0.5, 0.05)
    torch.cuda.synchronize()
    assert torch.equal(nv2, nv) and torch.equal(packed, want)
    # a plan for two images: the bits of image 0 do not depend on the batch of the call
    net2 = rt.Net(program)
    net2.load_weights(weights)
    net2.set_low_latency(True)
    net2.plan(2, size)
    assert max(net2.split_k(i) for i in range(len(net2.conv_ops))) > 1
    both = [g.clone() for g in net2.forward(_cuda(x))]
    alone = net2.forward(x1)
    torch.cuda.synchronize()
    assert net2.max_batch == 2
    assert all(torch.equal(a[:1], b) for a, b in zip(both, alone))


def test_low_latency_detect_graph_capture(rt, program, weights, anchors):
    """The split launches and their finish launches enqueue work only: a one-image detect is captured and replayed three times."""
    x = _cuda(np.random.default_rng(31).random((1, 64, 64, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.set_low_latency(True)
    net.plan(1, 64)
    assert any(net.split_k(i) > 1 for i in range(len(net.conv_ops)))
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


def test_forced_splits_two_lanes_equal_one_lane(rt, program, weights):
    """Four images, every eligible conv forced to two slices: two concurrent lanes (each with its own slab workspace) give the bits of
    one lane."""
    x = _cuda(np.random.default_rng(41).random((4, 64, 64, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    forced = 0
    for i in range(len(net.conv_ops)):
        try:
            net.set_split_k(i, 2)
            forced += 1
        except rt.Y3Error:
            pass
    net.plan(4, 64)
    n_split = sum(net.split_k(i) == 2 for i in range(len(net.conv_ops)))
    print(f"forced {forced} convs, {n_split} split after planning")
    assert n_split >= 60
    net.set_lanes(1)
    one = [g.clone() for g in net.forward(x)]
    net.set_lanes(2)
    assert sum(net.split_k(i) == 2 for i in range(len(net.conv_ops))) == n_split
    for _ in range(2):
        two = net.forward(x)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(one, two))


def test_split_refusals(rt, program, weights):
    net = rt.Net(program)
    net.load_weights(weights)
    ops = net.conv_ops
    head = next(i for i, o in enumerate(ops) if o.dst in program.outputs)
    with pytest.raises(rt.Y3Error, match="head"):
        net.set_split_k(head, 2)
    with pytest.raises(rt.Y3Error, match="first layer"):
        net.set_split_k(0, 2)
    res = next(i for i, o in enumerate(ops) if o.size == 3 and o.stride == 1 and o.cin == 32)
    with pytest.raises(rt.Y3Error, match="tile"):
        net.set_split_k(res, 2)                       # the weight-resident tile 33
    small = next(i for i, o in enumerate(ops) if o.size == 1 and o.cin == 128 and o.cout == 64)
    with pytest.raises(rt.Y3Error, match="K tiles"):
        net.set_split_k(small, 8)                     # 4 K tiles
    net.set_split_k(small, 4)
    net.set_split_k(head, 1)                          # "off" is never refused
    net.set_split_k(head, -1)
    # a bf16 plan splits nothing and refuses a forced value
    net.set_low_latency(True)
    net.plan(1, 64, _lib.Y3_DTYPE_BF16)
    assert all(net.split_k(i) == 1 for i in range(len(ops)))
    with pytest.raises(rt.Y3Error, match="F32"):
        net.set_split_k(small, 2)
    # ... and the same net planned fp32 takes the forced value and the heuristic
    net.plan(1, 64, _lib.Y3_DTYPE_F32)
    assert net.split_k(small) == 4 and net.split_k(head) == 1 and net.split_k(0) == 1
    with pytest.raises(rt.Y3Error, match="fused stem"):
        net.set_split_k(1, 2)
