"""Border skip of the fp32 3x3 convs (y3_net_set_border_skip): batch-minor GEMM rows over the sorted position table,
every workgroup leaving out the taps that are padding for all of its positions.  Only products with zero are left out, so every case asserts

  torch.equal between set_border_skip(1) and set_border_skip(0) on the same net, inputs and tiles, and
  the project's per-layer bar against the oracle for the skipping arm: |got - ref| <= 2e-5 * max(1, |ref|max) per launch

on the smallest shapes at which the kernel can go wrong: a 5 x 5 grid (every mask class and an interior) on every built generic tile, grids
whose first live tap is not tap 0 / with one live tap / ending in a partial tile, the chunk-major K order, stride 2, a rectangular grid, every
epilogue form, lane batches that are and are not multiples of 32, and the whole YOLOv3 program at a 64 x 64 canvas, eager and captured."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import _Graph, mini_program, oracle_launch  # noqa: E402
from yolo_v3_tf2_amd import _lib  # noqa: E402

RULE_DEFAULT = 1      # set_border_skip(-1), the library's rule: on for every eligible conv (profiles/border_skip_ab.txt)
GENERIC_TILES = [t for t in range(len(_lib.TILES)) if t not in _lib.RETIRED_TILES and t != 33]


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bar(got, ref, what):
    err, bar = float(np.abs(got - ref).max()), 2e-5 * max(1.0, float(np.abs(ref).max()))
    print(f"border-skip {what}: worst {err / bar:.3f} of the bar")
    assert got.shape == ref.shape and err <= bar, (what, err, bar)


def _heads(cin, heads, seed):
    """Three 3x3 convs reading the input directly, each a launch that writes a caller-owned fp32 grid: (program, weights)."""
    from yolo_v3_tf2_amd.weights import synthetic_weights
    p = mini_program(cin, [], [dict(size=3, **h) for h in heads])
    return p, synthetic_weights(p, seed=seed)


def _force(rt, net, tile):
    """The tile on every 3x3 conv it fits -> how many took it."""
    n = 0
    for slot, o in enumerate(net.conv_ops):
        if o.size != 3:
            continue
        try:
            net.set_tile(slot, tile)
            n += 1
        except rt.Y3Error as e:
            if "tile does not" not in str(e):
                raise
    return n


def _both_arms(rt, p, w, x, canvas, lanes=1, tile=None, taken=None):
    """The three grids of a forward with the skip on and off (same net, plan, tiles, input); `taken`: in how many lanes each 3x3 conv must
    take the skipping launch with the switch on (default: every lane) -- and none with it off."""
    B = x.shape[0]
    net = rt.Net(p)
    net.load_weights(w)
    if tile is not None:
        assert _force(rt, net, tile) > 0, f"tile {tile} fits no 3x3 conv of the case"
    net.plan(B, canvas)
    net.set_lanes(lanes)
    xin = _cuda(x)
    arms = {}
    for mode in (1, 0):
        net.set_border_skip(mode)
        for slot, o in enumerate(net.conv_ops):
            if o.size == 3:
                assert net.border_skip(slot, B) == ((lanes if taken is None else taken) if mode else 0), (slot, mode)
        arms[mode] = [g.clone() for g in net.forward(xin)]
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(arms[1], arms[0])):
        assert torch.equal(a, b), f"output {k}: the skipping launch and the raster launch differ"
    return arms[1]


def _check_heads(rt, p, w, x, canvas, what, **kw):
    from oracle import oracle as O
    got = _both_arms(rt, p, w, x, canvas, **kw)
    for k, (g, r) in enumerate(zip(got, O.forward(p, w, x))):
        _bar(g.cpu().numpy().reshape(r.shape), r, f"{what} head {k}")


PLAIN = [dict(filters=128, bn=True, act="leaky"), dict(filters=128, bn=False, act="linear"), dict(filters=128, bn=True, act="linear")]


@pytest.fixture(scope="module")
def conv_5x5():
    p, w = _heads(64, PLAIN, seed=11)
    return p, w, np.random.default_rng(11).standard_normal((32, 5, 5, 64)).astype(np.float32)


@pytest.mark.parametrize("tile", [t for t in GENERIC_TILES if 128 % _lib.TILES[t][1] == 0], ids=lambda t: f"t{t}")
def test_5x5_grid_on_every_generic_tile(rt, conv_5x5, tile):
    """64 -> 128 at 5 x 5, 32 images (M = 800: a partial last tile for every BM): register-staged 64-, 128- and 256-row tiles on four and
    eight waves, LDS-DMA with one and two stages."""
    p, w, x = conv_5x5
    _check_heads(rt, p, w, x, 5, f"5x5 tile {tile}", tile=tile)


@pytest.mark.parametrize("g", [1, 2, 3])
def test_small_grids_first_live_tap_single_tap_partial_tile(rt, g):
    """1 x 1: the centre tap alone is live (the walk starts at tap 4 and has one tap); 2 x 2: every tile starts at tap 4 or later;
    3 x 3: M = 288 ends in a partial tile."""
    p, w = _heads(64, PLAIN, seed=20 + g)
    x = np.random.default_rng(20 + g).standard_normal((32, g, g, 64)).astype(np.float32)
    _check_heads(rt, p, w, x, g, f"{g}x{g}")
    _check_heads(rt, p, w, x, g, f"{g}x{g} tile 26", tile=26)


@pytest.mark.parametrize("cin", [256, 512])
def test_chunk_major_k_order(rt, cin):
    """Cin 256 and 512 with the default k_chunk (128 channels per chunk): the live taps of every channel chunk."""
    p, w = _heads(cin, PLAIN, seed=cin)
    x = np.random.default_rng(cin).standard_normal((32, 4, 4, cin)).astype(np.float32)
    _check_heads(rt, p, w, x, 4, f"4x4 cin {cin}")
    _check_heads(rt, p, w, x, 4, f"4x4 cin {cin} tile 31", tile=31)


def test_stride_2(rt):
    p, w = _heads(64, [dict(stride=2, **h) for h in PLAIN], seed=31)
    x = np.random.default_rng(31).standard_normal((32, 8, 8, 64)).astype(np.float32)
    _check_heads(rt, p, w, x, 8, "8x8 -> 4x4 stride 2")


def test_rectangular_grid(rt):
    p, w = _heads(64, PLAIN, seed=32)
    x = np.random.default_rng(32).standard_normal((32, 3, 7, 64)).astype(np.float32)
    _check_heads(rt, p, w, x, (3, 7), "3x7")


def test_every_epilogue_form(rt):
    """leaky and linear, each with and without a shortcut (teacher-forced on the launch's own device inputs), and a Cout short of the
    launch's padded width: 96 in the 32-wide tile's 96 and 100 in 128 (channels >= Cout inside the tile)."""
    from oracle import oracle as O
    from yolo_v3_tf2_amd.weights import synthetic_weights
    g = _Graph(64)
    a = g.conv(g.input, 128, 3)                                  # leaky
    c = g.shortcut(g.conv(a, 128, 3, act="linear"), a)           # linear + shortcut
    d = g.shortcut(g.conv(c, 128, 3), c)                         # leaky + shortcut
    h0 = g.conv(d, 96, 3, bn=False, act="linear", sub="head")    # linear, bias
    h1 = g.conv(d, 100, 3, sub="head")
    h2 = g.conv(d, 128, 3, act="linear", sub="head")
    p = g.program([h0, h1, h2])
    w = synthetic_weights(p, seed=33)
    x = np.random.default_rng(33).standard_normal((32, 5, 5, 64)).astype(np.float32)
    B = 32
    net = rt.Net(p)
    net.load_weights(w)
    net.keep_activations(True)
    net.plan(B, 5)
    stored = [o.dst for o in p.conv_ops() if o.dst not in p.outputs]
    arms = {}
    for mode in (1, 0):
        net.set_border_skip(mode)
        assert all(net.border_skip(s, B) == mode for s in range(len(net.conv_ops)))
        grids = net.forward(_cuda(x))
        arms[mode] = [t.clone() for t in grids] + [net.read_tensor(t, B).clone() for t in stored]
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(arms[1], arms[0]))
    dev = {t: v.cpu().numpy().reshape(B, 5, 5, -1) for t, v in zip(list(p.outputs) + stored, arms[1])}
    dev[p.input_tensor] = x
    ops = list(p.conv_ops())
    assert [o.residual >= 0 for o in ops] == [False, True, True, False, False, False] and [o.leaky for o in ops] == [1, 0, 1, 0, 1, 0]
    for k, o in enumerate(ops):
        _bar(dev[o.dst], oracle_launch(O, o, w, dev.__getitem__), f"epilogue forms conv {k}")


@pytest.mark.parametrize("B,lanes,taken", [(64, 1, 1), (96, 1, 1), (64, 2, 2), (48, 2, 0), (33, 1, 0)],
                         ids=["64x1", "96x1", "64x2", "48x2-raster", "33x1-raster"])
def test_lane_batches(rt, B, lanes, taken):
    """64 and 96 images in one lane (two and three 32-image blocks per position), 64 on two lanes; 48 on two lanes (24 each) and 33 in
    one are not whole blocks: the switch must leave them the raster launch."""
    p, w = _heads(64, PLAIN, seed=40)
    x = np.random.default_rng(40 + B).standard_normal((B, 5, 5, 64)).astype(np.float32)
    _check_heads(rt, p, w, x, 5, f"5x5 {B} images {lanes} lanes", lanes=lanes, taken=taken)


def test_switch_arguments_and_other_plans(rt):
    """A bad mode is refused by name; before a plan, and on a plan that is not fp32, no conv takes the skipping launch."""
    p, w = _heads(64, PLAIN, seed=41)
    net = rt.Net(p)
    with pytest.raises(rt.Y3Error, match="y3_net_set_border_skip"):
        net.set_border_skip(2)
    net.set_border_skip(1)
    assert net.border_skip(0, 32) == 0
    net.load_weights(w)
    net.plan(32, 5, _lib.Y3_DTYPE_BF16)
    assert [net.border_skip(s, 32) for s in range(3)] == [0, 0, 0]
    net.plan(32, 5, _lib.Y3_DTYPE_F32)
    assert [net.border_skip(s, 32) for s in range(3)] == [1, 1, 1]
    net.set_border_skip(-1)
    assert [net.border_skip(s, 32) for s in range(3)] == [RULE_DEFAULT] * 3


@pytest.fixture(scope="module")
def yolo_64(rt, program, weights):
    """The whole YOLOv3 program at a 64 x 64 canvas (grids 2 / 4 / 8), 64 images on two lanes, skip on and off."""
    x = _cuda(np.random.default_rng(50).random((64, 64, 64, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(64, 64)
    net.set_lanes(2)
    net.set_border_skip(1)
    n_taken = sum(net.border_skip(s, 64) == 2 for s in range(len(net.conv_ops)))
    assert n_taken >= 20, n_taken      # the stride-1 3x3 convs of the residual blocks and the necks, the stride-2 convs
    return net, x


def test_yolov3_64_forward_and_decode_routes(rt, yolo_64, program, weights, anchors):
    from oracle import oracle as O
    net, x = yolo_64
    out = {}
    for mode in (1, 0):
        net.set_border_skip(mode)
        grids = [g.clone() for g in net.forward(x)]
        out[mode] = grids + list(rt.yolo_decode_scores(grids, anchors, 80)) + list(net.forward_decode(x, anchors))
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(out[1], out[0]))
    assert all(torch.equal(u, v) for u, v in zip(out[1][3:6], out[1][6:9])), "forward_decode differs from forward + yolo_decode_scores"
    # the batch contract: image 5 alone (one image: the raster launch) has the bits of image 5 of the batch
    net.set_border_skip(1)
    alone = net.forward(x[5:6].contiguous())
    torch.cuda.synchronize()
    for a, g in zip(alone, out[1][:3]):
        assert torch.equal(a[0], g[5])
    for r, g in zip(O.forward(program, weights, x[5:6].cpu().numpy()), out[1][:3]):
        assert np.abs(g[5:6].cpu().numpy() - r).max() <= 1e-4      # the network bar of tests/test_gpu_parity.py


def test_yolov3_64_captured_graph_replay(rt, yolo_64):
    net, x = yolo_64
    net.set_border_skip(1)
    ref = [g.clone() for g in net.forward(x)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        net.forward(x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = net.forward(x)
    for t in out:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(out, ref))
