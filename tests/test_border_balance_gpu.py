"""Balanced tile -> XCD mapping of the border-skip launches (csrc/y3_kernels.h, balanced_tile): a batch-minor launch
deals its border tiles and its interior tiles evenly over the XCD pixel-tile ranges, so which workgroup computes a tile changes and nothing
of the tile does.  Every case asserts

  torch.equal between set_border_skip(1) and set_border_skip(0), under set_xcd_mode(0) and set_xcd_mode(1), and between the two modes,

into output grids filled with NaN before every forward and over intermediates overwritten by a forward of other data in between, so a tile
no workgroup computed cannot pass for one that was -- on the smallest shapes at which the mapping can go wrong: fewer interior tiles than
ranges, no interior at all, shares that do not divide by the ranges in the contiguous and in the blocked order, tiles of one, two, four and
eight positions and tiles that straddle positions, padding workgroups, two lanes, every epilogue form."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import _Graph, mini_program  # noqa: E402
from yolo_v3_tf2_amd import _lib  # noqa: E402

GENERIC_TILES = [t for t in range(len(_lib.TILES)) if t not in _lib.RETIRED_TILES and t != 33]
PLAIN = [dict(filters=128, bn=True, act="leaky"), dict(filters=128, bn=False, act="linear"), dict(filters=128, bn=True, act="linear")]


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _heads(cin, heads, seed):
    """Three 3x3 convs reading the input directly, each a launch that writes a caller-owned fp32 grid: (program, weights)."""
    from yolo_v3_tf2_amd.weights import synthetic_weights
    p = mini_program(cin, [], [dict(size=3, **h) for h in heads])
    return p, synthetic_weights(p, seed=seed)


def _force(rt, net, tile):
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


def _check(rt, p, w, x, canvas, lanes=1, tile=None, stored=()):
    """Skip on == skip off in both XCD modes, and the modes among themselves; `stored`: intermediate tensors to compare as well."""
    B = x.shape[0]
    net = rt.Net(p)
    net.load_weights(w)
    if tile is not None:
        assert _force(rt, net, tile) > 0, f"tile {tile} fits no 3x3 conv of the case"
    if stored:
        net.keep_activations(True)
    net.plan(B, canvas)
    net.set_lanes(lanes)
    xin = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    other = torch.flip(xin, dims=(0,)) * 0.5 + 1.0
    arms = {}
    for xcd in (0, 1):
        net.set_xcd_mode(xcd)
        for skip in (1, 0):
            net.set_border_skip(skip)
            for slot, o in enumerate(net.conv_ops):
                if o.size == 3:
                    assert net.border_skip(slot, B) == (lanes if skip else 0), (slot, skip)
            out = [torch.full_like(g, float("nan")) for g in net.forward(other)]      # other values into every intermediate
            net.forward(xin, out=out)
            arms[xcd, skip] = out + [net.read_tensor(t, B) for t in stored]
    torch.cuda.synchronize()
    ref = arms[0, 0]
    assert not any(bool(torch.isnan(t).any()) for t in ref)
    for key, got in arms.items():
        for k, (a, b) in enumerate(zip(got, ref)):
            assert torch.equal(a, b), f"xcd mode {key[0]}, skip {key[1]}, tensor {k}: differs from the raster launch in the contiguous order"


@pytest.fixture(scope="module")
def conv_5x5():
    p, w = _heads(64, PLAIN, seed=61)
    return p, w, np.random.default_rng(61).standard_normal((32, 5, 5, 64)).astype(np.float32)


@pytest.mark.parametrize("tile", [t for t in GENERIC_TILES if 128 % _lib.TILES[t][1] == 0], ids=lambda t: f"t{t}")
def test_5x5_grid_on_every_generic_tile(rt, conv_5x5, tile):
    """64 -> 128 at 5 x 5, 32 images: 16 border positions and 9 interior ones.  On 64-row tiles 13 tiles, Tb = 8, five interior tiles for
    eight ranges (three ranges hold a border tile alone); on 128- and 256-row tiles four and eight positions per tile, 7 and 4 tiles, fewer
    than ranges, and the tile at the class boundary holds both kinds."""
    p, w, x = conv_5x5
    _check(rt, p, w, x, 5, tile=tile)


@pytest.mark.parametrize("g", [1, 2, 3])
def test_small_grids_no_interior_or_one_interior_position(rt, g):
    """1 x 1 and 2 x 2: Tb = T, nothing interior (one and two tiles on eight ranges); 3 x 3: a single interior position, in a partial tile."""
    p, w = _heads(64, PLAIN, seed=62 + g)
    x = np.random.default_rng(62 + g).standard_normal((32, g, g, 64)).astype(np.float32)
    _check(rt, p, w, x, g)
    _check(rt, p, w, x, g, tile=26)


def test_6x6_blocked_order(rt):
    """256 -> 512 at 6 x 6 on tile 10 (64 x 128): 18 x 4 = 72 workgroups, so set_xcd_mode(1) takes the XCD-blocked order (choose_xcd_gn: the
    4.7 MB of weights must be cut, and with 1.2 MB of activations its cost formula cuts them four ways: two M-ranges) with Tb = 10, Ti = 8;
    set_xcd_mode(0) runs the same launch on eight ranges, where neither divides."""
    p, w = _heads(256, [dict(h, filters=512) for h in PLAIN], seed=66)
    x = np.random.default_rng(66).standard_normal((32, 6, 6, 256)).astype(np.float32)
    _check(rt, p, w, x, 6, tile=10)


def test_8x8_blocked_order_four_ranges(rt):
    """256 -> 256 at 8 x 8 on tile 10: 32 x 2 = 64 workgroups, 2.4 MB of weights against 2.1 MB of activations -- choose_xcd_gn cuts the
    weights in two (gn = 2), the four M-ranges of the headline's 26 x 26 launches, with Tb = 14 and Ti = 18, neither divisible by 4:
    ranges of 3 + 4, 4 + 5, 3 + 4, 4 + 5 tiles and padding workgroups in two of them."""
    p, w = _heads(256, [dict(h, filters=256) for h in PLAIN], seed=67)
    x = np.random.default_rng(67).standard_normal((32, 8, 8, 256)).astype(np.float32)
    _check(rt, p, w, x, 8, tile=10)


def test_rectangular_grid(rt):
    p, w = _heads(64, PLAIN, seed=68)
    x = np.random.default_rng(68).standard_normal((32, 5, 7, 64)).astype(np.float32)
    _check(rt, p, w, x, (5, 7))


def test_stride_2(rt):
    """8 x 8 -> 4 x 4: only the top row and the left column lose taps (7 border positions of 16)."""
    p, w = _heads(64, [dict(stride=2, **h) for h in PLAIN], seed=69)
    x = np.random.default_rng(69).standard_normal((32, 8, 8, 64)).astype(np.float32)
    _check(rt, p, w, x, 8)


@pytest.mark.parametrize("B,lanes", [(64, 1), (96, 1), (64, 2)], ids=["64x1", "96x1", "64x2"])
def test_lane_batches(rt, B, lanes):
    """64 images in one lane: a 64-row tile is one position, Tb = 16 of 25; 96: a position is a tile and a half, tiles straddle positions (Tb = 16 * 96 / 64 = 24 of
    38); 64 on two lanes: two launches of 32 side by side."""
    p, w = _heads(64, PLAIN, seed=70)
    x = np.random.default_rng(70 + B).standard_normal((B, 5, 5, 64)).astype(np.float32)
    _check(rt, p, w, x, 5, lanes=lanes)


def test_shortcut_and_linear_epilogues(rt):
    """leaky and linear, each with and without a shortcut, and a Cout short of the launch's padded width."""
    from yolo_v3_tf2_amd.weights import synthetic_weights
    g = _Graph(64)
    a = g.conv(g.input, 128, 3)                                  # leaky
    c = g.shortcut(g.conv(a, 128, 3, act="linear"), a)           # linear + shortcut
    d = g.shortcut(g.conv(c, 128, 3), c)                         # leaky + shortcut
    h0 = g.conv(d, 96, 3, bn=False, act="linear", sub="head")    # linear, bias
    h1 = g.conv(d, 100, 3, sub="head")
    h2 = g.conv(d, 128, 3, act="linear", sub="head")
    p = g.program([h0, h1, h2])
    ops = list(p.conv_ops())
    assert [o.residual >= 0 for o in ops] == [False, True, True, False, False, False] and [o.leaky for o in ops] == [1, 0, 1, 0, 1, 0]
    x = np.random.default_rng(71).standard_normal((32, 5, 5, 64)).astype(np.float32)
    _check(rt, p, synthetic_weights(p, seed=71), x, 5, stored=[o.dst for o in ops if o.dst not in p.outputs])
