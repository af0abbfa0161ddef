"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle on the same seeded
inputs.  Tolerances are stated per test; integer/index outputs must match bit for bit.

Oracle status: PARITY UNPINNED (TensorFlow absent, reference ships no golden outputs) -- see
oracle/y3_oracle.c and DESIGN.md.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from yolo_v3_tf2_amd import _lib  # noqa: E402  (tile tables for the parametrised tile tests)
from tests.helpers import NETWORK_GRID_BAR, bf16_tile_bar, check_f32_conv  # noqa: E402  (the bars tests/test_class_counts_gpu.py shares)


@pytest.fixture(scope="module")
def rt():
    from yolo_v3_tf2_amd import runtime
    from yolo_v3_tf2_amd._lib import require_gpu
    require_gpu()  # fail loudly, never fall back
    return runtime


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _boxes_close(got, ref):
    """north_star's 1e-4 on box coordinates: strictly absolute wherever |coord| <= 1 (where detections live), relative
    to |coord| for the unclipped random-init boxes many image widths wide (w = exp(tw) * anchor turns a 1e-5
    summation-order difference in tw into 1e-5 * w).  tests/test_oracle.py::
    test_two_cpu_fp32_implementations_bound_the_box_bar shows two CPU fp32 implementations already miss an absolute
    1e-4 on those wide boxes (5e-4 on girl.png) while meeting both parts of this bar."""
    err = np.abs(got - ref)
    unit = np.abs(ref) <= 1.0
    strict = (not unit.any()) or float(err[unit].max()) <= 1e-4
    return strict and float((err / np.maximum(1.0, np.abs(ref))).max()) <= 1e-4


def _selection_explained(ref5, dev5, iou=0.5, score=0.1):
    """End-to-end selections equal, or every difference attributed to a near-tie (oracle/flip_attribution.py) whose
    margin the measured box / score deviation covers.  Returns the flips (reported by the caller, never hidden)."""
    from oracle import flip_attribution as FA
    rb, _, rs, rsel, rnv = ref5
    gb, _, gs, gsel, gnv = dev5
    flips = FA.attribute(rb, rs, rsel, rnv, gb, gs, gsel, gnv, iou, score)
    err = np.abs(gb - rb)
    unit = np.abs(rb) <= 1.0
    dbox = float(err[unit].max()) if unit.any() else 0.0
    assert FA.explained(flips, float(np.abs(gs - rs).max()), dbox), f"selection differs without a near-tie: {flips}"
    if flips:
        print("selection flips (near-ties):", flips)
    return flips


# ---------------------------------------------------------------------------------------------- conv
CONV_CASES = [
    # (in_ch, S, B, chain, heads)  -- heads are three raw outputs exercising different tiles/shapes
    (32, 32, 2, [], [dict(filters=64, size=3, stride=2), dict(filters=64, size=3), dict(filters=32, size=1)]),
    (64, 16, 3, [], [dict(filters=128, size=3, stride=2), dict(filters=128, size=3), dict(filters=255, size=1, bn=False, act="linear")]),
    (128, 13, 2, [dict(filters=64, size=1), dict(filters=128, size=3, shortcut=-3)],
     [dict(filters=256, size=3), dict(filters=256, size=3, stride=1), dict(filters=64, size=1)]),
    (256, 26, 1, [], [dict(filters=512, size=3), dict(filters=128, size=1), dict(filters=255, size=1, bn=False, act="linear")]),
    (3, 32, 2, [dict(filters=32, size=3)], [dict(filters=64, size=3, stride=2), dict(filters=32, size=1), dict(filters=64, size=3)]),
]


@pytest.mark.parametrize("case", range(len(CONV_CASES)))
def test_conv_layers_match_oracle(rt, case):
    """Single fused conv launches (3x3/1, 3x3/2, 1x1, bias head, residual, first layer) vs the oracle.
    Tolerance: |diff| <= 2e-5 * max(1, |ref|max) -- fp32 with a different summation order over K <= 4608."""
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from oracle import oracle as O
    in_ch, S, B, chain, heads = CONV_CASES[case]
    # stride-2 heads need an even input; image_size must be divisible by every tensor's divisor
    p = mini_program(in_ch, chain, heads)
    w = synthetic_weights(p, seed=100 + case)
    rng = np.random.default_rng(case)
    x = (rng.standard_normal((B, S, S, in_ch)) if in_ch != 3 else rng.random((B, S, S, in_ch))).astype(np.float32)
    ref = O.forward(p, w, x)
    net = rt.Net(p)
    net.load_weights(w)
    net.plan(B, S)
    got = net.forward(_cuda(x))
    torch.cuda.synchronize()
    for r, g in zip(ref, got):
        check_f32_conv(g.cpu().numpy().reshape(r.shape), r, case)


def _real_tiles():
    from yolo_v3_tf2_amd._lib import TILES, RETIRED_TILES
    return [t for t in range(len(TILES)) if t not in RETIRED_TILES and t != 33]   # 33: the weight-resident kernel (Cin = 32 only), tested on its own


@pytest.mark.parametrize("tile", _real_tiles())
def test_conv_every_tile_shape(rt, tile):
    """Force each block tile of the MFMA kernel on a shape with ragged M (M % BM != 0)."""
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from yolo_v3_tf2_amd._lib import TILES
    from oracle import oracle as O
    cout = TILES[tile][1]
    p = mini_program(64, [], [dict(filters=cout, size=3), dict(filters=cout, size=1), dict(filters=cout, size=3, stride=2)])
    w = synthetic_weights(p, seed=7)
    x = np.random.default_rng(7).standard_normal((3, 14, 14, 64)).astype(np.float32)  # M = 588, 147
    ref = O.forward(p, w, x)
    net = rt.Net(p)
    net.load_weights(w)
    for slot in range(3):
        net.set_tile(slot, tile)
    net.plan(3, 14)
    got = net.forward(_cuda(x))
    torch.cuda.synchronize()
    for r, g in zip(ref, got):
        g = g.cpu().numpy().reshape(r.shape)
        assert np.abs(g - r).max() <= 2e-5 * max(1.0, float(np.abs(r).max()))


@pytest.mark.parametrize("cout,S,B", [(64, 48, 3), (128, 41, 2), (64, 208, 1)])
def test_f32_weight_resident_conv_bit_identical_to_generic_tiles(rt, cout, S, B):
    """fp32 tile id 33 (csrc/conv_res_f32.hip): the 3x3 / stride-1 / 32-input-channel conv with its weights resident in registers and
    its input patch (8 x 16-pixel tiles) fetched by LDS-DMA.  Same k order and lane grouping as conv_f32_mfma, so: BIT-IDENTICAL to
    the generic 64x64 tile, with and without a shortcut, leaky and linear, on sizes that are not multiples of the tile (41: ragged
    last row and column of tiles), over several images, and at the network's own 208 x 208; against the oracle within the layer bar."""
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from oracle import oracle as O
    chain = [dict(filters=cout, size=3), dict(filters=32, size=1), dict(filters=cout, size=3, shortcut=-3),
             dict(filters=32, size=1, act="linear"), dict(filters=cout, size=3, bn=False, act="linear"), dict(filters=32, size=1)]
    heads = [dict(filters=64, size=3), dict(filters=128, size=3), dict(filters=64, size=3, bn=False, act="linear")]
    p = mini_program(32, chain, heads)
    w = synthetic_weights(p, seed=61)
    x = np.random.default_rng(61).standard_normal((B, S, S, 32)).astype(np.float32)
    ref = O.forward(p, w, x)
    outs = {}
    for name, tile in (("resident", 33), ("generic", 11)):
        net = rt.Net(p)
        net.load_weights(w)
        forced = 0
        for slot, o in enumerate(net.conv_ops):
            if o.size == 3:
                net.set_tile(slot, tile)
                forced += 1
        assert forced == 6
        net.plan(B, S)
        outs[name] = [g.clone() for g in net.forward(_cuda(x))]
        again = net.forward(_cuda(x))
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs[name], again))
    for a, b, r in zip(outs["resident"], outs["generic"], ref):
        assert torch.equal(a, b)
        assert np.abs(a.cpu().numpy().reshape(r.shape) - r).max() <= 2e-5 * max(1.0, float(np.abs(r).max()))
    with pytest.raises(rt.Y3Error):
        net.set_tile(1, 33)     # the 1x1 conv: tile 33 is for 3x3 / stride-1 / Cin = 32 convs only


def test_xcd_blocked_tile_order_is_bit_identical(rt):
    """Placement of the fp32 conv tiles on the 8 XCDs (y3_net_set_xcd_mode): the weight-heavy 3x3 convs take the
    XCD-blocked order (512->1024: 18.9 MB of weights -> every XCD one eighth of the channel tiles; 256->512 with 64x128
    tiles: a 4 x 2 grid whose M split is uneven, so padding workgroups exit).  Same per-tile arithmetic: results equal
    the contiguous order bit for bit, and the oracle within the layer bar."""
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from oracle import oracle as O
    cases = [(512, 13, 8, dict(filters=1024, size=3), 11),      # 22 x 16 tiles of 64x64, gn = 8
             (256, 26, 2, dict(filters=512, size=3), 10),       # 22 x 4 tiles of 64x128, gn = 2 (M blocks 5/6/5/6)
             (128, 52, 2, dict(filters=256, size=3, stride=2), 10)]   # light weights: stays on the contiguous order
    for cin, S, B, head, tile in cases:
        p = mini_program(cin, [], [head, dict(filters=64, size=1), dict(filters=64, size=1)])
        w = synthetic_weights(p, seed=5)
        x = np.random.default_rng(5).standard_normal((B, S, S, cin)).astype(np.float32)
        ref = O.forward(p, w, x)[0]
        outs = []
        for mode in (0, 1):
            net = rt.Net(p)
            net.load_weights(w)
            net.set_xcd_mode(mode)
            net.set_tile(0, tile)
            net.plan(B, S)
            outs.append(net.forward(_cuda(x))[0])
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]), (cin, S)
        g = outs[1].cpu().numpy().reshape(ref.shape)
        assert np.abs(g - ref).max() <= 2e-5 * max(1.0, float(np.abs(ref).max())), (cin, S)


def test_upsample_concat_fused_conv(rt, program, weights):
    """neck1/neck2 lateral path: 1x1 conv reading nearest-upsampled src0 and src1 in place."""
    from oracle import oracle as O
    S, B = 64, 2
    x = np.random.default_rng(3).random((B, S, S, 3), dtype=np.float32)
    cat_convs = [o for o in program.conv_ops() if o.src1 >= 0]
    assert len(cat_convs) == 2 and all(o.src0_upsample for o in cat_convs)
    keep = {o.dst for o in cat_convs}
    _, kept = O.forward(program, weights, x, keep=keep)
    net = rt.Net(program)
    net.load_weights(weights)
    net.keep_activations(True)
    net.plan(B, S)
    net.forward(_cuda(x))
    for o in cat_convs:
        g = net.read_tensor(o.dst, B).cpu().numpy()
        r = kept[o.dst]
        assert np.abs(g - r).max() <= 2e-5 * max(1.0, float(np.abs(r).max()))


# ---------------------------------------------------------------------------------------------- f32x3
# fp32-accurate arithmetic on the bf16 matrix cores (three bf16 planes per value): held to the fp32 path's tolerances
# against the fp32 oracle.
@pytest.mark.parametrize("case", range(len(CONV_CASES)))
def test_x3_conv_layers_match_fp32_oracle(rt, case):
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from yolo_v3_tf2_amd import _lib
    from oracle import oracle as O
    in_ch, S, B, chain, heads = CONV_CASES[case]
    p = mini_program(in_ch, chain, heads)
    w = synthetic_weights(p, seed=100 + case)
    rng = np.random.default_rng(case)
    x = (rng.standard_normal((B, S, S, in_ch)) if in_ch != 3 else rng.random((B, S, S, in_ch))).astype(np.float32)
    ref = O.forward(p, w, x)
    net = rt.Net(p)
    net.load_weights(w)
    net.plan(B, S, _lib.Y3_DTYPE_F32X3)
    xin = _cuda(x) if in_ch == 3 else rt.split3_planes(_cuda(x))
    got = net.forward(xin)
    torch.cuda.synchronize()
    for r, g in zip(ref, got):
        check_f32_conv(g.cpu().numpy().reshape(r.shape), r, case)


@pytest.mark.parametrize("tile", _lib.TILES_X3_BUILT)
def test_x3_every_tile(rt, tile):
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from yolo_v3_tf2_amd import _lib
    from oracle import oracle as O
    bm, bn, _, bk = _lib.TILES_X3[tile]
    p = mini_program(64, [], [dict(filters=bn, size=3), dict(filters=bn, size=1), dict(filters=bn, size=3, stride=2)])
    w = synthetic_weights(p, seed=9)
    x = np.random.default_rng(9).standard_normal((3, 14, 14, 64)).astype(np.float32)
    ref = O.forward(p, w, x)
    net = rt.Net(p)
    net.load_weights(w)
    for slot in range(3):
        net.set_tile_x3(slot, tile)
    net.plan(3, 14, _lib.Y3_DTYPE_F32X3)
    got = net.forward(rt.split3_planes(_cuda(x)))
    torch.cuda.synchronize()
    for r, g in zip(ref, got):
        assert np.abs(g.cpu().numpy().reshape(r.shape) - r).max() <= 2e-5 * max(1.0, float(np.abs(r).max()))


@pytest.mark.parametrize("S,B", [(96, 2), (160, 1)])
def test_x3_network_and_detect_match_fp32_oracle(rt, program, weights, anchors, S, B):
    """Full network + decode + NMS in the three-plane mode: head logits within 1e-4 of the fp32 oracle (the fp32 path's
    bar), boxes/scores within 1e-4, NMS bit-exact on the device's own boxes/scores; fused upsample+concat convs and
    residual tensors checked as fp32 reconstructions."""
    from yolo_v3_tf2_amd import _lib
    from oracle import oracle as O
    x = np.random.default_rng(1234).random((B, S, S, 3), dtype=np.float32)
    ops = program.conv_ops()
    probe = [ops[3].dst, ops[25].dst] + [o.dst for o in ops if o.src1 >= 0]
    ref, kept = O.forward(program, weights, x, keep=set(probe))
    net = rt.Net(program)
    net.load_weights(weights)
    net.keep_activations(True)
    net.plan(B, S, _lib.Y3_DTYPE_F32X3)
    got = net.forward(_cuda(x))
    torch.cuda.synchronize()
    for r, g in zip(ref, got):
        assert np.abs(g.cpu().numpy() - r).max() <= 1e-4
    for t in probe:
        g = net.read_tensor(t, B).cpu().numpy()
        assert np.abs(g - kept[t]).max() <= 2e-5 * max(1.0, float(np.abs(kept[t]).max()))
    gb, gc, gs = rt.yolo_decode_scores(got, anchors, 80)
    gsel, gnv = rt.nms_padded(gb, gs, 100, 0.5, 0.1)
    rb, rc, rs, rsel, rnv = O.yolo_nms(O.yolo_decode(ref, anchors, 80), 100, 0.5, 0.1)
    assert np.abs(gb.cpu().numpy() - rb).max() <= 1e-4 and np.abs(gs.cpu().numpy() - rs).max() <= 1e-4
    s2, n2 = O.nms_padded(gb.cpu().numpy(), gs.cpu().numpy(), 100, 0.5, 0.1)
    assert np.array_equal(s2, gsel.cpu().numpy()) and np.array_equal(n2, gnv.cpu().numpy())


# ---------------------------------------------------------------------------------------------- f32x2
# Two fp16 planes per value (x = h + l' * 2^-11), three fp16 MFMAs per product: representation error 2^-22 (fp32: 2^-24).
# Held to the same tolerances as the fp32 and three-plane paths against the fp32 oracle.
@pytest.mark.parametrize("case", range(len(CONV_CASES)))
def test_x2_conv_layers_match_fp32_oracle(rt, case):
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from yolo_v3_tf2_amd import _lib
    from oracle import oracle as O
    in_ch, S, B, chain, heads = CONV_CASES[case]
    p = mini_program(in_ch, chain, heads)
    w = synthetic_weights(p, seed=100 + case)
    rng = np.random.default_rng(case)
    x = (rng.standard_normal((B, S, S, in_ch)) if in_ch != 3 else rng.random((B, S, S, in_ch))).astype(np.float32)
    ref = O.forward(p, w, x)
    net = rt.Net(p)
    net.load_weights(w)
    net.plan(B, S, _lib.Y3_DTYPE_F32X2)
    xin = _cuda(x) if in_ch == 3 else rt.split2_planes(_cuda(x))
    got = net.forward(xin)
    torch.cuda.synchronize()
    for r, g in zip(ref, got):
        check_f32_conv(g.cpu().numpy().reshape(r.shape), r, case)


def test_x2_split_is_accurate_to_2_pow_minus_22(rt):
    x = torch.randn(4096, device="cuda") * torch.logspace(-6, 3, 4096, device="cuda")
    pl = rt.split2_planes(x[None, :]).float()
    back = pl[0, 0] + pl[0, 1] / 2048.0
    big = x.abs() > 2.0 ** -13
    assert ((back - x).abs()[big] <= 2.0 ** -22 * x.abs()[big]).all()
    assert ((back - x).abs()[~big] <= 2.0 ** -36).all()      # lo plane subnormal: absolute error <= 2^-25 * 2^-11


def test_x2_rejects_weights_outside_fp16_range_only_in_that_mode(rt):
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from yolo_v3_tf2_amd import _lib
    p = mini_program(64, [], [dict(filters=64, size=1), dict(filters=64, size=1), dict(filters=64, size=1)])
    w = synthetic_weights(p, seed=1)
    k = next(k for k in w if k.endswith(".w"))
    w[k] = w[k].copy()
    w[k].flat[0] = 1.0e6          # far outside fp16 after any BN scale
    net = rt.Net(p)
    net.load_weights(w)           # loading succeeds: the other modes can use these weights
    net.plan(1, 8, _lib.Y3_DTYPE_F32)
    net.forward(_cuda(np.zeros((1, 8, 8, 64), np.float32)))
    with pytest.raises(rt.Y3Error, match="fp16 range"):
        net.plan(1, 8, _lib.Y3_DTYPE_F32X2)


@pytest.mark.parametrize("tile", _lib.TILES_X2_BUILT)
def test_x2_every_tile(rt, tile):
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from yolo_v3_tf2_amd import _lib
    from oracle import oracle as O
    assert tile in _lib.TILES_X2_BUILT
    bm, bn, _, bk = _lib.TILES_X3[tile]
    p = mini_program(64, [], [dict(filters=bn, size=3), dict(filters=bn, size=1), dict(filters=bn, size=3, stride=2)])
    w = synthetic_weights(p, seed=9)
    x = np.random.default_rng(9).standard_normal((3, 14, 14, 64)).astype(np.float32)
    ref = O.forward(p, w, x)
    net = rt.Net(p)
    net.load_weights(w)
    for slot in range(3):
        net.set_tile_x2(slot, tile)
    net.plan(3, 14, _lib.Y3_DTYPE_F32X2)
    got = net.forward(rt.split2_planes(_cuda(x)))
    torch.cuda.synchronize()
    for r, g in zip(ref, got):
        assert np.abs(g.cpu().numpy().reshape(r.shape) - r).max() <= 2e-5 * max(1.0, float(np.abs(r).max()))
    with pytest.raises(rt.Y3Error):
        net.set_tile_x2(0, 5)          # a tile id of the shared table that is not built for two planes


@pytest.mark.parametrize("S,B", [(96, 2), (160, 1)])
def test_x2_network_and_detect_match_fp32_oracle(rt, program, weights, anchors, S, B):
    """Full network + decode + NMS in the two-plane mode, same bar as the three-plane mode: head logits, boxes and scores
    within 1e-4 of the fp32 oracle, NMS bit-exact on the device's own boxes/scores."""
    from yolo_v3_tf2_amd import _lib
    from oracle import oracle as O
    x = np.random.default_rng(1234).random((B, S, S, 3), dtype=np.float32)
    ops = program.conv_ops()
    probe = [ops[3].dst, ops[25].dst] + [o.dst for o in ops if o.src1 >= 0]
    ref, kept = O.forward(program, weights, x, keep=set(probe))
    net = rt.Net(program)
    net.load_weights(weights)
    net.keep_activations(True)
    net.plan(B, S, _lib.Y3_DTYPE_F32X2)
    got = net.forward(_cuda(x))
    torch.cuda.synchronize()
    for r, g in zip(ref, got):
        assert np.abs(g.cpu().numpy() - r).max() <= 1e-4, float(np.abs(g.cpu().numpy() - r).max())
    for t in probe:
        g = net.read_tensor(t, B).cpu().numpy()
        assert np.abs(g - kept[t]).max() <= 2e-5 * max(1.0, float(np.abs(kept[t]).max()))
    gb, gc, gs = rt.yolo_decode_scores(got, anchors, 80)
    gsel, gnv = rt.nms_padded(gb, gs, 100, 0.5, 0.1)
    rb, rc, rs, rsel, rnv = O.yolo_nms(O.yolo_decode(ref, anchors, 80), 100, 0.5, 0.1)
    assert np.abs(gb.cpu().numpy() - rb).max() <= 1e-4 and np.abs(gs.cpu().numpy() - rs).max() <= 1e-4
    s2, n2 = O.nms_padded(gb.cpu().numpy(), gs.cpu().numpy(), 100, 0.5, 0.1)
    assert np.array_equal(s2, gsel.cpu().numpy()) and np.array_equal(n2, gnv.cpu().numpy())


# ---------------------------------------------------------------------------------------------- bf16 (config 5)
BF16_CASES = [
    (64, 16, 3, [], [dict(filters=128, size=3, stride=2), dict(filters=128, size=3), dict(filters=255, size=1, bn=False, act="linear")]),
    (128, 13, 2, [dict(filters=64, size=1), dict(filters=128, size=3, shortcut=-3)],
     [dict(filters=256, size=3), dict(filters=64, size=1), dict(filters=32, size=1)]),
    (32, 32, 2, [], [dict(filters=64, size=3, stride=2), dict(filters=64, size=3), dict(filters=64, size=1)]),
    (3, 32, 2, [dict(filters=32, size=3)], [dict(filters=64, size=3, stride=2), dict(filters=64, size=3), dict(filters=64, size=1)]),
]


def _bf16_ulp(x):
    return 2.0 ** -8 * max(1.0, float(np.abs(x).max()))


def _bf16_ulp_elem(a, b):
    """Per element: the spacing of bf16 numbers (8 significand bits) in the binade of the larger of |a|, |b|."""
    m = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.float32(2.0 ** -126)).astype(np.float64)
    return np.ldexp(1.0, np.floor(np.log2(m)).astype(np.int64) - 7)


@pytest.mark.parametrize("case", range(len(BF16_CASES)))
def test_bf16_conv_layers_match_bf16_oracle(rt, case):
    """bf16 MFMA conv vs the oracle run with the same roundings (bf16 weights/activations, fp32 arithmetic).
    Tolerance: 1 bf16 ulp of the output's magnitude (a different fp32 summation order can flip a final rounding);
    head outputs (fp32) are held to 2e-4 relative."""
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from yolo_v3_tf2_amd import _lib
    from oracle import oracle as O
    in_ch, S, B, chain, heads = BF16_CASES[case]
    p = mini_program(in_ch, chain, heads)
    w = synthetic_weights(p, seed=200 + case)
    rng = np.random.default_rng(case)
    x = (rng.standard_normal((B, S, S, in_ch)) if in_ch != 3 else rng.random((B, S, S, in_ch))).astype(np.float32)
    ref = O.forward(p, w, x, bf16=True)
    net = rt.Net(p)
    net.load_weights(w)
    net.plan(B, S, _lib.Y3_DTYPE_BF16)
    xin = _cuda(x) if in_ch == 3 else _cuda(O.round_bf16(x)).to(torch.bfloat16)
    got = net.forward(xin)
    torch.cuda.synchronize()
    for r, g in zip(ref, got):
        g = g.cpu().numpy().reshape(r.shape)
        assert np.abs(g - r).max() <= 2e-4 * max(1.0, float(np.abs(r).max())), (case, float(np.abs(g - r).max()))


@pytest.mark.parametrize("tile", [t for t, row in enumerate(_lib.TILES_BF16) if row[0] > 0 and t != 32])    # 32: the weight-resident kernel, tested below
def test_bf16_every_tile(rt, tile):
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from yolo_v3_tf2_amd import _lib
    from oracle import oracle as O
    bm, bn, _, bk = _lib.TILES_BF16[tile]
    cin = 32 if bk == 32 else 64
    p = mini_program(cin, [], [dict(filters=bn, size=3), dict(filters=bn, size=1), dict(filters=bn, size=3, stride=2)])
    w = synthetic_weights(p, seed=8)
    x = O.round_bf16(np.random.default_rng(8).standard_normal((3, 14, 14, cin)).astype(np.float32))
    ref = O.forward(p, w, x, bf16=True)
    net = rt.Net(p)
    net.load_weights(w)
    for slot in range(3):
        net.set_tile_bf16(slot, tile)
    net.plan(3, 14, _lib.Y3_DTYPE_BF16)
    got = net.forward(_cuda(x).to(torch.bfloat16))
    torch.cuda.synchronize()
    for r, g in zip(ref, got):
        assert np.abs(g.cpu().numpy().reshape(r.shape) - r).max() <= bf16_tile_bar(r)


@pytest.mark.parametrize("cin,cout,S,B", [(32, 64, 40, 3), (64, 128, 36, 2), (64, 64, 33, 2), (32, 128, 70, 1)])
def test_bf16_weight_resident_3x3_matches_oracle_and_generic_tiles(rt, cin, cout, S, B):
    """bf16 tile id 32 (csrc/conv_res_bf16.hip): 3x3 / stride-1 convs with 32 / 64 input channels run with their weights resident in
    LDS and the input patch of a 4 x 32-pixel tile fetched by LDS-DMA (zero padding = the buffer bounds check).  With and without
    a shortcut, BN + leaky and linear + bias, image widths that are not multiples of the 32-pixel tile (40, 36, 33, 70 -> ragged
    last column of tiles), heights not multiples of 4 (33, 70 -> ragged last row), several images (these shapes give at most 60 tiles
    to 256 workgroups, 36 to 128 per slice: ONE tile per workgroup; walks of three tiles across images are
    tests/test_persistent_walk_gpu.py): every output against the bf16-emulating oracle under the per-layer bf16 bar, and against the
    generic LDS-DMA tile of the same MFMA shape (same k order: tap * Cin + c in groups of 16) bit for bit."""
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from yolo_v3_tf2_amd import _lib
    from oracle import oracle as O
    chain = [dict(filters=cout, size=3), dict(filters=cin, size=1), dict(filters=cout, size=3, shortcut=-3),
             dict(filters=cin, size=1, act="linear"), dict(filters=cout, size=3, bn=False, act="linear")]
    heads = [dict(filters=64, size=1), dict(filters=32, size=1), dict(filters=64, size=1, bn=False, act="linear")]
    p = mini_program(cin, chain, heads)
    w = synthetic_weights(p, seed=52)
    x = np.random.default_rng(52).standard_normal((B, S, S, cin)).astype(np.float32)
    ops = p.conv_ops()
    probe = [o.dst for o in ops if o.size == 3]
    assert len(probe) == 3
    ref, kept = O.forward(p, w, x, bf16=True, keep=set(probe))
    xin = _cuda(O.round_bf16(x)).to(torch.bfloat16)
    outs, mids = {}, {}
    for name, tile in (("resident", 32), ("generic", 5 if cin == 32 else 10)):
        net = rt.Net(p)
        net.load_weights(w)
        net.keep_activations(True)
        for slot, o in enumerate(net.conv_ops):
            if o.size == 3:
                net.set_tile_bf16(slot, tile)
        net.plan(B, S, _lib.Y3_DTYPE_BF16)
        outs[name] = [g.clone() for g in net.forward(xin)]
        mids[name] = [net.read_tensor(t, B).clone() for t in probe]
        again = net.forward(xin)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs[name], again))
        for k, (t, g) in enumerate(zip(probe, mids[name])):
            # the 3x3 outputs themselves.  The first one reads the input directly: every element within its OWN bf16 ulp (a different
            # fp32 summation order may flip the final rounding); the later ones sit behind layers whose flipped roundings move their
            # sums by a fraction of an ulp of the layer's scale as well
            g = g.cpu().numpy()
            d = np.abs(g - kept[t])
            slack = (1e-5 if k == 0 else 2.0 ** -8) * float(np.abs(kept[t]).max())
            assert (d <= _bf16_ulp_elem(g, kept[t]) + slack).all(), (name, t, float(d.max()))
            assert float((d > 0).mean()) <= (0.002 if k == 0 else 0.05), (name, t, float((d > 0).mean()))
        for r, g in zip(ref, outs[name]):
            g = g.cpu().numpy().reshape(r.shape)
            assert np.abs(g - r).max() <= 4e-3 * max(1.0, float(np.abs(r).max())), (name, float(np.abs(g - r).max()))
    for a, b in zip(mids["resident"] + outs["resident"], mids["generic"] + outs["generic"]):
        assert torch.equal(a, b)


def test_bf16_intermediate_tensors_within_one_ulp(rt, program, weights):
    """Intermediate bf16 activations (after residual adds / the fused upsample+concat conv) vs the bf16 oracle."""
    from yolo_v3_tf2_amd import _lib
    from oracle import oracle as O
    S, B = 64, 2
    x = np.random.default_rng(3).random((B, S, S, 3), dtype=np.float32)
    ops = program.conv_ops()
    probe = [ops[0].dst, ops[3].dst, ops[8].dst, ops[25].dst] + [o.dst for o in ops if o.src1 >= 0]
    _, kept = O.forward(program, weights, x, keep=set(probe), bf16=True)
    net = rt.Net(program)
    net.load_weights(weights)
    net.keep_activations(True)
    net.plan(B, S, _lib.Y3_DTYPE_BF16)
    net.forward(_cuda(x))
    for t in probe:
        g = net.read_tensor(t, B).cpu().numpy()
        r = kept[t]
        bad = np.abs(g - r) > 2 * _bf16_ulp(r)          # a flipped rounding upstream moves a value by <= 1-2 ulp
        assert bad.mean() < 1e-3, (t, float(bad.mean()), float(np.abs(g - r).max()))


def test_bf16_network_deviation_is_reported(rt, program, weights, anchors):
    """Full network in bf16, free running, vs (a) the bf16-emulating oracle and (b) the fp32 oracle (what bf16 costs).

    What bounds (a): two bf16 pipelines that differ ONLY in the order of their fp32 partial sums do not stay within a
    few ulp of each other over 75 layers.  A perturbation of relative size e << ulp crosses a rounding boundary with
    probability e/ulp and then costs a whole ulp, so its rms after one rounding is sqrt(e * ulp) >> e: the fixed point
    of e -> sqrt(e * ulp) is e = ulp, and the two runs decorrelate to ~1 ulp rms (2^-8 relative) within ~10 layers.
    tests/test_oracle.py::test_bf16_free_running_floor shows this on the CPU alone (the oracle against itself with
    fp64 partial sums: 60-75 % of the elements differ from conv12 on, head logits differ by 4.6e-3 ... 5.5e-3 rel).
    The bar here is therefore that floor, measured in this very test: the kernel must be no further from the oracle
    than twice the oracle is from itself.  The per-layer kernel-correctness bar (every element within one ulp of the
    oracle's value on the same inputs) is test_bf16_every_layer_teacher_forced_within_one_ulp.
    The 1e-4 box bar of north_star is an fp32 statement; (b) is reported and bounded."""
    from yolo_v3_tf2_amd import _lib
    from oracle import oracle as O
    S, B = 96, 2
    x = np.random.default_rng(1234).random((B, S, S, 3), dtype=np.float32)
    ref16 = O.forward(program, weights, x, bf16=True)
    ref16b = O.forward(program, weights, x, bf16=True, acc64=True)      # same roundings, other summation
    ref32 = O.forward(program, weights, x)
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    floor_rel = max(rel(a, b) for a, b in zip(ref16b, ref16))
    floor_max = max(float(np.abs(a - b).max()) for a, b in zip(ref16b, ref16))
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(B, S, _lib.Y3_DTYPE_BF16)
    got = [g.cpu().numpy() for g in net.forward(_cuda(x))]
    d16 = max(float(np.abs(g - r).max()) for g, r in zip(got, ref16))
    d32 = max(float(np.abs(g - r).max()) for g, r in zip(got, ref32))
    rel16 = max(rel(g, r) for g, r in zip(got, ref16))
    rel32 = max(rel(g, r) for g, r in zip(got, ref32))
    print(f"bf16 head logits: vs bf16-oracle max {d16:.3e} rel {rel16:.3e} (oracle-vs-oracle floor: max {floor_max:.3e} "
          f"rel {floor_rel:.3e}); vs fp32-oracle max {d32:.3e} rel {rel32:.3e}")
    assert 2e-3 < floor_rel < 1.5e-2
    assert rel16 <= 2.0 * floor_rel and d16 <= 3.0 * floor_max
    assert rel32 < 3e-2 and d32 < 0.5          # bf16 quantisation through 75 layers


def test_bf16_every_layer_teacher_forced_within_one_ulp(rt, program, weights):
    """Kernel-correctness bar of the bf16 path, layer by layer on the real network: every fused launch is recomputed by
    the oracle FROM THE DEVICE'S OWN INPUT TENSORS (bf16 values are exact in fp32), rounded where the kernel rounds,
    and compared with the device's output: every element within one bf16 ulp (+ 1e-5 of the layer's magnitude for values
    that are tiny through cancellation), and at most 0.2 % of the elements different at all (a different fp32 summation order may flip a rounding; nothing else may differ).
    The free-running comparison (test_bf16_network_deviation_is_reported) cannot be this tight: two bf16 pipelines
    that differ by one flipped rounding decorrelate to ~1 ulp rms within a few layers (see that test)."""
    from yolo_v3_tf2_amd import _lib
    from oracle import oracle as O
    S, B = 96, 2
    x = np.random.default_rng(31).random((B, S, S, 3), dtype=np.float32)
    net = rt.Net(program)
    net.load_weights(weights)
    net.keep_activations(True)
    net.plan(B, S, _lib.Y3_DTYPE_BF16)
    grids = net.forward(_cuda(x))
    torch.cuda.synchronize()
    outs = {t: g.cpu().numpy().reshape(B, g.shape[1], g.shape[2], -1) for t, g in zip(program.outputs, grids)}

    def dev(t):
        return x if t == program.input_tensor else net.read_tensor(t, B).cpu().numpy()

    worst_frac, worst_ulp = 0.0, 0.0
    for o in program.conv_ops():
        a = dev(o.src0)
        if o.src0_upsample:
            a = O.upsample2x(a)
        if o.src1 >= 0:
            a = O.concat(a, dev(o.src1))
        i = o.conv_index
        w = {k: v for k, v in weights.items() if k.startswith(f"conv{i}.")}
        if o.cin != 3:
            w[f"conv{i}.w"] = O.round_bf16(w[f"conv{i}.w"])
        y = O.conv_block(a, w, i, o.size, o.stride, o.bn, o.leaky)
        if o.residual >= 0:
            y = O.add(dev(o.residual), y)
        if o.dst in outs:                                   # head conv: fp32 straight from the accumulators
            check_f32_conv(outs[o.dst], y, i)
            continue
        exp = O.round_bf16(y)
        got = net.read_tensor(o.dst, B).cpu().numpy()
        diff = np.abs(got.astype(np.float64) - exp.astype(np.float64))
        # one ulp of the element, plus the fp32 summation noise of the dot product itself (absolute, ~1e-6 of the
        # layer's magnitude: it exceeds an ulp only for results that are tiny through cancellation)
        ulp = _bf16_ulp_elem(got, exp) + 1e-5 * float(np.abs(exp).max())
        assert (diff <= ulp).all(), (i, float((diff / ulp).max()))
        frac = float((diff > 0).mean())
        worst_frac, worst_ulp = max(worst_frac, frac), max(worst_ulp, float((diff / ulp).max()))
        assert frac <= 2e-3, (i, frac)
    print(f"bf16 teacher-forced: worst per-layer mismatch fraction {worst_frac:.2e}, worst error {worst_ulp:.2f} ulp")


def test_bf16_full_size_batch128_graph_replay(rt, program, weights, anchors):
    """BASELINE config 5 per-GPU geometry: bf16, 128 x 416^2, the per-batch pipeline replayed from a HIP graph.
    Size-independent properties: replay == eager bit for bit, determinism across replays, batch independence (image i
    of the batch == the same image alone), detect rows sorted and above the threshold; images 0 and 127 against the
    bf16-emulating oracle at the free-running bar (relative L2 of the head logits; see the teacher-forced test for the
    per-layer ulp bar)."""
    from yolo_v3_tf2_amd import _lib
    from oracle import oracle as O
    B, S = 128, 416
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand((B, S, S, 3), generator=gen, device="cuda")
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(B, S, _lib.Y3_DTYPE_BF16)
    grids = [torch.empty((B, g, g, 3, 85), device="cuda") for g in net.grid_sizes()]

    def step():
        net.forward(x, out=grids)
        bb, cls, sc = rt.yolo_decode_scores(grids, anchors, 80)
        sel, nv = rt.nms_padded(bb, sc, 100, 0.5, 0.1)
        return rt.pack_detections(bb, cls, sc, sel, nv), nv

    ep, en = step()
    ep, en = ep.clone(), en.clone()
    eg = [g.clone() for g in grids]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gp, gn = step()
    for g in grids:
        g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gp, ep) and torch.equal(gn, en) and all(torch.equal(a, b) for a, b in zip(grids, eg))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gp, ep) and torch.equal(gn, en)
    for i in (0, 77, B - 1):
        gi = net.forward(x[i:i + 1].contiguous())
        assert all(torch.equal(a[i:i + 1], b) for a, b in zip(eg, gi)), i
    pb, ps, pc, pi = rt.unpack_detections(ep)
    psn, nvn = ps.cpu().numpy(), en.cpu().numpy()
    assert nvn.min() >= 0 and nvn.max() <= 100
    for i in range(B):
        s_ = psn[i, :nvn[i]]
        assert (s_ > 0.1).all() and (np.diff(s_) <= 0).all()
    for i in (0, B - 1):
        ref = O.forward(program, weights, x[i:i + 1].cpu().numpy(), bf16=True)
        rel = max(float(np.linalg.norm(g[i:i + 1].cpu().numpy() - r) / np.linalg.norm(r)) for g, r in zip(eg, ref))
        assert rel < 1.5e-2, (i, rel)


# ---------------------------------------------------------------------------------------------- network
@pytest.mark.parametrize("S,B", [(96, 2), (160, 1)])
def test_network_grids_match_oracle(rt, program, weights, S, B):
    """Full 75-conv forward.  Tolerance 1e-4 absolute on head logits of O(1) (north_star's bar is 1e-4 on
    boxes/scores; logits are upstream of them)."""
    from oracle import oracle as O
    x = np.random.default_rng(1234).random((B, S, S, 3), dtype=np.float32)
    ref = O.forward(program, weights, x)
    net = rt.Net(program)
    net.load_weights(weights)
    got = net.forward(_cuda(x))
    torch.cuda.synchronize()
    for r, g in zip(ref, got):
        assert np.abs(g.cpu().numpy() - r).max() <= NETWORK_GRID_BAR


def test_forward_is_deterministic(rt, program, weights):
    x = _cuda(np.random.default_rng(5).random((2, 96, 96, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    a = [g.clone() for g in net.forward(x)]
    b = net.forward(x)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("lanes", [2, 4])
def test_forward_lanes_bit_identical(rt, program, weights, lanes):
    """Sub-batches on forked streams (y3_net_set_lanes) give exactly the single-stream result."""
    x = _cuda(np.random.default_rng(6).random((4, 96, 96, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    a = [g.clone() for g in net.forward(x)]
    net.set_lanes(lanes)
    b = net.forward(x)
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("B", [1, 3, 5])
def test_lanes_on_a_side_stream_back_to_back(rt, program, weights, anchors, B):
    """Lane 0 of a multi-lane forward runs on the CALLER's stream and the other lanes fork from / join into it: the whole detect step
    enqueued several times back to back on a non-default stream, without a host synchronisation in between and with a different batch in
    every call, gives what one lane gives -- also when the batch is smaller than the lane count (fewer lanes) or ragged."""
    rng = np.random.default_rng(61)
    xs = [_cuda(rng.random((B, 96, 96, 3), dtype=np.float32)) for _ in range(3)]
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(B, 96)
    net.set_lanes(1)
    want = []
    for x in xs:
        p_, n_ = net.detect(x, anchors, 100, 0.5, 0.1)
        want.append((p_.clone(), n_.clone()))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for lanes in (2, 3):
        net.set_lanes(lanes)
        got = []
        with torch.cuda.stream(side):
            for x in xs:                       # three steps in a row on the side stream, no synchronisation in between
                got.append(net.detect(x, anchors, 100, 0.5, 0.1))
        side.synchronize()
        for (gp, gn), (wp, wn) in zip(got, want):
            assert torch.equal(gp, wp) and torch.equal(gn, wn)


@pytest.mark.parametrize("mode", ["f32x3", "f32x2", "bf16"])
def test_forward_lanes_bit_identical_other_modes(rt, program, weights, mode):
    """Same check in the plane-split and bf16 modes, with the three unequal lanes the tuning tables use."""
    from yolo_v3_tf2_amd import _lib
    dt = {"f32x3": _lib.Y3_DTYPE_F32X3, "f32x2": _lib.Y3_DTYPE_F32X2, "bf16": _lib.Y3_DTYPE_BF16}[mode]
    x = _cuda(np.random.default_rng(6).random((7, 96, 96, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(7, 96, dt)
    net.set_lanes(1)
    a = [g.clone() for g in net.forward(x)]
    for lanes in (2, 3):
        net.set_lanes(lanes)
        b = net.forward(x)
        torch.cuda.synchronize()
        for u, v in zip(a, b):
            assert torch.equal(u, v)


def test_bf16_heuristic_tiles_are_batch_and_lane_independent(rt, program, weights, monkeypatch):
    """without a tuning table the bf16 heuristic picks the 16x16x32 MFMA form (another K grouping than
    32x32x16: last bits differ) for the large 3x3 convs -- from the PLANNED batch, never from the rows of the call, or image i
    of a batch and the same image alone (or lanes 1 vs 2) would run different arithmetic.  32 x 416^2: the 52x52 convs (Cout 256)
    take the 16x16x32 form (M_plan = 86528 rows -> 338 tiles of 256x256), while a one-image call has 11."""
    from yolo_v3_tf2_amd import _lib
    monkeypatch.setenv("Y3_NO_TUNING", "1")
    B, S = 32, 416
    gen = torch.Generator(device="cuda").manual_seed(11)
    x = torch.rand((B, S, S, 3), generator=gen, device="cuda")
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(B, S, _lib.Y3_DTYPE_BF16)
    net.set_lanes(1)
    a = [g.clone() for g in net.forward(x)]
    net.set_lanes(2)
    b = net.forward(x)
    torch.cuda.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(a, b))                  # lanes 1 == lanes 2
    for i in (0, 19, B - 1):
        gi = net.forward(x[i:i + 1].contiguous())
        torch.cuda.synchronize()
        assert all(torch.equal(u[i:i + 1], v) for u, v in zip(a, gi)), i  # image i of the batch == the same image alone
    g4 = net.forward(x[8:12].contiguous())
    torch.cuda.synchronize()
    assert all(torch.equal(u[8:12], v) for u, v in zip(a, g4))


@pytest.mark.parametrize("mode", ["f32", "f32x2", "bf16"])
def test_early_chunk_bit_identical(rt, program, weights, mode):
    """y3_net_set_early_chunk: the first convs run a few images at a time, alone and together with lanes -- same bits."""
    from yolo_v3_tf2_amd import _lib
    dt = {"f32": _lib.Y3_DTYPE_F32, "f32x2": _lib.Y3_DTYPE_F32X2, "bf16": _lib.Y3_DTYPE_BF16}[mode]
    x = _cuda(np.random.default_rng(16).random((7, 96, 96, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    # same kernels in both schedules: the chunked leading segment runs conv0 and conv1 as two launches (the fused stem
    # sums conv0's 27 products in another order), so the reference run does too
    net.set_stem_fusion(False)
    net.plan(7, 96, dt)
    net.set_lanes(1)
    a = [g.clone() for g in net.forward(x)]
    for n_convs, chunk, lanes in ((9, 2, 1), (4, 3, 1), (9, 2, 2), (26, 1, 3), (9, 16, 1)):
        net.set_early_chunk(n_convs, chunk)
        net.plan(7, 96, dt)
        net.set_lanes(lanes)
        b = net.forward(x)
        torch.cuda.synchronize()
        for u, v in zip(a, b):
            assert torch.equal(u, v), (n_convs, chunk, lanes)
    with pytest.raises(rt.Y3Error):
        net.set_early_chunk(75, 2)


@pytest.mark.parametrize("B,lanes", [(3, 1), (5, 2), (7, 3)])
def test_detect_single_call_equals_composed_pipeline(rt, program, weights, anchors, B, lanes):
    """y3_net_detect (forward -> decode/score -> NMS -> pack on net-owned scratch) == the four calls made one by one: with one, two and three
    sub-batch lanes (ragged lane sizes 5 = 2 + 3, 7 = 2 + 2 + 3), on a second call (scratch reused), and replayed from a captured graph."""
    x = _cuda(np.random.default_rng(31).random((B, 128, 128, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(B, 128)
    net.set_lanes(lanes)
    grids = net.forward(x)
    bb, cc, ss = rt.yolo_decode_scores(grids, anchors, 80)
    sel, nv = rt.nms_padded(bb, ss, 100, 0.5, 0.05)
    want = rt.pack_detections(bb, cc, ss, sel, nv)
    for _ in range(2):     # second call reuses the scratch
        packed, nv2 = net.detect(x, anchors, 100, 0.5, 0.05)
        torch.cuda.synchronize()
        assert torch.equal(nv2, nv) and torch.equal(packed, want) and int(nv.sum()) > 0
    boxes, scores, classes, idx = rt.unpack_detections(packed)
    n0 = int(nv[0])
    assert torch.equal(idx[0, :n0], sel[0, :n0]) and torch.equal(boxes[0, :n0], bb[0][sel[0, :n0].long()])
    with pytest.raises(rt.Y3Error):
        net.detect(x, anchors, 0, 0.5, 0.05)
    # the same call captured into a HIP graph (the lanes' forked streams inside the capture) and replayed
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net.detect(x, anchors, 100, 0.5, 0.05)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gp, gn = net.detect(x, anchors, 100, 0.5, 0.05)
    for _ in range(2):
        gp.zero_()
        gn.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(gn, nv) and torch.equal(gp, want)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("S,B,lanes", [(96, 3, 1), (128, 5, 2), (416, 2, 1)])
def test_forward_decode_fused_heads_equal_the_composed_route(rt, program, weights, anchors, mode, S, B, lanes):
    """y3_net_forward_decode: the three head convs (1x1 + bias, 255 channels) decode their own output tiles -- sigmoid / exp *
    anchor / grid offset, class arg-max, score -- and never write the grids.  Boxes, class indices and scores must be BIT-
    IDENTICAL to y3_net_forward + y3_yolo_decode_scores on the same plan (fp32: conv_head.hip repeats the k order of the
    stand-alone launch; bf16: the fused epilogue decodes the very fp32 tile the grid store would have written), for sub-batch
    lanes too, on ragged last tiles (3 x 3^2 = 27 pixels of a 64-pixel tile), and on a second call."""
    from yolo_v3_tf2_amd import _lib
    dt = {"f32": _lib.Y3_DTYPE_F32, "bf16": _lib.Y3_DTYPE_BF16}[mode]
    x = _cuda(np.random.default_rng(41).random((B, S, S, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(B, S, dt)
    net.set_lanes(lanes)
    grids = net.forward(x)
    bb, cc, ss = rt.yolo_decode_scores(grids, anchors, 80)
    for _ in range(2):
        fb, fc, fs = net.forward_decode(x, anchors)
        torch.cuda.synchronize()
        assert torch.equal(fb, bb) and torch.equal(fc, cc) and torch.equal(fs, ss)
    # a smaller batch on the same plan
    fb1, fc1, fs1 = net.forward_decode(x[1:2].contiguous(), anchors)
    assert torch.equal(fb1, bb[1:2]) and torch.equal(fc1, cc[1:2]) and torch.equal(fs1, ss[1:2])


def test_forward_decode_falls_back_when_heads_cannot_decode(rt, program, weights, anchors, monkeypatch):
    """keep_activations plans (and the plane-split modes) take the composed route inside y3_net_forward_decode: same results."""
    from yolo_v3_tf2_amd import _lib
    x = _cuda(np.random.default_rng(42).random((2, 96, 96, 3), dtype=np.float32))
    for dt, keep in ((_lib.Y3_DTYPE_F32, True), (_lib.Y3_DTYPE_F32X2, False)):
        net = rt.Net(program)
        net.load_weights(weights)
        net.keep_activations(keep)
        net.plan(2, 96, dt)
        grids = net.forward(x)
        bb, cc, ss = rt.yolo_decode_scores(grids, anchors, 80)
        fb, fc, fs = net.forward_decode(x, anchors)
        assert torch.equal(fb, bb) and torch.equal(fc, cc) and torch.equal(fs, ss)


def test_full_size_batch_properties(rt, program, weights, anchors):
    """BASELINE size (batch 64, 416x416) through size-independent properties: (1) determinism, (2) batch
    independence -- image i of the 64-batch equals the same image run alone, bit for bit (the per-pixel K order does
    not depend on the tile an output pixel falls in), (3) the detect pipeline on the batch equals per-image runs."""
    from oracle import oracle as O
    B, S = 64, 416
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.rand((B, S, S, 3), generator=gen, device="cuda")
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(B, S)
    assert net.lanes == 2          # the shipped plan of the headline: two 32-image lanes on forked streams (tuning/f32_b64_s416.json)
    g1 = [t.clone() for t in net.forward(x)]
    g2 = net.forward(x)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    # (0) VERDICT r03 weak #2: one image of EACH lane of this very plan (tuned tiles, fused stem, chunk-major K) against the
    # oracle -- image 0 runs in lane 0, image 63 in lane 1 -- grids within 1e-4, then decode + NMS with every selection
    # difference attributed to a near-tie
    bb_, cls_, sc_ = rt.yolo_decode_scores(g1, anchors, 80)
    sel_, nv_ = rt.nms_padded(bb_, sc_, 100, 0.5, 0.1)
    for i in (0, B - 1):
        xi = x[i:i + 1].cpu().numpy()
        ref = O.forward(program, weights, xi)
        for r, g in zip(ref, g1):
            assert np.abs(g[i:i + 1].cpu().numpy().reshape(r.shape) - r).max() <= 1e-4, i
        r5 = O.yolo_nms(O.yolo_decode(ref, anchors, 80), 100, 0.5, 0.1)
        gb, gs = bb_[i:i + 1].cpu().numpy(), sc_[i:i + 1].cpu().numpy()
        assert _boxes_close(gb, r5[0]) and np.abs(gs - r5[2]).max() <= 1e-4, i
        s2, n2 = O.nms_padded(gb, gs, 100, 0.5, 0.1)
        assert np.array_equal(s2, sel_[i:i + 1].cpu().numpy()) and np.array_equal(n2, nv_[i:i + 1].cpu().numpy()), i
        _selection_explained(r5, (gb, cls_[i:i + 1].cpu().numpy(), gs, sel_[i:i + 1].cpu().numpy(), nv_[i:i + 1].cpu().numpy()))
    # (0b) VERDICT r04 weak #2: the route bench.py times -- y3_net_forward_decode, the head convs decoding their own tiles -- at the
    # driver's geometry and two-lane plan: its OWN outputs for images 0 and 63 against the oracle (boxes, scores, class index; NMS
    # bit-exact on identical inputs), and bit-identical to the composed route on the whole batch
    fb_, fc_, fs_ = net.forward_decode(x, anchors)
    assert torch.equal(fb_, bb_) and torch.equal(fc_, cls_) and torch.equal(fs_, sc_)
    fsel_, fnv_ = rt.nms_padded(fb_, fs_, 100, 0.5, 0.1)
    for i in (0, B - 1):
        r5 = O.detect(program, weights, x[i:i + 1].cpu().numpy(), anchors, 100, 0.5, 0.1)
        gb, gs, gc = fb_[i:i + 1].cpu().numpy(), fs_[i:i + 1].cpu().numpy(), fc_[i:i + 1].cpu().numpy()
        assert _boxes_close(gb, r5[0]) and np.abs(gs - r5[2]).max() <= 1e-4, i
        # class index: equal wherever the oracle's best class leads the runner-up by more than the score bar
        assert (gc != r5[1]).mean() <= 1e-3, i
        s2, n2 = O.nms_padded(gb, gs, 100, 0.5, 0.1)
        assert np.array_equal(s2, fsel_[i:i + 1].cpu().numpy()) and np.array_equal(n2, fnv_[i:i + 1].cpu().numpy()), i
    del bb_, cls_, sc_, sel_, nv_, fb_, fc_, fs_, fsel_, fnv_
    for i in (0, 17, 63):
        gi = net.forward(x[i:i + 1].contiguous())
        assert all(torch.equal(a[i:i + 1], b) for a, b in zip(g1, gi))
    bb, cls, sc = rt.yolo_decode_scores(g1, anchors, 80)
    sel, nv = rt.nms_padded(bb, sc, 100, 0.5, 0.1)
    assert bb.shape == (B, 10647, 4) and sel.shape == (B, 100) and int(nv.min()) >= 0 and int(nv.max()) <= 100
    for i in (3, 40):
        s1, n1 = rt.nms_padded(bb[i:i + 1].contiguous(), sc[i:i + 1].contiguous(), 100, 0.5, 0.1)
        assert torch.equal(s1[0], sel[i]) and int(n1[0]) == int(nv[i])
    # selected boxes are sorted by score and all above the threshold
    scn, seln, nvn = sc.cpu().numpy(), sel.cpu().numpy(), nv.cpu().numpy()
    for i in range(B):
        s_ = scn[i, seln[i, :nvn[i]]]
        assert (s_ > 0.1).all() and (np.diff(s_) <= 0).all()


def test_608_grids_match_oracle(rt, program, weights):
    """BASELINE config 3 geometry: 608x608 -> grids 19/38/76 (the reference's YAML hard-codes 13/26/52, F5)."""
    from oracle import oracle as O
    x = np.random.default_rng(608).random((1, 608, 608, 3), dtype=np.float32)
    ref = O.forward(program, weights, x)
    net = rt.Net(program)
    net.load_weights(weights)
    got = net.forward(_cuda(x))
    assert [g.shape[1] for g in got] == [19, 38, 76]
    for r, g in zip(ref, got):
        assert np.abs(g.cpu().numpy() - r).max() <= 1e-4


def test_608_end_to_end_detect(rt, program, weights, anchors):
    """BASELINE config 3 pipeline at its own resolution (608x608, N = 22743 boxes): boxes / scores within 1e-4 of the
    oracle's, NMS bit-exact on the device's own boxes, gathered detections equal."""
    from oracle import oracle as O
    x = np.random.default_rng(6080).random((1, 608, 608, 3), dtype=np.float32)
    rb, rc, rs, rsel, rnv = O.detect(program, weights, x, anchors, 100, 0.5, 0.1)
    net = rt.Net(program)
    net.load_weights(weights)
    grids = net.forward(_cuda(x))
    bb, cls, sc = rt.yolo_decode_scores(grids, anchors, 80)
    sel, nv = rt.nms_padded(bb, sc, 100, 0.5, 0.1)
    gb, gs = bb.cpu().numpy(), sc.cpu().numpy()
    assert gb.shape == (1, 22743, 4)
    assert _boxes_close(gb, rb) and np.abs(gs - rs).max() <= 1e-4
    s2, n2 = O.nms_padded(gb, gs, 100, 0.5, 0.1)
    assert np.array_equal(s2, sel.cpu().numpy()) and np.array_equal(n2, nv.cpu().numpy())
    _selection_explained((rb, rc, rs, rsel, rnv), (gb, cls.cpu().numpy(), gs, sel.cpu().numpy(), nv.cpu().numpy()))
    packed, nvd = net.detect(_cuda(x), anchors, 100, 0.5, 0.1)
    assert torch.equal(nvd, nv)
    pb, ps, pc, pi = rt.unpack_detections(packed)
    assert torch.equal(pi[0, :int(nv[0])], sel[0, :int(nv[0])])


def test_full_size_608_batch64_properties(rt, program, weights, anchors):
    """BASELINE config 3 at its own size: 64 x 608^2, fp32 -- the geometry whose first activations (64 x 608^2 x 32 x 4 B
    = 3.03 GB, 64 x 304^2 x 64 x 4 B = 1.51 GB) put byte offsets above 2^31.  Checks: images 0 and 63 of the batch
    against the oracle (head grids <= 1e-4, and conv0 / conv1 / conv2 outputs of the LAST image -- the highest
    addresses -- within 2e-5 of their magnitude), determinism, batch independence, detect == per-image runs."""
    from oracle import oracle as O
    B, S = 64, 608
    gen = torch.Generator(device="cuda").manual_seed(608)
    x = torch.rand((B, S, S, 3), generator=gen, device="cuda")
    ops = program.conv_ops()
    probe = [ops[0].dst, ops[1].dst, ops[2].dst]
    net = rt.Net(program)
    net.load_weights(weights)
    net.keep_activations(True)
    net.plan(B, S)
    g1 = [t.clone() for t in net.forward(x)]
    assert [tuple(g.shape) for g in g1] == [(B, 19, 19, 3, 85), (B, 38, 38, 3, 85), (B, 76, 76, 3, 85)]
    for i in (0, B - 1):
        ref, kept = O.forward(program, weights, x[i:i + 1].cpu().numpy(), keep=set(probe))
        for r, g in zip(ref, g1):
            assert np.abs(g[i:i + 1].cpu().numpy() - r).max() <= 1e-4, i
        if i == B - 1:
            for t in probe:
                full = net.read_tensor(t, B)
                got = full[i:i + 1].cpu().numpy()
                del full
                scale = max(1.0, float(np.abs(kept[t]).max()))
                assert np.abs(got - kept[t]).max() <= 2e-5 * scale, t
    g2 = net.forward(x)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))           # determinism
    del g2
    net.keep_activations(False)
    net.plan(B, S)
    packed, nv = net.detect(x, anchors, 100, 0.5, 0.1)
    assert int(nv.min()) >= 0 and int(nv.max()) <= 100
    # this plan runs conv0 + conv1 as the fused stem kernel (the keep_activations plan above could not): same network,
    # conv0 summed in another order -> close to g1, not equal
    gf = [t.clone() for t in net.forward(x)]
    for a, b in zip(g1, gf):
        assert float((a - b).abs().max()) <= 2e-5 * max(1.0, float(a.abs().max()))
    del g1
    for i in (7, B - 1):                                              # batch independence of the whole pipeline
        gi = net.forward(x[i:i + 1].contiguous())
        for a, b in zip(gf, gi):
            assert torch.equal(a[i:i + 1], b)                         # bit for bit: no kernel of the plan splits a sum by batch
        p1, n1 = net.detect(x[i:i + 1].contiguous(), anchors, 100, 0.5, 0.1)
        assert int(n1[0]) == int(nv[i])
        b_a, s_a, c_a, i_a = rt.unpack_detections(packed[i:i + 1])
        b_b, s_b, c_b, i_b = rt.unpack_detections(p1)
        assert torch.equal(i_a, i_b) and torch.equal(c_a, c_b) and torch.equal(b_a, b_b)
    pb, ps, pc, pi = rt.unpack_detections(packed)
    psn, nvn = ps.cpu().numpy(), nv.cpu().numpy()
    for i in range(B):
        s_ = psn[i, :nvn[i]]
        assert (s_ > 0.1).all() and (np.diff(s_) <= 0).all() and (psn[i, nvn[i]:] == 0).all()


def test_hipgraph_capture_replays_identically(rt, program, weights, anchors):
    """The whole per-batch pipeline (conv program incl. forked lanes, decode, NMS, pack) captured in a HIP graph."""
    x = _cuda(np.random.default_rng(9).random((4, 96, 96, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(4, 96)
    net.set_lanes(2)

    def step():
        grids = net.forward(x)
        bb, cls, sc = rt.yolo_decode_scores(grids, anchors, 80)
        sel, nv = rt.nms_padded(bb, sc, 100, 0.5, 0.1)
        return rt.pack_detections(bb, cls, sc, sel, nv), nv

    ref_p, ref_n = step()
    ref_p, ref_n = ref_p.clone(), ref_n.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_p, out_n = step()
    out_p.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_p, ref_p) and torch.equal(out_n, ref_n)


# ---------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("gs,B,nc", [((13, 26, 52), 2, 80), ((3, 6, 12), 5, 80), ((19, 38, 76), 1, 80), ((2, 4, 8), 3, 7)])
def test_decode_matches_oracle(rt, anchors, gs, B, nc):
    """yolo_decode: boxes/conf/probs within 2e-6 abs (expf differs by <= 1-2 ulp between ocml and libm;
    values are O(1)); shapes and concatenation order exact."""
    from oracle import oracle as O
    rng = np.random.default_rng(11)
    grids = [rng.normal(0, 1.5, (B, g, g, 3, 5 + nc)).astype(np.float32) for g in gs]
    rb, rc, rp = O.yolo_decode(grids, anchors, nc)
    gb, gc, gp = rt.yolo_decode([_cuda(g) for g in grids], anchors, nc)
    torch.cuda.synchronize()
    assert gb.shape == rb.shape and gc.shape == rc.shape and gp.shape == rp.shape
    scale = max(1.0, float(np.abs(rb).max()))
    assert np.abs(gb.cpu().numpy() - rb).max() <= 2e-6 * scale
    assert np.abs(gc.cpu().numpy() - rc).max() <= 2e-6
    assert np.abs(gp.cpu().numpy() - rp).max() <= 2e-6


def test_decode_scores_fused_equals_two_step(rt, anchors):
    """Fused decode+argmax/score == decode then class_scores, bit for bit (same device arithmetic)."""
    rng = np.random.default_rng(12)
    grids = [_cuda(rng.normal(0, 1.5, (3, g, g, 3, 85)).astype(np.float32)) for g in (13, 26, 52)]
    b1, cls1, s1 = rt.yolo_decode_scores(grids, anchors, 80)
    b2, conf, probs = rt.yolo_decode(grids, anchors, 80)
    cls2, s2 = rt.class_scores(conf, probs)
    assert torch.equal(b1, b2) and torch.equal(cls1, cls2) and torch.equal(s1, s2)
    # and the oracle's argmax on the device probabilities agrees exactly
    from oracle import oracle as O
    c = np.empty(cls2.shape, np.int64)
    s = np.empty(s2.shape, np.float32)
    O.lib().y3o_scores(conf.cpu().numpy().reshape(-1), probs.cpu().numpy(), c.size, 80, c.reshape(-1), s.reshape(-1))
    assert np.array_equal(c, cls2.cpu().numpy()) and np.array_equal(s, s2.cpu().numpy())


# ---------------------------------------------------------------------------------------------- nms
def _check_nms(rt, boxes, scores, M, T, S):
    from oracle import oracle as O
    rs, rn = O.nms_padded(boxes, scores, M, T, S)
    gs_, gn = rt.nms_padded(_cuda(boxes), _cuda(scores), M, T, S)
    torch.cuda.synchronize()
    assert np.array_equal(gn.cpu().numpy(), rn), (gn.cpu().numpy(), rn)
    assert np.array_equal(gs_.cpu().numpy(), rs)
    return rn


@pytest.mark.parametrize("N", [10647, 22743, 1000, 37])
def test_nms_stress_bit_exact(rt, N):
    """Index selection is bit-exact on identical inputs (duplicates force IoU==1 and sort ties)."""
    from tests.helpers import nms_stress_set
    boxes, scores = nms_stress_set(np.random.default_rng(99), 4, N)
    nv = _check_nms(rt, boxes, scores, 100, 0.5, 0.1)
    assert nv.max() > 0


@pytest.mark.parametrize("survivors", [0, 1, 99, 100, 101, "half"])
def test_nms_survivor_counts(rt, survivors):
    """0, 1, 99, 100, 101 and > N/2 survivors (disjoint boxes so that nothing is suppressed)."""
    N = 4096
    k = N // 2 + 17 if survivors == "half" else survivors
    rng = np.random.default_rng(5)
    # disjoint unit cells on a 64x64 lattice
    ii = np.arange(N)
    x0, y0 = (ii % 64) / 64.0, (ii // 64) / 64.0
    boxes = np.stack([x0 + 0.001, y0 + 0.001, x0 + 0.014, y0 + 0.014], -1).astype(np.float32)[None].repeat(2, 0)
    scores = np.full((2, N), 0.05, np.float32)
    for b in range(2):
        scores[b, rng.permutation(N)[:k]] = rng.uniform(0.2, 0.9, k).astype(np.float32)
    nv = _check_nms(rt, boxes, scores, 100, 0.5, 0.1)
    assert (nv == min(k, 100)).all()


def test_nms_many_candidates_global_sort_path(rt):
    """More candidates than the LDS sort holds (4096): exercises the global-memory sort, still bit-exact."""
    from tests.helpers import nms_stress_set
    boxes, scores = nms_stress_set(np.random.default_rng(1), 2, 10647, score_scale=3.0)
    assert (scores > 0.1).sum(1).min() > 4096
    _check_nms(rt, boxes, scores, 100, 0.5, 0.1)


@pytest.mark.parametrize("M,T,S", [(10, 0.3, 0.05), (1, 0.5, 0.1), (300, 0.7, 0.0), (100, 0.0, 0.1), (100, 1.0, 0.1)])
def test_nms_parameters(rt, M, T, S):
    from tests.helpers import nms_stress_set
    boxes, scores = nms_stress_set(np.random.default_rng(2), 3, 3000)
    _check_nms(rt, boxes, scores, M, T, S)


def test_nms_heavy_overlap_long_chains(rt):
    """Thousands of near-identical boxes: most candidates suppressed, many 256-candidate chunks walked."""
    rng = np.random.default_rng(8)
    N = 8000
    c = rng.integers(0, 12, N)
    base = np.stack([0.1 + 0.07 * c, 0.2 + 0.0 * c, 0.16 + 0.07 * c, 0.5 + 0.0 * c], -1)
    boxes = (base + rng.normal(0, 0.004, (N, 4))).astype(np.float32)[None]
    scores = rng.uniform(0.11, 0.99, (1, N)).astype(np.float32)
    _check_nms(rt, boxes, scores, 100, 0.5, 0.1)


def test_nms_kept_list_spills_past_lds_capacity(rt):
    """More than 2048 surviving boxes that are never *selected* (no positive coordinate: TF counts a position as
    selected iff any coordinate of its box is > 0): the kept list outgrows its LDS array and continues in the global
    workspace; later candidates must still be suppressed by those spilled survivors.  Bit-exact against the oracle."""
    from oracle import oracle as O
    rng = np.random.default_rng(21)
    n_neg, n_ord = 3000, 400
    # disjoint cells in the negative quadrant (all survive, none is selected), highest scores, score order = index order
    gx, gy = np.meshgrid(np.arange(60), np.arange(50))
    x0 = -(gx.reshape(-1)[:n_neg] + 1.0) * 0.01
    y0 = -(gy.reshape(-1)[:n_neg] + 1.0) * 0.01
    neg = np.stack([x0, y0, x0 + 0.008, y0 + 0.008], -1)
    # next in score: copies of survivors that sit in the SPILL region (kept-list position >= 2048) and touch x = 0,
    # stretched to xmax = +0.001 -> one positive coordinate (selectable), IoU with the original 0.73 >= 0.5 (suppressed)
    src = np.array([i for i in range(2100, n_neg) if i % 60 == 0])
    cop = neg[src].copy()
    cop[:, 2] = 0.001
    c = rng.random((n_ord, 2)) * 0.8 + 0.1
    wh = rng.random((n_ord, 2)) * 0.05 + 0.01
    ordn = np.concatenate([c - wh, c + wh], -1)
    boxes = np.concatenate([neg, cop, ordn]).astype(np.float32)[None]
    scores = np.concatenate([0.9 - 1e-5 * np.arange(n_neg), 0.6 - 1e-4 * np.arange(len(src)),
                             0.5 - 1e-4 * rng.permutation(n_ord)]).astype(np.float32)[None]
    is_copy = np.zeros(boxes.shape[1], bool)
    is_copy[n_neg:n_neg + len(src)] = True
    perm = rng.permutation(boxes.shape[1])
    boxes, scores, is_copy = np.ascontiguousarray(boxes[:, perm]), np.ascontiguousarray(scores[:, perm]), is_copy[perm]
    rsel, rnv = O.nms_padded(boxes, scores, 100, 0.5, 0.1)
    assert int(rnv[0]) == 100 and not is_copy[rsel[0]].any()          # every copy is suppressed by a spilled survivor
    sel, nv = rt.nms_padded(_cuda(boxes), _cuda(scores), 100, 0.5, 0.1)
    assert np.array_equal(nv.cpu().numpy(), rnv) and np.array_equal(sel.cpu().numpy(), rsel)
    # control: without the negative boxes the copies are the first boxes selected
    keep = scores[0] < 0.7
    sel2, nv2 = rt.nms_padded(_cuda(boxes[:, keep]), _cuda(scores[:, keep]), 100, 0.5, 0.1)
    assert int(is_copy[keep][sel2.cpu().numpy()[0, :int(nv2[0])]].sum()) == len(src) == 15


def test_detect_first_call_inside_graph_capture(rt, program, weights, anchors):
    """y3_net_detect allocates nothing: planned once, its FIRST invocation can be the one that is captured."""
    x = _cuda(np.random.default_rng(10).random((3, 96, 96, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(3, 96)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            packed, nv = net.detect(x, anchors, 100, 0.5, 0.1)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    p1, n1 = packed.clone(), nv.clone()
    p2, n2 = net.detect(x, anchors, 100, 0.5, 0.1)
    torch.cuda.synchronize()
    assert torch.equal(p1, p2) and torch.equal(n1, n2) and int(n1.min()) >= 0
    with pytest.raises(rt.Y3Error):
        net.detect(x, anchors, 0, 0.5, 0.1)
    with pytest.raises(rt.Y3Error, match="max_boxes"):
        net.detect(x, anchors, 2000, 0.5, 0.1)


def test_y3_comm_allgather_single_rank_and_graph(rt, program, weights, anchors):
    """The collective behind the C ABI (y3_comm_init_rank / y3_allgather_results) with one rank: RCCL really runs
    (communicator, group of two all-gathers on the compute stream), the gathered rows equal the local rows, and
    y3_net_detect + the gather replay from ONE HIP graph.  (More ranks need more GPUs: the world-size-2 semantics are
    covered on CPU tensors by tests/test_distributed_gloo.py.)"""
    from yolo_v3_tf2_amd.parallel import Y3Comm
    comm = Y3Comm(Y3Comm.new_unique_id(), 1, 0)
    x = _cuda(np.random.default_rng(12).random((4, 96, 96, 3), dtype=np.float32))
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(4, 96)
    packed, nv = net.detect(x, anchors, 100, 0.5, 0.1)
    g_p, g_n = comm.allgather(packed, nv)
    torch.cuda.synchronize()
    assert torch.equal(g_p, packed) and torch.equal(g_n, nv) and int(nv.sum()) > 0
    out = (torch.zeros_like(g_p), torch.zeros_like(g_n))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            p2, n2 = net.detect(x, anchors, 100, 0.5, 0.1)
            comm.allgather(p2, n2, out=out)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], packed) and torch.equal(out[1], nv)
    with pytest.raises(rt.Y3Error):
        comm.allgather(packed.float(), nv)
    comm.close()


def test_pack_detections(rt):
    from tests.helpers import nms_stress_set
    from oracle import oracle as O
    boxes, scores = nms_stress_set(np.random.default_rng(4), 3, 2000)
    cls = np.random.default_rng(4).integers(0, 80, scores.shape).astype(np.int64)
    sel, nv = rt.nms_padded(_cuda(boxes), _cuda(scores), 100, 0.5, 0.1)
    packed = rt.pack_detections(_cuda(boxes), _cuda(cls), _cuda(scores), sel, nv)
    pb, ps, pc, pi = [t.cpu().numpy() for t in rt.unpack_detections(packed)]
    sel, nv = sel.cpu().numpy(), nv.cpu().numpy()
    for b in range(3):
        ob, oc, os_ = O.gather_valid(boxes[b], cls[b], scores[b], sel[b], nv[b])
        n = int(nv[b])
        assert np.array_equal(pb[b, :n], ob) and np.array_equal(pc[b, :n], oc) and np.array_equal(ps[b, :n], os_)
        assert np.array_equal(pi[b, :n], sel[b, :n])
        assert not pb[b, n:].any() and not pc[b, n:].any()


# ---------------------------------------------------------------------------------------------- image input
@pytest.mark.parametrize("H,W,C,S", [(667, 812, 4, 416), (100, 37, 3, 64), (32, 32, 3, 96), (1080, 1920, 3, 608)])
def test_preprocess_matches_host_restatement(rt, H, W, C, S):
    """uint8 -> [0,1] -> bilinear resize on the GPU == the NumPy restatement of TF's kernel, bit for bit
    (same fp32 operations in the same order, no contraction)."""
    from yolo_v3_tf2_amd.core.utils import resize_bilinear
    rng = np.random.default_rng(H)
    img = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    ref = resize_bilinear(img[..., :3].astype(np.float32) * np.float32(1.0 / 255.0), S, S)
    batch = torch.zeros((2, S, S, 3), device="cuda")
    rt.preprocess_image(_cuda(img), batch, 1)
    torch.cuda.synchronize()
    got = batch[1].cpu().numpy()
    assert not batch[0].any()
    assert np.array_equal(got, ref), float(np.abs(got - ref).max())
    # float32 input path
    f = rng.random((H, W, 3), dtype=np.float32)
    rt.preprocess_image(_cuda(f), batch, 0)
    assert np.array_equal(batch[0].cpu().numpy(), resize_bilinear(f, S, S))


def test_preprocess_divide_after_matches_tfrecord_host_path(rt):
    """tfrecords source order of operations (reference core/load_tfrecords.py:46-48): resize the 0..255 values, then a
    true divide by 255 -- GPU == parse_tfrecord_fn's NumPy arithmetic, bit for bit."""
    from yolo_v3_tf2_amd.core.utils import resize_bilinear
    rng = np.random.default_rng(77)
    for (H, W, S) in ((37, 61, 32), (128, 128, 416), (500, 375, 96)):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        ref = resize_bilinear(img.astype(np.float32), S, S) / np.float32(255)
        batch = torch.zeros((1, S, S, 3), device="cuda")
        rt.preprocess_image(_cuda(img), batch, 0, divide_after=True)
        got = batch[0].cpu().numpy()
        assert np.array_equal(got, ref), float(np.abs(got - ref).max())
    with pytest.raises(rt.Y3Error):
        rt.preprocess_image(_cuda(rng.random((8, 8, 3), dtype=np.float32)), torch.zeros((1, 8, 8, 3), device="cuda"), 0,
                            divide_after=True)


# ---------------------------------------------------------------------------------------------- end to end
def test_end_to_end_detect(rt, program, weights, anchors):
    """image -> 5-tuple.  Two-stage bar: (i) NMS on the *device's own* boxes/scores is
    bit-exact vs the oracle NMS on those same tensors; (ii) boxes/scores within 1e-4 of the oracle's
    end-to-end values and the selected sets equal unless a near-tie (|delta| < 1e-5 around a threshold)
    explains the flip, which is reported, not hidden."""
    from oracle import oracle as O
    from yolo_v3_tf2_amd.inference import DetectModel
    from yolo_v3_tf2_amd.core.parse_model import YoloModel
    S, B = 160, 2
    x = np.random.default_rng(1234).random((B, S, S, 3), dtype=np.float32)
    m = YoloModel(program)
    m.set_weights_dict(weights)
    det = DetectModel(m, anchors, 80, 100, 0.5, 0.1)
    gb, gc, gs_, gsel, gnv = det.predict(x)
    rb, rc, rs, rsel, rnv = O.detect(program, weights, x, anchors)
    assert np.abs(gb - rb).max() <= 1e-4 and np.abs(gs_ - rs).max() <= 1e-4
    # (i) NMS bit-exact on identical inputs
    s2, n2 = O.nms_padded(gb, gs_, 100, 0.5, 0.1)
    assert np.array_equal(s2, gsel) and np.array_equal(n2, gnv)
    # (ii) end-to-end selection: equal, or every flip is a near-tie of the score threshold, the sort order or the IoU
    # threshold (image, position, boxes and margin printed)
    _selection_explained((rb, rc, rs, rsel, rnv), (gb, gc, gs_, gsel, gnv))
    assert np.array_equal(gc, rc) or np.abs(gs_ - rs).max() < 1e-4


def test_inference_counterpart_config1(rt, program, weights, anchors, tmp_path):
    """BASELINE config 1 (plumbing): the reference's YAML keys -> Inference()(**cfg) on the reference's own test image
    (datasets/coco2012/images/girl.png, config/detect_config_coco.yaml:11) with the config's own limits; detect.txt and
    the gathered detections equal the committed oracle fixture (tests/golden/girl_416_detections.npz) and what the
    oracle produces live from the same resized image."""
    import os
    import yaml
    from oracle import oracle as O
    from yolo_v3_tf2_amd.inference import Inference
    from yolo_v3_tf2_amd.weights import save_weights
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "config/detect_config_coco.yaml")))
    assert cfg["image_file_path"].endswith("girl.png") and cfg["nms_score_threshold"] == 0.1
    wpath = str(tmp_path / "w.safetensors")
    save_weights(wpath, weights)
    cfg.update(input_weights_path=wpath, output_dir=str(tmp_path / "out"),
               model_config_file=os.path.join(root, cfg["model_config_file"]),
               classes_name_file=os.path.join(root, cfg["classes_name_file"]),
               anchors_file=os.path.join(root, cfg["anchors_file"]),
               image_file_path=os.path.join(root, cfg["image_file_path"]))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        results = Inference()(**cfg)
    finally:
        os.chdir(cwd)
    assert len(results) == 1
    bboxes, classes, scores, names = results[0]
    lines = open(os.path.join(cfg["output_dir"], "detect.txt")).read().strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("[") and os.path.exists(os.path.join(cfg["output_dir"], "detect_0.jpg"))
    d = np.load(os.path.join(root, "tests/golden/girl_416_detections.npz"))
    assert len(bboxes) == int(d["num_valid"][0]) and np.array_equal(classes, d["classes"])
    assert _boxes_close(bboxes, d["boxes"]) and np.abs(scores - d["scores"]).max() <= 1e-4
    img = O.resize_bilinear(O.decode_image_rgb01(cfg["image_file_path"]), 416, 416)[None]
    rb, rc, rs, rsel, rnv = O.detect(program, weights, img, anchors, 100, 0.5, 0.1)
    ob, oc, os_ = O.gather_valid(rb[0], rc[0], rs[0], rsel[0], rnv[0])
    assert len(bboxes) == len(ob) and np.array_equal(classes, oc)
    assert _boxes_close(bboxes, ob) and np.abs(scores - os_).max() <= 1e-4
    assert lines[0].count("%") == len(ob)


def test_plugin_surface_composition(rt, program, weights, anchors):
    """The reference's own composition, executed on the GPU through the drop-in modules (reference: inference.py:109-115):
        grids = model(x); decoded = yolo_decode(grids, anchors_table, nclasses); out = YoloNmsLayer(100, .5, .1)(decoded)
    Every stage against the oracle; and the fused one-kernel decode+score path gives the identical 5-tuple."""
    from oracle import oracle as O
    from yolo_v3_tf2_amd.core.parse_model import Input, ParseModel
    from yolo_v3_tf2_amd.core.yolo_decode_layer import yolo_decode
    from yolo_v3_tf2_amd.core.yolo_nms import yolo_nms
    from yolo_v3_tf2_amd.core.yolo_nms_layer import YoloNmsLayer
    from yolo_v3_tf2_amd.inference import DetectModel
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "config/models/yolov3/model.yaml")))
    model = ParseModel().build_model(Input(shape=(None, None, 3)), cfg["sub_models_configs"], cfg["output_stage"],
                                     nclasses=80, config_root=root)
    model.set_weights_dict(weights)
    x = np.random.default_rng(77).random((3, 96, 96, 3), dtype=np.float32)
    grids = model(x)                                                         # inference.py:109
    ref_grids = O.forward(program, weights, x)
    for g, r in zip(grids, ref_grids):
        assert tuple(g.shape) == r.shape and np.abs(g.cpu().numpy() - r).max() <= 1e-4
    decoded = yolo_decode(grids, anchors, 80)                                # inference.py:111
    rb, rconf, rprobs = O.yolo_decode(ref_grids, anchors, 80)
    assert [tuple(t.shape) for t in decoded] == [rb.shape, rconf.shape, rprobs.shape]
    assert np.abs(decoded[0].cpu().numpy() - rb).max() <= 1e-4
    assert np.abs(decoded[1].cpu().numpy() - rconf).max() <= 1e-4 and np.abs(decoded[2].cpu().numpy() - rprobs).max() <= 1e-4
    layer = YoloNmsLayer(100, 0.5, 0.1, name="nms")                          # inference.py:114
    out = layer(decoded)                                                     # inference.py:115
    assert len(out) == 5
    bboxes, cls, scores, sel, nv = (t.cpu().numpy() for t in out)
    assert cls.dtype == np.int64 and sel.dtype == np.int32 and nv.dtype == np.int32 and sel.shape == (3, 100)
    # NMS is defined on identical inputs: the oracle NMS of the device's own decoded tensors, bit-exact
    ob, ocls, osc, osel, onv = O.yolo_nms(tuple(t.cpu().numpy() for t in decoded), 100, 0.5, 0.1)
    assert np.array_equal(cls, ocls) and np.array_equal(scores, osc) and np.array_equal(sel, osel) and np.array_equal(nv, onv)
    assert np.array_equal(bboxes, ob)
    # end to end against the oracle's own pipeline: values within the 1e-4 bar
    eb, ecls, esc, esel, env_ = O.detect(program, weights, x, anchors, 100, 0.5, 0.1)
    assert np.abs(bboxes - eb).max() <= 1e-4 and np.abs(scores - esc).max() <= 1e-4
    # the function form and the two DetectModel routes
    out_fn = yolo_nms(decoded, 100, 0.5, 0.1)
    assert all(torch.equal(a, b) for a, b in zip(out, out_fn))
    for fused in (False, True):
        dm = DetectModel(model, anchors, 80, 100, 0.5, 0.1, fused=fused)
        got = dm.predict(x)
        for a, b in zip(got, (bboxes, cls, scores, sel, nv)):
            assert np.array_equal(a, b), fused


def test_backbone_only_config2(rt, program, weights):
    """BASELINE config 2 (Darknet-53 backbone forward only, fp32): a program built from the backbone sub-model alone
    (output_stage='backbone' -> its three feature maps) vs the oracle at a small size, and -- at the config's own
    geometry, batch 32 x 416^2 -- bit-identical to the same tensors inside the full network (size-independent check)."""
    import os
    import yaml
    from oracle import oracle as O
    from yolo_v3_tf2_amd.graph import build_program, find_config_root
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mf = os.path.join(root, "config/models/yolov3/model.yaml")
    cfg = yaml.safe_load(open(mf))
    bb_cfg = [c for c in cfg["sub_models_configs"] if c["name"] == "backbone"]
    bb = build_program(bb_cfg, "backbone", 0, find_config_root(mf, bb_cfg))
    assert len(bb.conv_nodes) == 52 and [bb.tensors[o].channels for o in bb.outputs] == [256, 512, 1024]
    assert abs(bb.flops_per_image(416) / 1e9 - 49.031610) < 1e-5
    bw = {k: v for k, v in weights.items() if int(k.split(".")[0][4:]) < 52}
    x = np.random.default_rng(2).random((2, 96, 96, 3), dtype=np.float32)
    ref = O.forward(bb, bw, x)
    net = rt.Net(bb)
    net.load_weights(bw)
    got = net.forward(_cuda(x))
    for r, g in zip(ref, got):
        assert np.abs(g.cpu().numpy() - r).max() <= 1e-4 * max(1.0, float(np.abs(r).max()))
    # config-2 geometry
    B, S = 32, 416
    xb = torch.rand((B, S, S, 3), generator=torch.Generator(device="cuda").manual_seed(3), device="cuda")
    net.plan(B, S)
    net.set_stem_fusion(False)   # the keep_activations plan below runs conv0 and conv1 as two launches: same kernels here
    outs = [t.clone() for t in net.forward(xb)]
    full = rt.Net(program)
    full.load_weights(weights)
    full.keep_activations(True)
    full.plan(B, S)
    full.forward(xb)
    # the full program's backbone outputs: dst of the convs with the same creation index as the backbone's output convs
    by_index = {o.conv_index: o.dst for o in program.conv_ops()}
    for t_bb, o in zip(bb.outputs, outs):
        idx = [c.conv_index for c in bb.conv_ops() if c.dst == t_bb][0]
        assert torch.equal(full.read_tensor(by_index[idx], B).reshape(o.shape), o)


def test_inference_counterpart_tfrecords_source(rt, program, weights, anchors, tmp_path):
    """input_data_source='tfrecords' (reference inference.py:119-144): records written with the TFRecord writer, batches
    of 2 through the GPU input stage and the detect path; per-image detections equal the oracle's on the host-parsed
    dataset images (core/load_tfrecords.parse_tfrecords)."""
    import os
    import yaml
    from oracle import oracle as O
    from tests.helpers import make_tfrecord_dataset as make_dataset
    from yolo_v3_tf2_amd.core.load_tfrecords import parse_tfrecords
    from yolo_v3_tf2_amd.inference import Inference
    from yolo_v3_tf2_amd.weights import save_weights
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "config/detect_config_coco.yaml")))
    rec_dir = tmp_path / "rec"
    rec_dir.mkdir()
    make_dataset(str(rec_dir), np.random.default_rng(8), n=5, sizes=((200, 260), (300, 300), (180, 420)))
    wpath = str(tmp_path / "w.safetensors")
    save_weights(wpath, weights)
    S = 160
    cfg.update(input_weights_path=wpath, output_dir=str(tmp_path / "out"), image_size=S, batch_size=2,
               input_data_source="tfrecords", tfrecords_dir=str(rec_dir),
               model_config_file=os.path.join(root, cfg["model_config_file"]),
               classes_name_file=os.path.join(root, cfg["classes_name_file"]),
               anchors_file=os.path.join(root, cfg["anchors_file"]), nms_score_threshold=0.05)
    results = Inference()(**cfg)
    assert len(results) == 5
    lines = open(os.path.join(cfg["output_dir"], "detect.txt")).read().strip().splitlines()
    assert len(lines) == 5 and all(os.path.exists(os.path.join(cfg["output_dir"], f"detect_{i}.jpg")) for i in range(5))
    imgs = np.stack([x for x, _ in parse_tfrecords(str(rec_dir), S, 100)])
    rb, rc, rs, rsel, rnv = O.detect(program, weights, imgs, anchors, 100, 0.5, 0.05)
    for i, (bboxes, classes, scores, _names) in enumerate(results):
        ob, oc, os_ = O.gather_valid(rb[i], rc[i], rs[i], rsel[i], rnv[i])
        assert len(bboxes) == len(ob) and np.array_equal(classes, oc)
        if len(ob):
            assert np.abs(bboxes - ob).max() <= 1e-4 and np.abs(scores - os_).max() <= 1e-4


def test_evaluate_driver_counters_match_oracle(rt, program, weights, anchors, tmp_path):
    """evaluate_yolov3.evaluate on a TFRecord set: the per-class counters equal those obtained by feeding the oracle's
    detections of the same host-parsed images through the same EvaluateDetections."""
    import os
    from oracle import oracle as O
    from tests.helpers import jpeg_bytes as _jpeg
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev
    from yolo_v3_tf2_amd.core import load_tfrecords as m
    from yolo_v3_tf2_amd.evaluate_detections import EvaluateDetections
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(21)
    names = [l.rstrip("\n") for l in open(os.path.join(root, "datasets/coco2012/coco.names"))]
    payloads = []
    for i in range(4):
        lo = (rng.random((2, 2)) * 0.5).astype(np.float32)
        hi = lo + 0.3
        payloads.append(m.make_example({"image/encoded": _jpeg(rng, 120, 150),
                                        "image/object/class/text": [names[i].encode(), names[i + 7].encode()],
                                        "image/object/bbox/xmin": lo[:, 0], "image/object/bbox/ymin": lo[:, 1],
                                        "image/object/bbox/xmax": hi[:, 0], "image/object/bbox/ymax": hi[:, 1]}))
    m.write_records(str(tmp_path / "set.tfrec"), payloads)
    S = 128
    cfg = dict(tfrecords_dir=str(tmp_path), image_size=S, batch_size=2, yolo_max_boxes=100, nms_iou_threshold=0.5,
               classes_name_file=os.path.join(root, "datasets/coco2012/coco.names"),
               anchors_file=os.path.join(root, "datasets/coco2012/anchors.txt"),
               model_config_file=os.path.join(root, "config/models/yolov3/model.yaml"))
    res = ev.evaluate(cfg, [0.05, 0.3], evaluate_iou_threshold=0.1, weights=weights)
    assert [r[0] for r in res] == [0.05, 0.3]
    data = list(m.parse_tfrecords(str(tmp_path), S, 100, cfg["classes_name_file"]))
    imgs = np.stack([x for x, _ in data])
    for thr, recall, precision, counters, one in res:
        rb, rc, rs, rsel, rnv = O.detect(program, weights, imgs, anchors, 100, 0.5, thr)
        ref, ref1 = EvaluateDetections(80, 0.1), EvaluateDetections(80, 0.1)
        for i, (_, y) in enumerate(data):
            y = y[y[:, 4] == 1]
            ob, oc, _s = O.gather_valid(rb[i], rc[i], rs[i], rsel[i], rnv[i])
            ref.evaluate(ob, oc, y[:, :4], y[:, 5].astype(np.int32))
            ref1.evaluate(ob, np.zeros_like(oc), y[:, :4], np.zeros(len(y), np.int32))
        for k in ("preds", "gts", "tp", "fp", "fn"):
            assert np.array_equal(counters[k], ref.counters[k]), (thr, k)
            assert np.array_equal(one[k], ref1.counters[k]), (thr, k)
        assert counters["examples"] == 4 and counters["gts"].sum() == 8 and recall.shape == (80,)


@pytest.mark.parametrize("mode", ["f32x2", "f32x3", "bf16"])
def test_backbone_only_other_modes(rt, program, weights, mode):
    """Backbone-only program in the non-fp32 modes: its outputs are residual convs that later convs read again, so they
    are produced in the arena in the mode's format and converted to the caller's fp32 buffers at the end of the forward.
    Plane-split modes: fp32 tolerance against the fp32 oracle; bf16: against the bf16-emulating oracle (which rounds the
    staged outputs like the kernel does), within three times the free-running floor -- the oracle's own deviation from
    itself when only the order of its fp32 partial sums changes (test_bf16_network_deviation_is_reported)."""
    import os
    import yaml
    from oracle import oracle as O
    from yolo_v3_tf2_amd import _lib
    from yolo_v3_tf2_amd.graph import build_program, find_config_root
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mf = os.path.join(root, "config/models/yolov3/model.yaml")
    cfg = yaml.safe_load(open(mf))
    bb_cfg = [c for c in cfg["sub_models_configs"] if c["name"] == "backbone"]
    bb = build_program(bb_cfg, "backbone", 0, find_config_root(mf, bb_cfg))
    bw = {k: v for k, v in weights.items() if int(k.split(".")[0][4:]) < 52}
    x = np.random.default_rng(2).random((3, 96, 96, 3), dtype=np.float32)
    dt = {"f32x2": _lib.Y3_DTYPE_F32X2, "f32x3": _lib.Y3_DTYPE_F32X3, "bf16": _lib.Y3_DTYPE_BF16}[mode]
    ref = O.forward(bb, bw, x, bf16=(mode == "bf16"))
    floor = None
    if mode == "bf16":   # free-running floor: the oracle against itself with another summation (see the deviation test)
        refb = O.forward(bb, bw, x, bf16=True, acc64=True)
        floor = [float(np.abs(a - b).max()) for a, b in zip(refb, ref)]
    net = rt.Net(bb)
    net.load_weights(bw)
    net.plan(3, 96, dt)
    for lanes in (1, 2):
        net.set_lanes(lanes)
        got = net.forward(_cuda(x))
        torch.cuda.synchronize()
        for k, (r, g) in enumerate(zip(ref, got)):
            g = g.cpu().numpy().reshape(r.shape)
            scale = max(1.0, float(np.abs(r).max()))
            tol = 3.0 * floor[k] if mode == "bf16" else 1e-4 * scale
            assert np.abs(g - r).max() <= tol, (mode, lanes, float(np.abs(g - r).max()), tol)


def test_darknet_weights_file_to_device_detect(rt, program, weights, anchors, tmp_path):
    """Row n1 on the GPU: a Darknet `.weights` file for the whole 75-conv program, laid out BY THIS TEST from the
    reference's description of the format (reference convert.py:93-95 five int32 of header; :50-55 a batch-normalised
    conv stores 4 x filters floats as beta, gamma, mean, var; :58 a bias conv its bias; :61-68 then
    filters x in_dim x size x size weights in (Cout, Cin, kh, kw) order, conv by conv in creation order :96-137) --
    not through this package's writer -- then `model.load_weights(path).expect_partial()` (reference inference.py:102)
    -> DetectModel.predict on the device, against the oracle fed the very arrays the file was laid out from."""
    import struct
    from oracle import oracle as O
    from yolo_v3_tf2_amd.core.parse_model import YoloModel
    from yolo_v3_tf2_amd.inference import DetectModel
    path = tmp_path / "hand_laid.weights"
    with open(path, "wb") as f:
        f.write(struct.pack("<5i", 0, 2, 5, 32013312, 0))
        for i, nd in enumerate(program.conv_nodes):
            assert nd.conv_index == i
            w = weights[f"conv{i}.w"]                                  # (kh, kw, Cin, Cout): the Keras layout
            k, _, cin, cout = w.shape
            if f"conv{i}.gamma" in weights:
                for key in ("beta", "gamma", "mean", "var"):              # Darknet order
                    f.write(np.asarray(weights[f"conv{i}.{key}"], "<f4").tobytes())
            else:
                f.write(np.asarray(weights[f"conv{i}.bias"], "<f4").tobytes())
            dk = np.empty((cout, cin, k, k), "<f4")                        # element by element: no transpose helper
            for u in range(k):
                for v in range(k):
                    dk[:, :, u, v] = w[u, v].T
            f.write(dk.tobytes())
    assert os.path.getsize(path) == 20 + 4 * program.n_params()
    S, B = 160, 2
    x = np.random.default_rng(77).random((B, S, S, 3), dtype=np.float32)
    model = YoloModel(program)
    status = model.load_weights(str(path))
    status.expect_partial()
    det = DetectModel(model, anchors, 80, 100, 0.5, 0.1)
    gb, gc, gs_, gsel, gnv = det.predict(x)
    rb, rc, rs, rsel, rnv = O.detect(program, weights, x, anchors)
    assert _boxes_close(gb, rb) and np.abs(gs_ - rs).max() <= 1e-4
    s2, n2 = O.nms_padded(gb, gs_, 100, 0.5, 0.1)
    assert np.array_equal(s2, gsel) and np.array_equal(n2, gnv)
    _selection_explained((rb, rc, rs, rsel, rnv), (gb, gc, gs_, gsel, gnv))
    # and the file path gives bit for bit what the in-memory path gives (the loader changes no value)
    m2 = YoloModel(program)
    m2.set_weights_dict(weights)
    hb, hc, hs, hsel, hnv = DetectModel(m2, anchors, 80, 100, 0.5, 0.1).predict(x)
    assert np.array_equal(hb, gb) and np.array_equal(hs, gs_) and np.array_equal(hsel, gsel)


@pytest.mark.parametrize("S,B", [(32, 1), (64, 3), (96, 2), (416, 1)])
def test_fused_stem_matches_oracle_and_the_two_launch_form(rt, S, B):
    """conv0 (3x3/1, 3 -> 32) + conv1 (3x3/2, 32 -> 64) as ONE kernel (csrc/conv_stem.hip; reference
    core/parse_model.py:27-52, the stride-2 conv padded top/left only :34-35): conv1's output against the oracle's
    layer-by-layer result within the layer bar, and against the two-launch form (same bar: conv0's summation order
    differs between the two kernels).  Sizes cover one tile per image row (32), borders on every side, several images
    and the real 416 geometry; the fused form must really be the one that ran (conv0 reports no launch of its own)."""
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from oracle import oracle as O
    # backbone.yaml layers 1-4: conv0, conv1, the 1x1 that follows (fp32 plans compute it inside the stem kernel too) and
    # the 3x3 + shortcut that closes the first residual block; heads read the block's output
    p = mini_program(3, [dict(filters=32, size=3), dict(filters=64, size=3, stride=2), dict(filters=32, size=1),
                         dict(filters=64, size=3, shortcut=-3)],
                     [dict(filters=32, size=1), dict(filters=32, size=1), dict(filters=32, size=1)])
    w = synthetic_weights(p, seed=11)
    x = np.random.default_rng(11).random((B, S, S, 3), dtype=np.float32)
    t1 = p.conv_ops()[1].dst
    ref, kept = O.forward(p, w, x, keep={t1})
    xd = _cuda(x)
    outs = {}
    for fused in (True, False):
        net = rt.Net(p)
        net.load_weights(w)
        net.plan(B, S)
        net.set_stem_fusion(fused)
        got = [g.clone() for g in net.forward(xd)]
        ms = net.profile_convs(xd)
        assert (ms[0] == 0.0) == fused, "fused stem did not engage" if fused else "fusion could not be switched off"
        assert (ms[2] == 0.0) == fused, "the 1x1 third layer did not join the stem kernel"
        outs[fused] = got
        for r, g in zip(ref, got):
            g = g.cpu().numpy().reshape(r.shape)
            assert np.abs(g - r).max() <= 2e-5 * max(1.0, float(np.abs(r).max())), (fused, float(np.abs(g - r).max()))
    for a, b in zip(outs[True], outs[False]):
        assert float((a - b).abs().max()) <= 2e-5 * max(1.0, float(b.abs().max()))
    # determinism of the persistent kernel
    net = rt.Net(p)
    net.load_weights(w)
    net.plan(B, S)
    again = net.forward(xd)
    assert all(torch.equal(a, b) for a, b in zip(outs[True], again))
    # keep_activations needs conv0's tensor in HBM: the fusion steps aside and the tensor is readable
    net = rt.Net(p)
    net.load_weights(w)
    net.keep_activations(True)
    net.plan(B, S)
    net.forward(xd)
    c1 = net.read_tensor(t1, B).cpu().numpy()
    assert np.abs(c1 - kept[t1]).max() <= 2e-5 * max(1.0, float(np.abs(kept[t1]).max()))
    assert net.profile_convs(xd)[0] > 0.0


@pytest.mark.parametrize("S,B", [(32, 1), (64, 3), (416, 2)])
def test_fused_stem_bf16_third_layer_bit_identical_to_its_own_launch(rt, S, B):
    """bf16 plans: the 1x1 conv that follows conv1 (64 -> 32, backbone.yaml layer 3; reference core/parse_model.py:27-52) is
    computed by the stem kernel from conv1's staged bf16 tile (phase 3 of conv_stem_bf16).  Same operands, same MFMA
    instruction and k grouping as the stand-alone conv_bf16_mfma launch: stem mode 1 (three layers in one kernel) must equal
    mode 2 (conv0 + conv1 fused, the 1x1 launched on its own) bit for bit on every head, the 1x1 must report no launch of its own
    in mode 1, and both stay within the free-running bf16 bar of the oracle."""
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from yolo_v3_tf2_amd import _lib
    from oracle import oracle as O
    p = mini_program(3, [dict(filters=32, size=3), dict(filters=64, size=3, stride=2), dict(filters=32, size=1),
                         dict(filters=64, size=3, shortcut=-3)],
                     [dict(filters=32, size=1, bn=False, act="linear"), dict(filters=32, size=1, bn=False, act="linear"),
                      dict(filters=64, size=1)])
    w = synthetic_weights(p, seed=13)
    x = np.random.default_rng(13).random((B, S, S, 3), dtype=np.float32)
    ref = O.forward(p, w, x, bf16=True)
    xd = _cuda(x)
    outs = {}
    for mode in (1, 2):
        net = rt.Net(p)
        net.load_weights(w)
        net.plan(B, S, _lib.Y3_DTYPE_BF16)
        net.set_lanes(1)
        net.set_stem_fusion(mode)
        got = [g.clone() for g in net.forward(xd)]
        ms = net.profile_convs(xd)
        assert ms[0] == 0.0, "fused stem did not engage"
        assert (ms[2] == 0.0) == (mode == 1), "the 1x1 third layer: wrong launch structure for this mode"
        outs[mode] = got
        for r, g in zip(ref, got):
            g = g.cpu().numpy().reshape(r.shape)
            scale = max(1.0, float(np.abs(r).max()))
            assert np.abs(g - r).max() <= 8e-3 * scale and np.abs(g - r).mean() <= 4e-4 * scale, \
                (mode, float(np.abs(g - r).max()), float(np.abs(g - r).mean()))
        again = net.forward(xd)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
    assert all(torch.equal(a, b) for a, b in zip(outs[1], outs[2])), "phase 3 differs from the stand-alone 1x1 launch"


@pytest.mark.parametrize("S,B", [(32, 1), (64, 3), (416, 2)])
def test_fused_stem_bf16_matches_oracle_and_the_two_launch_form(rt, S, B):
    """The bf16 form of the fused stem (config 5): conv0 in fp32 arithmetic rounded to bf16 into the LDS patch, conv1 on
    the bf16 matrix cores.  conv1's output feeds three linear 1x1 heads whose fp32 outputs are compared (a) with the
    bf16-emulating oracle under the free-running bar of two bf16 layers (a flipped rounding of one conv0 value moves a
    conv1 sum by ~2^-8/sqrt(288) of its scale; flipped conv1 roundings move a head sum by ~2^-8/sqrt(64)) and (b) with the
    two-launch form of the same plan under the same bar; determinism over repeats."""
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from yolo_v3_tf2_amd import _lib
    from oracle import oracle as O
    p = mini_program(3, [dict(filters=32, size=3), dict(filters=64, size=3, stride=2)],
                     [dict(filters=32, size=1, bn=False, act="linear"), dict(filters=32, size=1, bn=False, act="linear"),
                      dict(filters=64, size=1)])
    w = synthetic_weights(p, seed=12)
    x = np.random.default_rng(12).random((B, S, S, 3), dtype=np.float32)
    ref = O.forward(p, w, x, bf16=True)
    xd = _cuda(x)
    outs = {}
    for fused in (True, False):
        net = rt.Net(p)
        net.load_weights(w)
        net.plan(B, S, _lib.Y3_DTYPE_BF16)
        net.set_lanes(1)
        net.set_stem_fusion(fused)
        got = [g.clone() for g in net.forward(xd)]
        ms = net.profile_convs(xd)
        assert (ms[0] == 0.0) == fused
        outs[fused] = got
        for r, g in zip(ref, got):
            g = g.cpu().numpy().reshape(r.shape)
            scale = max(1.0, float(np.abs(r).max()))
            assert np.abs(g - r).max() <= 4e-3 * scale and np.abs(g - r).mean() <= 2e-4 * scale, \
                (fused, float(np.abs(g - r).max()), float(np.abs(g - r).mean()))
        again = net.forward(xd)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
    for a, b in zip(outs[True], outs[False]):
        scale = max(1.0, float(b.abs().max()))
        assert float((a - b).abs().max()) <= 4e-3 * scale and float((a - b).abs().mean()) <= 2e-4 * scale


@pytest.mark.parametrize("S,B", [(96, 2), (416, 1)])
def test_fused_stem_bf16_conv0_error_bounded_through_identity_heads(rt, S, B):
    """the bf16 fused stem computes conv0 from split bf16 operands (hi*hi + hi*lo + lo*hi: ~2^-16 per product, not
    fp32 arithmetic).  Its effect is bounded DIRECTLY here: conv1's bf16 output is read bit for bit through a 1x1 head with
    identity weights (64 -> 64, linear, zero bias: y = 1.0 * x exactly, fp32 out) from the fused kernel and from the
    one-launch-per-conv form of the same plan.  A conv0 value whose rounding to bf16 flips moves a conv1 sum by ~2^-8 / sqrt(288)
    of its scale, which flips a few percent of conv1's own roundings: every element within ONE bf16 ulp, a bounded fraction
    different at all.  Both forms against the bf16-emulating oracle under the same bar."""
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from yolo_v3_tf2_amd import _lib
    from oracle import oracle as O
    ident = dict(filters=64, size=1, bn=False, act="linear")
    p = mini_program(3, [dict(filters=32, size=3), dict(filters=64, size=3, stride=2)], [ident, ident, ident])
    w = synthetic_weights(p, seed=13)
    for i in (2, 3, 4):
        w[f"conv{i}.w"] = np.eye(64, dtype=np.float32).reshape(1, 1, 64, 64)
        w[f"conv{i}.bias"] = np.zeros(64, np.float32)
    x = np.random.default_rng(13).random((B, S, S, 3), dtype=np.float32)
    ref = O.forward(p, w, x, bf16=True)[0]
    xd = _cuda(x)
    outs = {}
    for fused in (True, False):
        net = rt.Net(p)
        net.load_weights(w)
        net.plan(B, S, _lib.Y3_DTYPE_BF16)
        net.set_lanes(1)
        net.set_stem_fusion(2 if fused else 0)
        outs[fused] = net.forward(xd)[0].cpu().numpy().reshape(ref.shape)
        assert (net.profile_convs(xd)[0] == 0.0) == fused
    scale = float(np.abs(ref).max())
    for name, a, b in (("fused vs two-launch", outs[True], outs[False]), ("fused vs oracle", outs[True], ref),
                       ("two-launch vs oracle", outs[False], ref)):
        d = np.abs(a - b)
        ulp = _bf16_ulp_elem(a, b)
        frac = float((d > 0).mean())
        beyond = float((d > ulp + 1e-5 * scale).mean())     # more than the element's own rounding: a flipped conv0 value upstream
        print(f"stem conv1 output, {name}: {100 * frac:.2f} % of elements differ, {100 * beyond:.3f} % by more than their own ulp, "
              f"max |d| = {d.max() / (2.0 ** -8 * scale):.3f} ulp of the layer's scale")
        # a conv0 value rounded the other way (1 bf16 ulp of ITS magnitude) moves a conv1 sum by |w| * ulp -- an absolute amount
        # however small the element itself is (sums cancel): the element's own rounding + 2^-8 of the layer's scale bounds it
        assert (d <= ulp + 2.0 ** -8 * scale).all(), (name, float(d.max()))
        assert frac <= 0.05 and beyond <= 0.01, (name, frac, beyond)


def test_measure_sclk_reads_a_plausible_clock(rt, program, weights):
    """y3_net_measure_sclk: the in-kernel stamp pair of the fused stem kernel gives a clock between the chip's idle and
    maximum frequency, leaves the results of a forward untouched, and refuses a plan without the stem kernel."""
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(8, 96)
    x = torch.rand((8, 96, 96, 3), device="cuda")
    g = [t.clone() for t in net.forward(x)]
    mhz = net.measure_sclk(x, [torch.empty_like(t) for t in g], forwards=20)
    assert 100.0 < mhz < 2600.0, mhz
    assert all(torch.equal(a, b) for a, b in zip(g, net.forward(x)))
    from yolo_v3_tf2_amd import _lib
    net.plan(8, 96, _lib.Y3_DTYPE_BF16)
    net.set_stem_fusion(False)      # a bf16 plan without the stem kernel has no launch that carries stamps
    with pytest.raises(rt.Y3Error, match="stamps"):
        net.measure_sclk(x, g, forwards=2)


def test_measure_sclk_per_conv_and_timeline(rt, program, weights):
    """y3_net_measure_sclk_conv / _all: every launch of an fp32 plan stamps; the convs inside the fused stem launch do not;
    starts are ordered like the launches and every stamped launch ends after it starts."""
    net = rt.Net(program)
    net.load_weights(weights)
    net.plan(8, 96)
    x = torch.rand((8, 96, 96, 3), device="cuda")
    g = [t.clone() for t in net.forward(x)]
    scratch = [torch.empty_like(t) for t in g]
    mhz, t0, t1 = net.measure_sclk_all(x, scratch, forwards=5)
    n = len(net.conv_ops)
    assert len(mhz) == n
    stamped = [i for i in range(n) if mhz[i] > 0]
    assert 0 not in stamped and 2 not in stamped and 1 in stamped          # conv0 and conv2 run inside conv1's launch
    assert stamped == [1] + list(range(3, n))
    assert all(100.0 < mhz[i] < 2600.0 for i in stamped), mhz
    assert all(t1[i] > t0[i] for i in stamped)
    assert all(t0[a] <= t0[b] for a, b in zip(stamped, stamped[1:]))      # one stream: launches start in program order
    one = net.measure_sclk(x, scratch, forwards=5, conv=stamped[5])
    assert 100.0 < one < 2600.0
    with pytest.raises(rt.Y3Error, match="stamps"):
        net.measure_sclk(x, scratch, forwards=2, conv=0)
    assert all(torch.equal(a, b) for a, b in zip(g, net.forward(x)))       # measurement launches leave no trace


@pytest.mark.parametrize("chunk", [32, 64, 128])
def test_chunk_major_k_order_matches_oracle_and_tap_major(rt, chunk):
    """y3_net_set_k_chunk: the fp32 3x3 convs summed chunk-major (all taps of `chunk` input channels, then the next chunk)
    give the oracle's values within fp32 rounding, like the tap-major order, for stride 1 and 2, with a shortcut, at an
    image size whose tiles straddle rows and images; chunk sizes that do not divide Cin leave the order tap-major."""
    from tests.helpers import mini_program
    from yolo_v3_tf2_amd.weights import synthetic_weights
    from oracle import oracle as O
    p = mini_program(256, [dict(filters=128, size=1), dict(filters=256, size=3, shortcut=-3), dict(filters=384, size=3, stride=2)],
                     [dict(filters=64, size=3), dict(filters=64, size=1), dict(filters=64, size=1)])
    w = synthetic_weights(p, seed=21)
    x = np.random.default_rng(21).standard_normal((3, 14, 14, 256)).astype(np.float32)
    ref = O.forward(p, w, x)
    outs = {}
    for ck in (0, chunk):
        net = rt.Net(p)
        net.load_weights(w)
        net.set_k_chunk(ck)
        net.plan(3, 14)
        outs[ck] = [t.cpu().numpy() for t in net.forward(_cuda(x))]
        torch.cuda.synchronize()
        for r, g in zip(ref, outs[ck]):
            assert np.abs(g.reshape(r.shape) - r).max() <= 2e-5 * max(1.0, float(np.abs(r).max()))
    # the two orders are different summations of the same products: equal to rounding, and (for these sizes) not bit-equal
    assert any(not np.array_equal(a, b) for a, b in zip(outs[0], outs[chunk]))
    with pytest.raises(rt.Y3Error):
        rt.Net(p).set_k_chunk(48)
